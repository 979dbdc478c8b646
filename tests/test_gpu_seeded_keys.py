"""Seeded evaluation keys and input ciphertexts (include/bmi_tfhe.h, csrc/chacha_expand.hip) on the GPU: the masks a server expands
from the 32-byte public key are the words of the numpy ChaCha20 reference (tests/seeded_cases.py), a server built from the seeded
form holds word for word the keys of one built from the full form, and the encrypted inverse runs from a seeded key file on seeded
inputs.  Keys come from the CSPRNG (keygen() without a seed): the seeded forms are refused for anything else."""
import os

import numpy as np
import pytest

import pbs_cases as pc
import seeded_cases as sc

pytestmark = pytest.mark.gpu

# name -> (parameter set with the small dimension cut to n, precision of the plain key, precision of the unrolled key)
SETS = {"default": (lambda tfhe, n: tfhe.default_params(n=n), 48, 42),
        "secure128_torus": (lambda tfhe, n: tfhe.preset_params("secure128_torus", n=n), 46, 40),
        "secure128_torus_wide": (lambda tfhe, n: tfhe.preset_params("secure128_torus_wide", n=n), 44, None)}


def round_key(words, precision):
    """the stored form of key words (csrc/t64_common.hpp round_key_word): half up to a multiple of 2^(64 - precision), wrapping"""
    drop = np.uint64(64 - precision)
    if drop == 0:
        return words
    return ((words + (np.uint64(1) << (drop - np.uint64(1)))) >> drop) << drop


def make_client(name, n, unroll=False):
    from bmi_amd import tfhe
    e = tfhe.Engine(SETS[name][0](tfhe, n))
    if unroll:
        e.set_bsk_unroll(2)
    e.keygen()
    return e


@pytest.fixture(scope="module")
def clients():
    """one CSPRNG client per parameter set at n = 16, shared by the tests that only read it or advance its encryption counter"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = make_client(name, 16)
        return made[name]
    yield get
    for e in made.values():
        e.close()


# ---- ciphertext expansion

@pytest.mark.parametrize("name,first,count", [("default", 0, 0), ("default", 0, 1), ("default", 0, 5), ("default", 0, 300),
                                              ("default", (1 << 32) - 2, 0), ("default", (1 << 32) - 2, 1),
                                              ("default", (1 << 32) - 2, 5), ("default", (1 << 32) - 2, 300),
                                              ("secure128_torus", 0, 3), ("secure128_torus_wide", 0, 3)])
def test_expanded_ciphertext_masks_equal_the_reference(clients, name, first, count):
    """expand_seeded_host on arbitrary bodies: every mask word is the stream's, the body word is the body given - across counters
    whose low 32 bits wrap, rows that are only 8-byte aligned (k N + 1 words) and more than one workgroup"""
    e = clients(name)
    pub = e.export_keys_seeded()[0]
    bodies = np.random.default_rng(first % 97 + count).integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    out = e.expand_seeded_host(first, bodies)
    assert out.shape == (count, e.P.big) and out.dtype == np.uint64
    N = e.P.k * e.P.N
    assert np.array_equal(out[:, N], bodies)
    for i in range(count):
        assert np.array_equal(out[i, :N], sc.row_masks(pub, "enc", first + i, N)), (name, first, i)


def test_device_form_equals_host_form(clients):
    import torch
    from bmi_amd import tfhe
    e = clients("default")
    bodies = np.arange(7, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    want = e.expand_seeded_host(41, bodies)
    dev = torch.device("cuda", e.device)
    d_out = torch.zeros((7, e.P.big), dtype=torch.int64, device=dev)
    d_bodies = torch.from_numpy(bodies.view(np.int64)).to(dev)
    with torch.cuda.device(dev):
        e.expand_seeded(tfhe.SeededCiphertexts(41, d_bodies), d_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize(dev)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)
    d_out.zero_()
    with torch.cuda.device(dev):       # host bodies, device output
        e.expand_seeded(tfhe.SeededCiphertexts(41, bodies), d_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize(dev)
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64), want)


# ---- encryption

def test_seeded_encryption_decrypts_and_shares_the_counter_with_encrypt(clients):
    """expand_seeded(encrypt_seeded(m)) decrypts to m for every 4-bit message with the noise of a fresh encryption: the centred
    phase error of each stays within 6 sigma, sigma = glwe_noise * 2^64 (the Gaussian the body was drawn with; 16 samples beyond 6
    sigma: 3e-8), + 1/2 for the rounding of the noise to a word.  A following encrypt() takes the next counter: its masks are the
    stream's words at that nonce."""
    e = clients("default")
    dl = e.delta_log()
    msgs = np.arange(-8, 8)
    s = e.encrypt_seeded(msgs, dl)
    assert len(s) == 16 and s.bodies.dtype == np.uint64
    ct = e.expand_seeded(s)
    assert list(e.decrypt(ct, dl)) == list(msgs)
    err = (e.phase(ct) - (msgs.astype(np.int64) << dl).view(np.uint64)).view(np.int64)
    sigma = e.P.glwe_noise * 2.0 ** 64
    print(f"\nseeded encryption: max |phase error| = {np.abs(err).max()} = {np.abs(err).max() / sigma:.2f} sigma")
    assert np.abs(err).max() <= 6 * sigma + 0.5
    assert np.abs(err).max() > 0          # noise was added
    pub = e.export_keys_seeded()[0]
    full = e.encrypt(msgs[:3], dl)
    N = e.P.k * e.P.N
    for i in range(3):
        assert np.array_equal(full[i, :N], sc.row_masks(pub, "enc", s.first_counter + 16 + i, N))
    again = e.encrypt_seeded(msgs[:2], dl)
    assert again.first_counter == s.first_counter + 19


# ---- key round trip

def check_round_trip(name, n, unroll):
    """client (CSPRNG keys) -> seeded export -> server; against a second server built from the full export"""
    from bmi_amd import tfhe
    P = SETS[name][0](tfhe, n)
    prec = SETS[name][2 if unroll else 1]
    client = make_client(name, n, unroll)
    server, full = tfhe.Engine(SETS[name][0](tfhe, n)), tfhe.Engine(SETS[name][0](tfhe, n))
    try:
        assert client.bsk_precision == prec
        pub, bsk_body, ksk_body = client.export_keys_seeded()
        _, _, bsk, ksk = client.export_keys(secret=False)
        assert np.array_equal(bsk_body, bsk[:, :, 1, :]) and np.array_equal(ksk_body, ksk[:, :, n])
        for e in (server, full):
            if unroll:
                e.set_bsk_unroll(2)
        server.import_keys_seeded(pub, bsk_body, ksk_body)
        full.import_keys(None, None, bsk, ksk)
        if unroll:
            bsk3 = client.export_bsk_unrolled()
            body3 = client.export_bsk_unrolled_seeded()
            assert np.array_equal(body3, bsk3[:, :, :, 1, :])
            server.import_bsk_unrolled_seeded(body3)
            full.import_bsk_unrolled(bsk3)
            assert np.array_equal(server.export_bsk_unrolled(), bsk3)
        _, _, s_bsk, s_ksk = server.export_keys(secret=False)
        assert np.array_equal(s_bsk, bsk) and np.array_equal(s_ksk, ksk)
        assert server.eval_key_fingerprint() == client.eval_key_fingerprint() == full.eval_key_fingerprint()
        assert server.key_bytes() == client.key_bytes() == full.key_bytes()
        # a sample of mask rows against the reference: first and last row of each key; a keyswitch row of n = 15 ends in a partial block
        rows = (P.k + 1) * P.bs_levels
        for ir in (0, 1, n * rows - 1):
            assert np.array_equal(s_bsk[ir // rows, ir % rows, 0], round_key(sc.row_masks(pub, "bsk", ir, P.N), prec)), ir
        for jr in (0, 1, P.k * P.N * P.ks_levels - 1):
            assert np.array_equal(s_ksk[jr // P.ks_levels, jr % P.ks_levels, :n], sc.row_masks(pub, "ksk", jr, n)), jr
        if unroll:
            flat3 = server.export_bsk_unrolled().reshape(-1, 2, P.N)
            for ir in (0, flat3.shape[0] - 1):
                assert np.array_equal(flat3[ir, 0], round_key(sc.row_masks(pub, "bsk3", ir, P.N), prec)), ir
        # the same bootstraps, word for word
        bits = 4
        dl = client.delta_log(bits)
        table = np.random.default_rng(n).integers(-8, 8, 1 << bits)
        ct = client.encrypt(np.array([-8, -3, 0, 5, 7]), dl)
        outs = [e.pbs_host(ct, np.full(5, e.lut_register(table, bits, dl), np.uint32)) for e in (server, full)]
        assert np.array_equal(outs[0], outs[1])
    finally:
        for e in (client, server, full):
            e.close()


@pytest.mark.parametrize("name,n", [("default", 16), ("default", 15), ("secure128_torus", 16), ("secure128_torus_wide", 16)])
def test_seeded_key_round_trip(name, n):
    """n = 16: keyswitch rows of pitch 17 in whole blocks (only every other row 16-byte aligned); n = 15: pitch 16, the last block
    partial; N = 2048 at 46 bits and N = 4096 at 44 bits"""
    check_round_trip(name, n, unroll=False)


@pytest.mark.parametrize("name,n", [("default", 16), ("default", 15), ("secure128_torus", 16), ("secure128_torus", 15)])
def test_seeded_unrolled_key_round_trip(name, n):
    """the unrolled key (domain BSK3_MASK) at 42 bits (N = 1024) and 40 bits (N = 2048); n = 15: the last pair is completed by a zero bit"""
    check_round_trip(name, n, unroll=True)


# ---- full size

def test_full_size_server_from_a_seeded_key_file(tmp_path):
    """the default set at n = 630: a server loaded from the seeded key file bootstraps every 4-bit message to its table value, and
    the file is smaller than 0.31 x the full one (include/bmi_tfhe.h: (30,965,760 + 65,536) / (61,931,520 + 41,353,216) = 0.300;
    both files are uncompressed .npz)"""
    from bmi_amd import tfhe
    client, server = tfhe.Engine(), tfhe.Engine()
    try:
        client.keygen()
        client.save_keys(tmp_path / "full.npz", secret=False)
        client.save_keys(tmp_path / "seeded.npz", secret=False, seeded=True)
        size_full, size_seeded = os.path.getsize(tmp_path / "full.npz"), os.path.getsize(tmp_path / "seeded.npz")
        print(f"\nkey files: full {size_full} B, seeded {size_seeded} B, ratio {size_seeded / size_full:.4f}")
        assert size_seeded < 0.31 * size_full
        with np.load(tmp_path / "seeded.npz") as z:
            assert sorted(z.files) == ["bsk_body", "bsk_precision", "ksk_body", "params", "pub_key"]
        assert server.load_keys(tmp_path / "seeded.npz") is False
        dl = client.delta_log()
        table = np.array([(3 * m * m + m) % 16 - 8 for m in range(-8, 8)])
        msgs = np.arange(-8, 8)
        out = server.pbs_host(client.encrypt(msgs, dl), np.full(16, server.lut_register(table, 4, dl), np.uint32))
        assert list(client.decrypt(out, dl)) == [int(table[m + 8]) for m in msgs]
        assert server.eval_key_fingerprint() == client.eval_key_fingerprint()
        with pytest.raises(tfhe.BmiError, match="evaluation-only"):
            server.encrypt(msgs, dl)
        with pytest.raises(tfhe.BmiError, match="evaluation keys only"):
            client.save_keys(tmp_path / "refused.npz", secret=True, seeded=True)
    finally:
        client.close()
        server.close()


# ---- refusals, each by its text

def test_refusals(clients):
    from bmi_amd import tfhe
    det = tfhe.Engine(tfhe.default_params(n=16))
    imp = tfhe.Engine(tfhe.default_params(n=16))
    bare = tfhe.Engine(tfhe.default_params(n=16))
    try:
        det.keygen(0x5EED)
        with pytest.raises(tfhe.BmiError, match="deterministic test keys"):
            det.export_keys_seeded()
        with pytest.raises(tfhe.BmiError, match="deterministic test keys"):
            det.encrypt_seeded(np.array([1]), det.delta_log())
        sk_small, sk_big, bsk, ksk = clients("default").export_keys()
        imp.import_keys(sk_small, sk_big, bsk, ksk)
        with pytest.raises(tfhe.BmiError, match="keys loaded by bmi_import_keys"):
            imp.export_keys_seeded()
        with pytest.raises(tfhe.BmiError, match="keys loaded by bmi_import_keys"):
            imp.encrypt_seeded(np.array([1]), imp.delta_log())
        with pytest.raises(tfhe.BmiError, match="keys loaded by bmi_import_keys"):
            imp.expand_seeded_host(0, np.zeros(1, np.uint64))
        with pytest.raises(tfhe.BmiError, match="no keys"):
            bare.export_keys_seeded()
        with pytest.raises(tfhe.BmiError, match="no keys"):
            bare.expand_seeded_host(0, np.zeros(1, np.uint64))
        bare.set_bsk_unroll(2)
        with pytest.raises(tfhe.BmiError, match="preceding bmi_import_keys_seeded"):
            bare.import_bsk_unrolled_seeded(np.zeros(bare.unrolled_key_shape()[:3] + (bare.P.N,), np.uint64))
        imp.set_bsk_unroll(2)      # derives an unrolled key from the imported secrets: still no seeded form, and no public key imported
        with pytest.raises(tfhe.BmiError, match="keys loaded by bmi_import_keys"):
            imp.export_bsk_unrolled_seeded()
        with pytest.raises(tfhe.BmiError, match="preceding bmi_import_keys_seeded"):
            imp.import_bsk_unrolled_seeded(np.zeros(imp.unrolled_key_shape()[:3] + (imp.P.N,), np.uint64))
    finally:
        for e in (det, imp, bare):
            e.close()
    for q_bits in (49, 64):
        field = tfhe.Engine(tfhe.default_params(q_bits=q_bits, n=16))
        try:
            field.keygen()
            with pytest.raises(tfhe.BmiError, match="rejection-sampled"):
                field.export_keys_seeded()
            with pytest.raises(tfhe.BmiError, match="rejection-sampled"):
                field.encrypt_seeded(np.array([1]), field.delta_log())
            P = field.P
            with pytest.raises(tfhe.BmiError, match="rejection-sampled"):
                field.import_keys_seeded(np.zeros(8, np.uint32), np.zeros((P.n, (P.k + 1) * P.bs_levels, P.N), np.uint64),
                                         np.zeros((P.k * P.N, P.ks_levels), np.uint64))
        finally:
            field.close()


# ---- application

def test_encrypted_inverse_from_a_seeded_key_file_on_seeded_inputs(tmp_path):
    """the golden 2x2: the client holds the secrets, the server is loaded from the seeded key file, the input travels as
    SeededCiphertexts (8 bytes per ciphertext), the result decrypts to the reference's digits; evaluate_many on two seeded inputs"""
    from bmi_amd import tfhe
    from bmi_amd.main import EncryptedMatrixInversion
    c = pc.golden_inverse("baseline_n2_len20_ints8")
    ce, se = tfhe.Engine(), tfhe.Engine()
    try:
        client = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=ce)
        client.keygen()
        ce.save_keys(tmp_path / "eval.npz", secret=False, seeded=True)
        se.load_keys(tmp_path / "eval.npz")
        server = EncryptedMatrixInversion(2, None, 2, c["len"], c["ints"], False, False, engine=se)
        q, s = client.quantize(np.array(c["M"]).reshape(2, 2))
        enc = client.encrypt(q, s, seeded=True)
        assert isinstance(enc, tfhe.SeededCiphertexts) and len(enc) == 4 * (c["len"] + 1) and enc.bodies.nbytes == 8 * len(enc)
        assert client.decrypt(server.evaluate(enc)).tolist() == c["out"]
        second = client.encrypt(q, s, seeded=True)
        assert second.first_counter == enc.first_counter + len(enc)
        many = server.evaluate_many([enc, second])
        assert many.shape[0] == 2
        for r in many:
            assert client.decrypt(r).tolist() == c["out"]
    finally:
        ce.close()
        se.close()
