// Host side of libbmi_tfhe.so: the C ABI of include/bmi_tfhe.h — context, deterministic key
// generation, encryption / decryption, LUT (test-polynomial) construction and the batch entry points
// that launch the HIP kernels of bmi_kernels.hip.  No CPU fallback exists for the PBS path: every
// batch call needs a HIP device and fails loudly without one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/bmi_tfhe.h"
#include "host_crypto.hpp"
#include "key_set.hpp"
#include "bmi_internal.hpp"
#include "field49.hpp"
#include "ntt_wave.hpp"
#include "ntt_half_f64.hpp"
#include "ntt_wave_f64.hpp"
#include "fft_half_f64.hpp"
#include "fft_wave_f64.hpp"
#include "fft_eighth_f64.hpp"
#include "fft_quarter_f64.hpp"
#include "t64_common.hpp"

using gl::i64;
using gl::u64;
// The library's cryptography - generators, key rows, encryption, phase, decoding - is host_crypto.hpp, and the key set with the host
// half of the entry points (which libbmi_client.so exports too) key_set.hpp; this file holds the context, the order of its refusals,
// and does the device work.
using namespace hc;
static_assert(GOLDILOCKS_P == gl::P && FIELD49_Q == f49::Q, "host_crypto.hpp states the moduli of goldilocks.hpp and field49.hpp");
static_assert(MAX_LWE_N == BMI_MAX_LWE_N, "key_set.hpp states the largest n of bmi_internal.hpp");

namespace {

// One device allocation, owned: freed when the buffer is destroyed, reset or assigned over.  Move-only.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
    DevBuf &operator=(DevBuf &&o) noexcept {
        reset();
        std::swap(p_, o.p_);
        std::swap(bytes_, o.bytes_);
        return *this;
    }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t bytes) {   // replaces the buffer held (if any)
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e == hipSuccess) bytes_ = bytes;
        else p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        bytes_ = 0;
    }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
    bool empty() const { return !p_; }

  private:
    T *p_ = nullptr;
    size_t bytes_ = 0;
};

using rotplan::Copy;
using rotplan::Rot;
using rotplan::Table;

}  // namespace

// The key set (key_set.hpp: parameters, keys, generators, the flags that decide a word) and the device that evaluates under it
struct bmi_ctx : hc::KeySet {
    const FieldOps *ops = nullptr;
    int device = 0;
    uint32_t ks_stride = 0;
    hipStream_t stream = nullptr;  // the context's own stream (host-buffer entry points)
    int bsk_limbs() const { return t64::limbs_of(bsk_prec); }
    // Tables (bmi_ctx_create), one per rotplan::Table, where the kernels that read each are listed; empty where the context's
    // modulus and N have no such kernel (rotplan::context_tables).
    DevBuf<void> tables[(int)Table::COUNT];
    DevWords table(Table t) const { return {t == Table::none ? nullptr : tables[(int)t].get()}; }
    DevBuf<u64> luts;           // BMI_LUT_CAP test polynomials of N words (49-bit field: centred doubles) - every blind rotation
    // The bootstrap key on the device, one buffer per layout (rotplan::Copy, with its conversion and the kernel that reads it).  A
    // copy exists where its kernel is selectable on the context (upload_eval_keys; the torus exact-transform pair when first chosen:
    // rotplan::on_demand_copies).  A buffer that is not empty holds a whole copy (build_key_copy).  Replaced with the key set.
    DevBuf<void> copies[(int)Copy::COUNT];
    void drop_copies(bool unrolled) {   // the copies of the plain key, or those of the unrolled key
        for (int k = 0; k < (int)Copy::COUNT; k++)
            if (rotplan::row((Copy)k).unrolled == unrolled) copies[k].reset();
    }
    // (the unrolled key: its device copy in the layout of the context's unrolled kernel, upload_bsk3)
    bool wide() const { return N == 2048; }
    bool quad() const { return N == 4096; }
    DevBuf<u64> ksk_padded, ks_bias;   // keyswitch key, rows padded to ks_stride words, and its bias vector - keyswitch
    DevBuf<signed char> ks_limbs;      // the keyswitch key as ops->ks_limbs limbs in MFMA operand order - keyswitch_mfma
    // compression of output ciphertexts (2^64 torus; lwe_pack.hip): the device copy of the packing keyswitch key, in the host copy's
    // layout, and the product's bias vector [2N]
    DevBuf<u64> pksk_dev, pk_bias;
    DevBuf<u64> sk_mask;               // the big SECRET key as big_n / 64 words of bits, built on first use (ensure_sk_mask), zeroed and
                                       // dropped with the key set (drop_sk_mask) - lwe_phase
    uint32_t n_luts = 0, lut_cap = 0;
    std::vector<std::vector<u64>> luts_host;
    // 2^64 torus, shared rotations (glwe_lookup.hip): per table the sparse factor P_f = (1 - X) TV_f / 2^scale as (position,
    // difference) pairs, filled at registration.  head[id] = {entries, scale}; entries = NO_SPARSE where the table has more than
    // BMI_SPARSE_CAP boxes, WIDE_DIFFERENCE where two neighbouring boxes differ by more than an int32 holds (neither can share a
    // rotation: the kernel counts any value above BMI_SPARSE_CAP as no entries); a base polynomial (bmi_lut_register_base) is
    // {1, unit}: P = 1.
    static constexpr uint32_t NO_SPARSE = 0xFFFFFFFFu, WIDE_DIFFERENCE = 0xFFFFFFFEu;
    DevBuf<uint2> sparse_head;         // [BMI_LUT_CAP]
    DevBuf<int2> sparse;               // [BMI_LUT_CAP][BMI_SPARSE_CAP]
    std::vector<uint2> sparse_head_host;
    uint32_t base_id_of_unit[64] = {};   // id + 1 of the base polynomial registered for a unit, 0 = none yet
    // growable device scratch (grow)
    DevBuf<u64> glwe;                  // accumulators of bmi_pbs_shared_batch ([groups][2 k N])
    DevBuf<u64> small;                 // keyswitched ciphertexts of bmi_pbs_batch / bmi_pbs_shared_batch
    DevBuf<unsigned char> arena;       // every region of a host-buffer form's call (Stage)
    DevBuf<unsigned __int128> ks_partial;   // partial sums of the sliced scalar keyswitch
    DevBuf<signed char> ks_digits;     // matrix-core keyswitch: digit matrix ...
    DevBuf<int> ks_sums;               // ... and int32 sums
    DevBuf<uint32_t> pk_digits;        // compression: digit matrix of a slice ...
    DevBuf<u64> pk_T, pk_acc;          // ... its products [slice][2N], and the block's accumulator [2N]
    int variant = 0;
    uint32_t lat_threshold = 0;    // auto dispatch: the latency kernels up to this batch size (rotplan::initial_settings)
    int ks_variant = 0;  // 0 = auto (matrix cores when the shape allows), 1 = scalar kernel
    uint32_t modswitch = 0;   // 0 = the rotation kernels' own rounding, 1 = centred (bmi_set_modswitch): bmi_pbs_batch / _shared_batch run
                              // k_modswitch_centre on the scratch small ciphertexts between the keyswitch and the rotation
    bool ks_mfma_ok = false;
};

namespace {

// A context as rotation_plan.hpp takes it: its shape, its settings and what it holds.  Which kernel runs, which key copies get
// built and what the setters accept is decided there, from these three; the entry points below act on the answers.
rotplan::Settings settings_of(const bmi_ctx *c) { return {c->bsk_prec, c->bsk_prec_explicit, c->unroll, c->variant, c->lat_threshold}; }
// (the one place where a buffer's presence is read as a fact about the context)
rotplan::Held held_of(const bmi_ctx *c) {
    rotplan::Held h{0, c->have_keys, c->have_bsk3};
    for (int k = 0; k < (int)Copy::COUNT; k++)
        if (!c->copies[k].empty()) h.copies |= rotplan::bit((Copy)k);
    return h;
}
#define HIP_OK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e__ = (call);                                                                       \
        if (e__ != hipSuccess)                                                                         \
            return fail(ctx, -2, std::string(#call) + ": " + hipGetErrorString(e__));                  \
    } while (0)

// a new device buffer holding the `count` host words at src
template <class T>
hipError_t upload(DevBuf<T> &dst, const T *src, size_t count) {
    const hipError_t e = dst.alloc(count * sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(dst.get(), src, count * sizeof(T), hipMemcpyHostToDevice);
}

// Grows a device scratch buffer to at least max(need, floor_bytes) bytes; never shrinks.  Queued work may still read the old
// buffer: a growth synchronises the device before freeing it.
template <class T>
int grow(bmi_ctx *c, DevBuf<T> &b, size_t need, size_t floor_bytes) {
    if (need <= b.bytes()) return 0;
    if (!b.empty()) HIP_OK(c, hipDeviceSynchronize());
    HIP_OK(c, b.alloc(std::max(need, floor_bytes)));
    return 0;
}
// What a launcher returned (a hipError_t as an int) -> the entry point's result: 0, or -2 and "<what><the error's name>"
int launched(const bmi_ctx *c, const char *what, int rc) {
    return rc ? fail(c, -2, std::string(what) + hipGetErrorString((hipError_t)rc)) : 0;
}

// The device side of one host-buffer form's call.  The entry point checks its arguments and the context's state, names its regions
// - each a count of elements of one type that is uploaded from a host pointer, filled with zeros, downloaded to a host pointer at the
// end, or several of these - and passes the device-pointer form to run().  All regions lie in the context's one arena, each from a
// 256-byte boundary; the arena grows before anything is queued (at most one device synchronisation per call, none once it holds
// the largest call so far).  Everything is queued on the context's stream, and run() returns only after that stream has drained,
// whatever refused or failed in between: no caller's array and no local variable is still in reach of a queued copy.
struct Stage {
    template <class T>
    struct Ref { int i; };   // a region, and through operator[] its device pointer (inside run())
    struct Region {
        size_t at, bytes;
        const void *up;
        void *down;
        bool zero;
    };
    Region regions[6];   // (the shared look-ups name five)
    int n = 0;
    size_t total = 0;
    unsigned char *base = nullptr;
    static size_t aligned(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

    template <class T>
    Ref<T> region(size_t count, const T *up, T *down, bool zero = false) {
        regions[n] = Region{total, count * sizeof(T), up, down, zero};
        total += aligned(count * sizeof(T));
        return {n++};
    }
    template <class T>
    Ref<T> upload(const T *from, size_t count) { return region<T>(count, from, nullptr); }
    template <class T>
    Ref<T> download(T *to, size_t count) { return region<T>(count, nullptr, to); }
    template <class T>
    T *operator[](Ref<T> r) const { return (T *)(base + regions[r.i].at); }

    template <class Form>
    int queue(bmi_ctx *c, Form device_form) const {
        for (int i = 0; i < n; i++) {
            const Region &r = regions[i];
            if (r.zero && r.bytes) HIP_OK(c, hipMemsetAsync(base + r.at, 0, r.bytes, c->stream));
            if (r.up && r.bytes) HIP_OK(c, hipMemcpyAsync(base + r.at, r.up, r.bytes, hipMemcpyHostToDevice, c->stream));
        }
        if (int rc = device_form()) return rc;
        for (int i = 0; i < n; i++)
            if (regions[i].down && regions[i].bytes)
                HIP_OK(c, hipMemcpyAsync(regions[i].down, base + regions[i].at, regions[i].bytes, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    template <class Form>
    int run(bmi_ctx *c, Form device_form) {
        HIP_OK(c, hipSetDevice(c->device));
        // the floor, held from the first call on (an empty call has pointers too): bmi_pbs_batch_host of 256 ciphertexts
        const size_t floor_bytes = 2 * aligned((size_t)256 * (c->big_n + 1) * sizeof(u64)) + aligned(256 * sizeof(uint32_t));
        if (int rc = grow(c, c->arena, std::max(total, floor_bytes), 0)) return rc;
        base = c->arena.get();
        const int rc = queue(c, device_form);
        const hipError_t drained = hipStreamSynchronize(c->stream);   // the one way out once a copy may be queued
        if (rc || drained == hipSuccess) return rc;   // (the first error stands)
        return fail(c, -2, std::string("hipStreamSynchronize(c->stream): ") + hipGetErrorString(drained));
    }
};

// The device copy of the big secret key (bmi_phase_batch / bmi_decrypt_batch): bit x % 64 of word x / 64 is key bit x.
int ensure_sk_mask(bmi_ctx *c) {
    if (!c->sk_mask.empty()) return 0;
    std::vector<u64> mask(c->big_n / 64, 0);
    for (uint32_t x = 0; x < c->big_n; x++) mask[x >> 6] |= (c->sk_big[x] & 1) << (x & 63);
    const hipError_t e = upload(c->sk_mask, mask.data(), mask.size());
    if (e != hipSuccess) {
        c->sk_mask.reset();
        return fail(c, -2, std::string("uploading the secret-key mask: ") + hipGetErrorString(e));
    }
    return 0;
}
// ... overwritten with zeros and freed when the key set is replaced or the context destroyed (queued kernels may still read it:
// the device is synchronised first)
void drop_sk_mask(bmi_ctx *c) {
    if (c->sk_mask.empty()) return;
    (void)hipDeviceSynchronize();
    (void)hipMemset(c->sk_mask.get(), 0, c->sk_mask.bytes());
    (void)hipDeviceSynchronize();
    c->sk_mask.reset();
}
// a compression key belongs to the key set it was made for: gone with it (queued kernels may still read it)
// new_key_set: the streams are new as well (or will never be read again): the shape bmi_compression_keygen is held to is forgotten
void drop_compression_key(bmi_ctx *c, bool new_key_set) {
    if (!c->pksk_dev.empty()) (void)hipDeviceSynchronize();
    forget_compression_key(c, new_key_set);
    c->pksk_dev.reset();
    c->pk_bias.reset();
}
// keyswitched ciphertexts of a batch (room for 1,024 at least)
int ensure_small(bmi_ctx *c, size_t count) {
    const size_t w = (size_t)(c->P.n + 1) * sizeof(u64);
    return grow(c, c->small, count * w, 1024 * w);
}
constexpr size_t KS_PARTIAL_BYTES = (size_t)96 << 20;  // covers every split configuration (<= 1024 workgroups x 8 ciphertexts)

// Twiddle tables of the wave NTT as canonical integers mod q: W1[k1][l] = psi^(l (2 k1 + 1)),
// W1I = psi^-(..) / N, W2[v][t] = (psi^32)^(t v), W2I its inverse (layout shared by both fields).
std::vector<u64> build_twiddles(const Fq &f, u64 psi, u64 psi_inv, u64 n_inv) {
    using namespace nttw;
    std::vector<u64> tw(TW_WORDS);
    for (int k1 = 0; k1 < 16; k1++)
        for (int l = 0; l < 64; l++) {
            const u64 e = (u64)l * (2 * k1 + 1);
            tw[TW_W1 + k1 * 64 + l] = f.pow(psi, e);
            tw[TW_W1I + k1 * 64 + l] = f.mul(f.pow(psi_inv, e), n_inv);
        }
    const u64 w64 = f.pow(psi, 32), w64i = f.pow(psi_inv, 32);
    for (int v = 0; v < 16; v++)
        for (int t = 0; t < 4; t++) {
            tw[TW_W2 + v * 4 + t] = f.pow(w64, (u64)t * v);
            tw[TW_W2I + v * 4 + t] = f.pow(w64i, (u64)t * v);
        }
    return tw;
}

std::vector<double> to_centred_doubles(const std::vector<u64> &v) {
    std::vector<double> d(v.size());
    for (size_t i = 0; i < v.size(); i++) d[i] = f49::to_f(v[i]);
    return d;
}

// Tables of the two-wave half transform (ntt_half_f64.hpp, tools/ntt_half_model.py), canonical integers mod q
std::vector<u64> build_twiddles_half(const Fq &f, u64 psi, u64 psi_inv) {
    using namespace ntth;
    std::vector<u64> tw(HT_WORDS);
    const u64 inv1024 = f.pow(1024 % f.q, f.q - 2);
    for (int k1 = 0; k1 < 8; k1++)
        for (int l = 0; l < 64; l++) {
            const u64 e = (u64)2 * (2 * k1 + 1) * l;
            tw[HT_W1 + k1 * 64 + l] = f.pow(psi, e);
            tw[HT_W1I + k1 * 64 + l] = f.mul(f.pow(psi_inv, e), inv1024);
        }
    for (int k2a = 0; k2a < 8; k2a++)
        for (int l0 = 0; l0 < 8; l0++) {
            tw[HT_W2 + k2a * 8 + l0] = f.pow(psi, (u64)32 * l0 * k2a);
            tw[HT_W2I + k2a * 8 + l0] = f.pow(psi_inv, (u64)32 * l0 * k2a);
        }
    for (int reg = 0; reg < 8; reg++)
        for (int lane = 0; lane < 64; lane++) {
            const u64 e = (u64)2 * kk_of(lane, reg) + 1;
            tw[HT_T + reg * 64 + lane] = f.pow(psi, e);
            tw[HT_TI + reg * 64 + lane] = f.pow(psi_inv, e);
        }
    return tw;
}

// N = 2048: T[reg * 64 + lane] = psi_4096^(2 kk + 1) at the evaluation slot (lane, reg) of the 1024-point wave transform
// (kk = k1 + 16 (4 vl + g) + 256 s for lane 4 k1 + g, register 4 vl + s), then the inverses.
std::vector<u64> build_twiddles_wide(const Fq &f) {
    const u64 psi4096 = f.pow(f49::GEN, (f.q - 1) / 4096), inv = f.pow(psi4096, f.q - 2);
    std::vector<u64> tw(2048);
    for (int reg = 0; reg < 16; reg++)
        for (int lane = 0; lane < 64; lane++) {
            const u64 kk = (u64)(lane >> 2) + 16 * (4 * (reg >> 2) + (lane & 3)) + 256 * (reg & 3);
            tw[reg * 64 + lane] = f.pow(psi4096, 2 * kk + 1);
            tw[1024 + reg * 64 + lane] = f.pow(inv, 2 * kk + 1);
        }
    return tw;
}

// N = 4096: T_j[reg * 64 + lane] = psi_8192^((2 kk + 1) j) for j = 1, 2, 3, then the three inverse tables
std::vector<u64> build_twiddles_quad(const Fq &f) {
    const u64 psi = f.pow(f49::GEN, (f.q - 1) / 8192), inv = f.pow(psi, f.q - 2);
    std::vector<u64> tw(6 * 1024);
    for (int j = 1; j <= 3; j++)
        for (int reg = 0; reg < 16; reg++)
            for (int lane = 0; lane < 64; lane++) {
                const u64 kk = (u64)(lane >> 2) + 16 * (4 * (reg >> 2) + (lane & 3)) + 256 * (reg & 3);
                tw[(j - 1) * 1024 + reg * 64 + lane] = f.pow(psi, (2 * kk + 1) * j);
                tw[(3 + j - 1) * 1024 + reg * 64 + lane] = f.pow(inv, (2 * kk + 1) * j);
            }
    return tw;
}

// Builds a device buffer of `bytes` bytes: fresh (launch(buffer) fills it on the context's stream), and moved into dst only once
// the launch and the stream synchronisation have succeeded, so that a buffer that is not empty is whole.
template <class T, class Launch>
int build_copy(bmi_ctx *c, DevBuf<T> &dst, size_t bytes, const char *what, Launch launch) {
    DevBuf<T> fresh;
    HIP_OK(c, fresh.alloc(bytes));
    if (launch(fresh.get())) return fail(c, -2, std::string(what) + " launch failed");
    HIP_OK(c, hipStreamSynchronize(c->stream));
    dst = std::move(fresh);
    return 0;
}

// How each kind of key copy is built, in the order of rotplan::Copy: its conversion launcher and what a failure is reported as
// (the tables the launcher reads are in the copy's row).  paired: the slot order of the 49-bit unrolled kernel.
struct Converter {
    int (*launch)(const KeyConv &);
    const char *what;
    bool paired;
};
const char *const U_LAT = "bsk_to_lat (unrolled key)";
const Converter CONVERTERS[] = {
    {bmi::launch_bsk_to_ntt, "bsk_to_ntt", false},              // ntt_gl
    {bmi49::launch_bsk_to_ntt, "bsk_to_ntt", false},            // ntt49
    {bmi49::launch_bsk_to_lat, "bsk_to_lat", false},            // lat49
    {bmi49::launch_bsk_to_wide, "bsk_to_wide", false},          // wide49
    {bmi49::launch_bsk_to_quad, "bsk_to_quad", false},          // quad49
    {bmit::launch_bsk_to_limbs, "bsk_to_limbs", false},         // exact
    {bmit::launch_bsk_to_lat, "bsk_to_lat (torus)", false},     // exact_lat
    {bmit::launch_bsk_to_fft, "bsk_to_fft (torus)", false},     // fft
    {bmit::launch_bsk_to_latf, "bsk_to_latf (torus)", false},   // fft_lat
    {bmit::launch_bsk_to_wide, "bsk_to_wide (torus)", false},   // wide
    {bmit::launch_bsk_to_wide2, "bsk_to_wide2 (torus)", false}, // wide2
    {bmit::launch_bsk_to_quad, "bsk_to_quad (torus)", false},   // quad
    {bmi49::launch_bsk_to_lat, U_LAT, true},                    // u_lat49
    {bmi49::launch_bsk_to_wide, U_LAT, false},                  // u_wide49
    {bmit::launch_bsk_to_lat, U_LAT, false},                    // u_exact_lat
    {bmit::launch_bsk_to_latf, U_LAT, false},                   // u_fft_lat
    {bmit::launch_bsk_to_wide, "bsk_to_wide (unrolled key)", false},   // u_wide
};
static_assert(sizeof(CONVERTERS) / sizeof(CONVERTERS[0]) == (size_t)Copy::COUNT, "one converter per key copy");

// std_polys = the `polys` standard-domain polynomials of the plain (Copy::ntt_gl .. quad) or the unrolled key (Copy::u_*) on the device
int build_key_copy(bmi_ctx *c, Copy kind, const u64 *std_polys, uint32_t polys, size_t bytes) {
    const Converter &cv = CONVERTERS[(int)kind];
    const rotplan::CopyRow &row = rotplan::row(kind);
    return build_copy(c, c->copies[(int)kind], bytes, cv.what, [&](void *d) {
        return cv.launch(KeyConv{std_polys, d, {c->table(row.tab[0]), c->table(row.tab[1])}, polys, c->bsk_prec, cv.paired, c->stream});
    });
}

// Builds those of the copies `kinds` (bits of rotplan::Copy) of the standard-domain key `std_key` (host words) that the context
// does not hold yet, in the order of the enumeration.  The plan names the copies: rotplan::plain_copies for a new key set,
// on_demand_copies for a kernel that auto dispatch never runs, unrolled_copies for the unrolled key.
int build_copies(bmi_ctx *c, uint32_t kinds, const std::vector<u64> &std_key) {
    kinds &= ~held_of(c).copies;
    if (!kinds) return 0;
    DevBuf<u64> d_std;
    HIP_OK(c, upload(d_std, std_key.data(), std_key.size()));
    const uint32_t polys = (uint32_t)(std_key.size() / c->N);
    const size_t bytes = d_std.bytes() * (c->t64() ? c->bsk_limbs() : 1);
    for (int k = 0; k < (int)Copy::COUNT; k++)
        if (kinds & rotplan::bit((Copy)k))
            if (int rc = build_key_copy(c, (Copy)k, d_std.get(), polys, bytes)) return rc;
    return 0;
}

// Evaluation keys (host copies in c->bsk_std / c->ksk) -> device: bootstrap key (in the layout of every kernel selectable on the
// context: rotplan::plain_copies), keyswitch key in word form (+ bias vector) and in limb form.
int upload_eval_keys(bmi_ctx *c) {
    const bmi_params &P = c->P;
    const uint32_t n = P.n, N = c->N, k = P.k, lk = P.ks_levels;
    round_eval_keys(c);   // (the key at the context's precision IS the key from here on)
    c->drop_copies(false);   // the copies of the previous key set
    c->drop_copies(true);
    if (int rc = build_copies(c, rotplan::plain_copies(shape_of(P), c->bsk_prec), c->bsk_std)) return rc;
    const size_t ksk_rows = (size_t)k * N * lk;
    HIP_OK(c, c->ksk_padded.alloc(ksk_rows * c->ks_stride * sizeof(u64)));
    HIP_OK(c, hipMemset(c->ksk_padded.get(), 0, c->ksk_padded.bytes()));
    HIP_OK(c, hipMemcpy2D(c->ksk_padded.get(), c->ks_stride * sizeof(u64), c->ksk.data(), (n + 1) * sizeof(u64),
                          (n + 1) * sizeof(u64), ksk_rows, hipMemcpyHostToDevice));
    // bias vector of the unsigned-digit keyswitch: (B/2) * sum_rows ksk[row][col]
    {
        std::vector<u64> bias(c->ks_stride, 0);
        column_bias(c->f, c->ksk.data(), ksk_rows, n + 1, P.ks_base_log, bias.data());
        HIP_OK(c, upload(c->ks_bias, bias.data(), bias.size()));
    }
    // limb-wise copy of the keyswitch key for the matrix-core keyswitch (int8 operands, int32 sums: the digits must
    // fit int8 and a column sum of rows * (B/2) * 128 must stay below 2^31)
    c->ks_mfma_ok = ksk_rows % 32 == 0 && P.ks_levels <= 16 && P.ks_base_log <= 7 &&
                    (ksk_rows << (P.ks_base_log - 1)) < ((size_t)1 << 24);
    if (c->ks_mfma_ok) {
        const uint32_t cbs = (n + 1 + 31) / 32;
        const size_t bytes = (size_t)cbs * (ksk_rows / 32) * c->ops->ks_limbs * 1024;
        if (int rc = build_copy(c, c->ks_limbs, bytes, "ksk_to_limbs", [&](signed char *d) {
                return c->ops->ksk_to_limbs(c->ksk_padded.get(), d, (uint32_t)ksk_rows, n, c->ks_stride, c->ops->ks_limbs, c->stream);
            }))
            return rc;
    }
    c->have_keys = true;
    return 0;
}

// unrolled bootstrap key (host copy in c->bsk3_std) -> device, in the layout of the context's unrolled kernel (rotplan::unrolled_copies)
int upload_bsk3(bmi_ctx *c) {
    HIP_OK(c, hipSetDevice(c->device));
    if (int rc = round_bsk3(c)) return rc;
    c->drop_copies(true);
    if (int rc = build_copies(c, rotplan::unrolled_copies(shape_of(c->P), c->bsk_prec), c->bsk3_std)) return rc;
    c->have_bsk3 = true;
    return 0;
}

// evaluation keys for the secret keys held in c->sk_small / c->sk_big, deterministic in `seed`
int gen_eval_keys(bmi_ctx *c, uint64_t seed) {
    HIP_OK(c, hipSetDevice(c->device));
    drop_sk_mask(c);
    drop_compression_key(c, true);
    gen_eval_key_words(c, seed);
    if (int rc = upload_eval_keys(c)) return rc;
    return c->unroll == 2 ? upload_bsk3(c) : 0;
}

// ------------------------------------------------------------------------------- the hot path
// K-slices of the matrix-core keyswitch: enough wavefronts (tiles x column blocks x slices) to fill 1024 SIMDs twice
uint32_t ks_mfma_slices(const bmi_ctx *c, uint32_t count) {
    const uint32_t tiles = (count + 31) / 32, cbs = (c->P.n + 1 + 31) / 32;
    const uint32_t ksteps = c->big_n * c->P.ks_levels / 32;
    uint32_t slices = 1;
    while (slices < 64 && slices * 2 <= ksteps && ksteps % (slices * 2) == 0 && (size_t)tiles * cbs * slices < 2048) slices *= 2;
    return slices;
}

int ensure_ks_mfma(bmi_ctx *c, uint32_t count) {
    const uint32_t cbs = (c->P.n + 1 + 31) / 32;
    const size_t sums = (size_t)ks_mfma_slices(c, count) * count * c->ops->ks_limbs * cbs * 32 * sizeof(int);
    const int rc = grow(c, c->ks_digits, (size_t)count * c->big_n * c->P.ks_levels, (size_t)8 << 20);
    return rc ? rc : grow(c, c->ks_sums, sums, (size_t)32 << 20);
}

// The kernel of bmi_blind_rotate_batch for a batch of `count` on this context (rotplan::choose_rotation): 0 and *rot, or a refusal.
int choose_rotation(const bmi_ctx *c, uint32_t count, Rot *rot) {
    const rotplan::Choice ch = rotplan::choose_rotation(shape_of(c->P), settings_of(c), held_of(c), count);
    if (!ch.refusal.empty()) return fail(c, -1, ch.refusal);
    *rot = ch.rot;
    return 0;
}

// The launcher of each kernel, in the order of rotplan::Rot
int (*const LAUNCHERS[])(const RotBatch &) = {
    bmit::launch_blind_rotate_wide_u, bmit::launch_blind_rotate_wide_u2, bmit::launch_blind_rotate_wide2, bmit::launch_blind_rotate_wide,
    bmit::launch_blind_rotate_quad, bmit::launch_blind_rotate_tp2u_fft, bmit::launch_blind_rotate_lat2u_fft, bmit::launch_blind_rotate_lat2u,
    bmit::launch_blind_rotate_lat_fft, bmit::launch_blind_rotate_lat, bmit::launch_blind_rotate_fft, bmit::launch_blind_rotate,
    bmi49::launch_blind_rotate_wide_u, bmi49::launch_blind_rotate_wide, bmi49::launch_blind_rotate_quad, bmi49::launch_blind_rotate_lat2u,
    bmi49::launch_blind_rotate_lat2, bmi49::launch_blind_rotate_tpx,
    bmi::launch_blind_rotate_lat, bmi::launch_blind_rotate_tp,
};
static_assert(sizeof(LAUNCHERS) / sizeof(LAUNCHERS[0]) == (size_t)Rot::COUNT, "one launcher per kernel");

// Launches `rot` on the key copy and the tables its row names; hipErrorInvalidValue where the context does not hold one of them (the
// plan never answers with such a kernel: tests/c_abi/rotation_plan_table.cpp).  stat: as RotBatch::stat, for the kernels that take it.
// glwe (has_accumulator_form(rot) only): out receives the accumulators [count][2N] instead of the extracted samples [count][N + 1].
int launch_rotation(const bmi_ctx *c, Rot rot, const u64 *cts, const uint32_t *ids, uint32_t count, u64 *out, unsigned long long *stat,
                    bool glwe, hipStream_t st) {
    const rotplan::RotRow &row = rotplan::row(rot);
    if (glwe && !row.accumulator) return (int)hipErrorInvalidValue;
    RotBatch b{cts, ids, {c->luts.get()}, {c->copies[(int)row.key].get()}, {}, out, count, c->P.n, c->bsk_prec, c->P.bs_levels, c->P.bs_base_log,
               row.stat ? stat : nullptr, glwe, st};
    if (!b.key.p) return (int)hipErrorInvalidValue;
    for (int t = 0; t < 3; t++) {
        b.tab[t] = c->table(row.tab[t]);
        if (row.tab[t] != Table::none && !b.tab[t].p) return (int)hipErrorInvalidValue;
    }
    return LAUNCHERS[(int)rot](b);
}

// accumulators of a batch (room for 256 at least)
int ensure_glwe(bmi_ctx *c, size_t count) {
    const size_t w = (size_t)2 * c->big_n * sizeof(u64);
    return grow(c, c->glwe, count * w, 256 * w);
}

// What the device-pointer forms of the shared look-ups document as preconditions, checked on host arrays: the group ranges
// partition [0, total), and every table is either its group's own base (a plain extraction) or a table with a sparse factor and a
// scale not below the unit of the group's base, which is then a polynomial of bmi_lut_register_base.
int check_groups(bmi_ctx *c, const uint32_t *group_ptr, const uint32_t *base_ids, const uint32_t *lut_ids, uint32_t groups, uint32_t total) {
    if (group_ptr[0] != 0 || group_ptr[groups] != total) return fail(c, -1, "group_ptr must run from 0 to the number of look-ups");
    for (uint32_t g = 0; g < groups; g++) {
        if (group_ptr[g + 1] < group_ptr[g]) return fail(c, -1, "group_ptr must not decrease");
        const uint32_t b = base_ids[g];
        if (b >= c->n_luts) return fail(c, -1, "look-up id " + std::to_string(b) + " is not registered");
        const uint32_t unit = c->sparse_head_host[b].y;
        const bool is_base = unit < 64 && c->base_id_of_unit[unit] == b + 1;
        for (uint32_t t = group_ptr[g]; t < group_ptr[g + 1]; t++) {
            const uint32_t id = lut_ids[t];
            if (id >= c->n_luts) return fail(c, -1, "look-up id " + std::to_string(id) + " is not registered");
            if (id == b) continue;   // the table is the group's own base: a plain extraction
            if (!is_base)
                return fail(c, -1, "id " + std::to_string(b) + " serves another table but is not a base polynomial (bmi_lut_register_base)");
            const uint2 h = c->sparse_head_host[id];
            if (h.x == bmi_ctx::NO_SPARSE) return fail(c, -1, "table " + std::to_string(id) + " has more than 64 boxes: it cannot share a rotation");
            if (h.x == bmi_ctx::WIDE_DIFFERENCE)
                return fail(c, -1, "table " + std::to_string(id) + " has neighbouring entries that differ by more than 2^31 - 1: it cannot share a rotation");
            if (h.y < unit) return fail(c, -1, "table " + std::to_string(id) + " is encoded below its group's unit (2^" + std::to_string(unit) + ")");
        }
    }
    return 0;
}

// a look-up id beyond the registered tables would make the kernels read past the table buffer: refused on the host
// (the device-pointer entry points cannot look at their ids without a synchronisation; their contract is ids < count)
int check_lut_ids(bmi_ctx *c, const uint32_t *lut_ids, uint32_t count) {
    for (uint32_t i = 0; i < count; i++)
        if (lut_ids[i] >= c->n_luts) return fail(c, -1, "look-up id " + std::to_string(lut_ids[i]) + " is not registered");
    return 0;
}

}  // namespace

extern "C" {

int bmi_default_params_for(uint32_t q_bits, bmi_params *out) { return default_params_for(q_bits, out); }

int bmi_default_params(bmi_params *out) { return default_params(out); }

int bmi_preset_params(const char *name, bmi_params *out) { return preset_params(name, out); }

const char *bmi_last_error(const bmi_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int bmi_ctx_create(const bmi_params *params, int device, bmi_ctx **out) {
    if (!params || !out) return fail(nullptr, -1, "null argument");
    std::string why;
    if (!params_supported(*params, why)) return fail(nullptr, -1, why);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(nullptr, -3, "no HIP device: the PBS path has no CPU fallback (hipGetDeviceCount: " +
                                     std::string(hipGetErrorString(e)) + ")");
    if (device < 0 || device >= ndev) return fail(nullptr, -1, "bad device index");
    bmi_ctx *c = new bmi_ctx();
    c->init(*params);
    c->lat_threshold = rotplan::initial_settings(shape_of(c->P)).lat_threshold;
    c->ops = c->f64() ? &bmi49::OPS : c->t64() ? &bmit::OPS : &bmi::OPS;
    c->device = device;
    c->ks_stride = (params->n + 1 + 7) & ~7u;
    auto bail = [&](const std::string &m) {   // releases whatever the context holds so far
        bmi_ctx_destroy(c);
        return fail(nullptr, -2, m);
    };
    if (hipSetDevice(device) != hipSuccess) return bail("hipSetDevice failed");
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) return bail("hipStreamCreate failed");
    hipError_t up = hipSuccess;   // the first failure of the table uploads below
    const uint32_t tabs = rotplan::context_tables(shape_of(c->P));   // the tables this modulus and N have kernels for
    auto want = [&](Table t) { return (tabs & rotplan::bit(t)) != 0; };
    auto put = [&](Table t, const auto &host) {
        const size_t bytes = host.size() * sizeof(host[0]);
        if (up == hipSuccess) up = c->tables[(int)t].alloc(bytes);
        if (up == hipSuccess) up = hipMemcpy(c->tables[(int)t].get(), host.data(), bytes, hipMemcpyHostToDevice);
    };
    const Fq f49q{f49::Q, 49};   // the torus kernels transform mod the 49-bit prime as well
    if (want(Table::tw_wave)) put(Table::tw_wave, to_centred_doubles(build_twiddles(f49q, nttf::PSI_U, nttf::PSI_INV_U, nttf::N_INV_U)));
    if (want(Table::tw_half)) put(Table::tw_half, to_centred_doubles(build_twiddles_half(f49q, nttf::PSI_U, nttf::PSI_INV_U)));
    if (want(Table::tw_gl)) put(Table::tw_gl, build_twiddles(c->f, nttw::PSI, nttw::PSI_INV, nttw::N_INV));
    auto zeta_pow = [](uint32_t e, double *dst) {   // zeta = exp(i pi / 1024)
        const long double ang = 3.14159265358979323846264338327950288L * (long double)(e % 2048) / 1024.0L;
        dst[0] = (double)cosl(ang);
        dst[1] = (double)sinl(ang);
    };
    if (want(Table::tw_fft)) {   // tables of the folded 512-point complex transform (fft_wave_f64.hpp): powers of zeta
        std::vector<double> tf(fftw::TW_WORDS);
        for (uint32_t k2 = 0; k2 < 8; k2++)
            for (uint32_t lane = 0; lane < 64; lane++) zeta_pow(lane * (4 * k2 + 1), &tf[fftw::TW_T1 + (k2 * 64 + lane) * 2]);
        for (uint32_t d = 0; d < 8; d++)
            for (uint32_t a = 0; a < 8; a++) zeta_pow(32 * a * d, &tf[fftw::TW_T2 + (d * 8 + a) * 2]);
        put(Table::tw_fft, tf);
    }
    if (want(Table::tw_fft_half)) {
        std::vector<double> th(ffth::HT_WORDS);
        ffth::build_tables(th.data());
        put(Table::tw_fft_half, th);
    }
    if (want(Table::zeta_pow)) {
        std::vector<double> zp(2048);
        for (uint32_t x = 0; x < 1024; x++) zeta_pow(x, &zp[2 * x]);
        put(Table::zeta_pow, zp);
    }
    if (want(Table::root_pow)) {   // psi^x for the unrolled blind rotation (X^c at the root psi^e is psi^(e c))
        // N = 1024: psi = psi_2048, x in [0, 2048).  N = 2048: psi = psi_4096, x in [0, 2048) (the upper half is the negative)
        std::vector<u64> rp(2048);
        const u64 psi = c->wide() ? f49q.pow(f49::GEN, (f49q.q - 1) / 4096) : (u64)nttf::PSI_U;
        rp[0] = 1;
        for (uint32_t x = 1; x < 2048; x++) rp[x] = f49q.mul(rp[x - 1], psi);
        put(Table::root_pow, to_centred_doubles(rp));
    }
    // tables of the quarter / eighth transforms: powers of zeta = exp(i pi / N)
    static_assert(ffte::ET_WORDS == fftq::QT_WORDS, "the two table sets share a size");
    std::vector<double> tq(fftq::QT_WORDS);
    if (want(Table::tw_quarter)) {
        fftq::build_tables(tq.data());
        put(Table::tw_quarter, tq);
    }
    if (want(Table::tw_eighth)) {
        ffte::build_tables(tq.data());
        put(Table::tw_eighth, tq);
    }
    if (want(Table::zeta_oct)) {   // one octant of the powers of zeta = exp(i pi / 2048): the unrolled kernel folds the rest onto it
        std::vector<double> zo(2 * 513);
        for (uint32_t x = 0; x <= 512; x++) {
            const long double ang = 3.14159265358979323846264338327950288L * (long double)x / 2048.0L;
            zo[2 * x] = (double)cosl(ang);
            zo[2 * x + 1] = (double)sinl(ang);
        }
        put(Table::zeta_oct, zo);
    }
    if (want(Table::tw_wide49)) put(Table::tw_wide49, to_centred_doubles(build_twiddles_wide(c->f)));
    if (want(Table::tw_quad49)) put(Table::tw_quad49, to_centred_doubles(build_twiddles_quad(c->f)));
    c->lut_cap = BMI_LUT_CAP;
    if (up == hipSuccess) up = c->luts.alloc((size_t)c->lut_cap * c->N * 8);
    if (c->t64()) {   // the tables' sparse factors (shared rotations): no entries until a table is registered
        if (up == hipSuccess) up = c->sparse_head.alloc((size_t)BMI_LUT_CAP * sizeof(uint2));
        if (up == hipSuccess) up = c->sparse.alloc((size_t)BMI_LUT_CAP * bmit::BMI_SPARSE_CAP * sizeof(int2));
        if (up == hipSuccess) up = hipMemset(c->sparse_head.get(), 0, c->sparse_head.bytes());
        if (up == hipSuccess) up = hipMemset(c->sparse.get(), 0, c->sparse.bytes());
    }
    if (up != hipSuccess) return bail(std::string("uploading the context's tables: ") + hipGetErrorString(up));
    *out = c;
    return 0;
}

void bmi_ctx_destroy(bmi_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    drop_sk_mask(c);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;   // the device buffers free themselves
}

int bmi_get_params(const bmi_ctx *c, bmi_params *out) {
    if (!c || !out) return -1;
    *out = c->P;
    return 0;
}

int bmi_keygen(bmi_ctx *c) {
    if (!c) return -1;
    if (int rc = rekey_csprng(c)) return rc;
    gen_secret_keys(c, 0);
    return gen_eval_keys(c, 0);
}

int bmi_keygen_insecure_deterministic(bmi_ctx *c, uint64_t seed) {
    if (!c) return -1;
    c->secure_rng = false;
    gen_secret_keys(c, seed);
    return gen_eval_keys(c, seed);
}

int bmi_keygen_from_secret(bmi_ctx *c, const uint64_t *sk_small, const uint64_t *sk_big, uint64_t seed) {
    if (!c || !sk_small || !sk_big) return -1;
    if (int rc = take_secret_keys(c, sk_small, sk_big, seed)) return rc;
    return gen_eval_keys(c, seed);
}

// ct words on the 2^64 torus <-> words mod q: the modulus switch round(x * q / 2^64) and back.  Context-free (host).
int bmi_torus64_to_field(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    return torus64_to_field_words(q_bits, in, words, out);
}

int bmi_field_to_torus64(uint32_t q_bits, const uint64_t *in, uint64_t words, uint64_t *out) {
    return field_to_torus64_words(q_bits, in, words, out);
}

int bmi_import_keys(bmi_ctx *c, const uint64_t *sk_small, const uint64_t *sk_big, const uint64_t *bsk, const uint64_t *ksk) {
    if (!c || !bsk || !ksk) return -1;
    if (int rc = import_keys_pairing(c, sk_small, sk_big)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    if (int rc = import_keys_canonical(c, bsk, ksk)) return rc;
    c->have_keys = false;
    drop_sk_mask(c);
    drop_compression_key(c, true);
    if (int rc = import_keys_store(c, sk_small, sk_big, bsk, ksk)) return rc;
    return upload_eval_keys(c);
}

int bmi_export_keys(const bmi_ctx *c, uint64_t *sk_small, uint64_t *sk_big, uint64_t *bsk, uint64_t *ksk) {
    return hc::export_keys(c, sk_small, sk_big, bsk, ksk);
}

int bmi_key_bytes(const bmi_ctx *c, uint64_t *bsk_bytes, uint64_t *ksk_bytes) {
    if (!c) return -1;
    // every resident device copy (one per kernel family that is selectable on this context), plus the unrolled key
    if (bsk_bytes) {
        *bsk_bytes = 0;
        for (int k = 0; k < (int)Copy::COUNT; k++)
            if (!rotplan::row((Copy)k).unrolled || c->have_bsk3) *bsk_bytes += c->copies[k].bytes();
    }
    if (ksk_bytes) *ksk_bytes = (u64)c->big_n * c->P.ks_levels * (c->P.n + 1) * 8;
    return 0;
}

int bmi_encrypt(bmi_ctx *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *ct_out) {
    return hc::encrypt(c, msgs, count, delta_log, ct_out);
}

int bmi_phase(const bmi_ctx *c, const uint64_t *ct_in, uint32_t count, uint64_t *phase) { return hc::phase(c, ct_in, count, phase); }

int bmi_decrypt(const bmi_ctx *c, const uint64_t *ct_in, uint32_t count, uint32_t delta_log, int64_t *msgs) {
    return hc::decrypt(c, ct_in, count, delta_log, msgs);
}

// the tail of a registration: the test polynomial and, on the torus, its sparse factor go to the device under the next free id
static int add_table(bmi_ctx *c, std::vector<u64> tv, uint2 head, const std::vector<int2> &sparse, uint32_t *lut_id) {
    const uint32_t N = c->N, id = c->n_luts;
    HIP_OK(c, hipSetDevice(c->device));
    {
        const std::vector<double> tvd = c->f64() ? to_centred_doubles(tv) : std::vector<double>();
        const void *src = c->f64() ? (const void *)tvd.data() : (const void *)tv.data();
        HIP_OK(c, hipMemcpy(c->luts.get() + (size_t)id * N, src, N * 8, hipMemcpyHostToDevice));
    }
    if (c->t64()) {
        if (!sparse.empty())
            HIP_OK(c, hipMemcpy(c->sparse.get() + (size_t)id * bmit::BMI_SPARSE_CAP, sparse.data(), sparse.size() * sizeof(int2), hipMemcpyHostToDevice));
        HIP_OK(c, hipMemcpy(c->sparse_head.get() + id, &head, sizeof(head), hipMemcpyHostToDevice));
        c->sparse_head_host.push_back(head);
    }
    c->luts_host.push_back(std::move(tv));
    *lut_id = c->n_luts++;
    return 0;
}

// Shared rotations exist on the 2^64 torus through the floating-point-transform kernels: refused elsewhere
static int shared_rotation_ok(const bmi_ctx *c) {
    if (!c->t64()) return fail(c, -1, "shared rotations exist on the 2^64 torus only (not on the 49-bit field or Goldilocks)");
    return 0;
}

int bmi_lut_register(bmi_ctx *c, const int64_t *table, uint32_t msg_bits, uint32_t out_delta_log, uint32_t *lut_id) {
    if (!c || !table || !lut_id) return -1;
    const uint32_t N = c->N;
    if (msg_bits == 0 || (1u << msg_bits) * 2 > N) return fail(c, -1, "msg_bits out of range for N");
    if (out_delta_log >= c->f.bits - 1) return fail(c, -1, "out_delta_log out of range");
    if (c->t64() && c->bsk_prec != 64 && out_delta_log < (uint32_t)(64 - c->bsk_prec))
        // the torus kernels on a rounded key (48 / 46 / 42 / 40 bits) keep the accumulator as a multiple of 2^16 / 2^18 / 2^22 / 2^24: a table
        // encoded below that scale would lose its low bits - and sits ~2^40 below the noise anyway.  (The exact key has no such grid.)
        return fail(c, -1, "out_delta_log below 64 - (bootstrap-key precision) on the 2^64 torus: test polynomials must be multiples of the key's grid");
    if (c->n_luts == c->lut_cap) return fail(c, -1, "LUT table full");
    // Signed messages on the whole negacyclic circle: box width w = N / 2^p, boxes centred on m*w.
    const uint32_t M = 1u << msg_bits, Mh = M >> 1, w = N >> msg_bits, half = w >> 1;
    std::vector<u64> tv(N);
    for (uint32_t j = 0; j < N; j++) {
        const uint32_t box = (j + half) / w;  // 0 .. M
        i64 f;
        bool negate;
        if (box < Mh) { f = table[box + Mh]; negate = false; }        // m = box >= 0
        else if (box < M) { f = table[box - Mh]; negate = true; }      // m = box - M < 0, reached as -X^(j-N)
        else { f = table[Mh]; negate = true; }                         // m = 0 from below
        const u64 v = c->f.mul(c->f.from_i64(f), (u64)1 << out_delta_log);
        tv[j] = negate ? c->f.neg(v) : v;
    }
    // 2^64 torus: the sparse factor P_f = (1 - X) TV_f / 2^out_delta_log (glwe_lookup.hip) - the differences of consecutive boxes
    // s_0 .. s_M = f(0 .. M/2-1), -f(-M/2 .. -1), -f(0), at the box boundaries b w - w/2.  Taken from the table's INTEGERS: a
    // difference of 2^p at full scale (f(M/2-1) = -M/2 next to -f(-M/2) = +M/2) has no sign once it is a torus word.
    uint2 head{bmi_ctx::NO_SPARSE, out_delta_log};
    std::vector<int2> sparse;
    if (c->t64() && M <= bmit::BMI_SPARSE_CAP) {
        auto box_value = [&](uint32_t b) -> i64 { return b < Mh ? table[b + Mh] : b < M ? -table[b - Mh] : -table[Mh]; };
        bool fits = true;
        for (uint32_t b = 1; b <= M; b++) {
            const i64 d = box_value(b) - box_value(b - 1);
            if (d > INT32_MAX || d < INT32_MIN) fits = false;
            else if (d) sparse.push_back(int2{(int)(b * w - half), (int)d});
        }
        head.x = fits ? (uint32_t)sparse.size() : bmi_ctx::WIDE_DIFFERENCE;
    }
    return add_table(c, std::move(tv), head, sparse, lut_id);
}

int bmi_lut_register_base(bmi_ctx *c, uint32_t unit_log, uint32_t *lut_id) {
    if (!c || !lut_id) return -1;
    if (int rc = shared_rotation_ok(c)) return rc;
    if (unit_log == 0 || unit_log >= 63) return fail(c, -1, "unit_log out of range");
    if (c->bsk_prec != 64 && unit_log < (uint32_t)(64 - c->bsk_prec) + 1)   // (the polynomial's words are 2^(unit_log - 1))
        return fail(c, -1, "unit_log - 1 below 64 - (bootstrap-key precision) on the 2^64 torus: test polynomials must be multiples of the key's grid");
    if (c->base_id_of_unit[unit_log]) {
        *lut_id = c->base_id_of_unit[unit_log] - 1;
        return 0;
    }
    if (c->n_luts == c->lut_cap) return fail(c, -1, "LUT table full");
    // TV_0 = + 2^(unit_log - 1) sum_x X^x: (1 - X) TV_0 = 2^unit_log, so its own sparse factor is the constant 1
    std::vector<u64> tv(c->N, (u64)1 << (unit_log - 1));
    const int rc = add_table(c, std::move(tv), uint2{1, unit_log}, std::vector<int2>{int2{0, 1}}, lut_id);
    if (!rc) c->base_id_of_unit[unit_log] = *lut_id + 1;
    return rc;
}

int bmi_lut_get(const bmi_ctx *c, uint32_t lut_id, uint64_t *test_vector) {
    if (!c || !test_vector) return -1;
    if (lut_id >= c->n_luts) return fail(c, -1, "unknown LUT id");
    std::memcpy(test_vector, c->luts_host[lut_id].data(), c->N * 8);
    return 0;
}

int bmi_set_bsk_precision(bmi_ctx *c, uint32_t bits) {
    if (!c) return -1;
    return hc::set_bsk_precision(c, settings_of(c), held_of(c), bits);
}

int bmi_get_bsk_precision(const bmi_ctx *c, uint32_t *bits) { return hc::get_bsk_precision(c, bits); }

int bmi_set_bsk_unroll(bmi_ctx *c, uint32_t factor) {
    if (!c) return -1;
    bool generated = false;
    if (int rc = hc::set_bsk_unroll(c, settings_of(c), held_of(c), factor, &generated)) return rc;
    return generated ? upload_bsk3(c) : 0;
}

int bmi_import_bsk_unrolled(bmi_ctx *c, const uint64_t *bsk3) {
    if (!c || !bsk3) return -1;
    if (int rc = import_bsk_unrolled_store(c, settings_of(c), held_of(c), bsk3)) return rc;
    return upload_bsk3(c);
}

int bmi_export_bsk_unrolled(const bmi_ctx *c, uint64_t *bsk3) { return hc::export_bsk_unrolled(c, bsk3); }

int bmi_set_keyswitch_variant(bmi_ctx *c, int variant) {
    if (!c) return -1;
    if (variant < 0 || variant > 1) return fail(c, -1, "keyswitch variant must be 0 or 1");
    c->ks_variant = variant;
    return 0;
}

int bmi_set_modswitch(bmi_ctx *c, uint32_t mode) {
    if (!c) return -1;
    if (mode > 1) return fail(c, -1, "modulus-switch mode must be 0 (standard) or 1 (centred)");
    if (mode == 1 && !c->t64() && !c->f64())
        return fail(c, -1, "the centred modulus switch exists on the 2^64 torus and the 49-bit field only (Goldilocks is a cross-check engine)");
    c->modswitch = mode;
    return 0;
}

int bmi_get_modswitch(const bmi_ctx *c, uint32_t *mode) {
    if (!c) return -1;
    if (!mode) return fail(c, -1, "bmi_get_modswitch: null result pointer");
    *mode = c->modswitch;
    return 0;
}

int bmi_rotation_kernel(const bmi_ctx *c, uint32_t count, const char **name) {
    if (!c || !name) return -1;
    Rot rot;
    if (int rc = choose_rotation(c, count, &rot)) return rc;
    *name = rotplan::rotation_name(rot);
    return 0;
}

int bmi_set_kernel_variant(bmi_ctx *c, int variant) {
    if (!c) return -1;
    const std::string refusal = rotplan::set_variant_refusal(shape_of(c->P), variant);
    if (!refusal.empty()) return fail(c, -1, refusal);
    c->variant = variant;
    return 0;
}

// ------------------------------------------------------------------------------- the hot path
int bmi_keyswitch_batch(bmi_ctx *c, const uint64_t *d_in, uint32_t count, uint64_t *d_small, void *stream) {
    if (!c || (count && (!d_in || !d_small))) return -1;
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    if (count == 0) return 0;
    HIP_OK(c, hipSetDevice(c->device));
    if (c->ks_variant == 0 && c->ks_mfma_ok && count >= BMI_KS_MFMA_MIN) {
        if (int rc = ensure_ks_mfma(c, count)) return rc;
        const int rc = c->ops->keyswitch_mfma(d_in, c->ks_limbs.get(), c->ks_digits.get(), c->ks_sums.get(), d_small, ks_mfma_slices(c, count),
                                              count, c->P.n, c->big_n, c->P.ks_levels, c->P.ks_base_log, (hipStream_t)stream);
        return launched(c, "keyswitch (matrix cores) launch: ", rc);
    }
    if (c->P.n + 1 > 3 * 256)   // ks_lincomb.hpp: KS_COLS x KS_THREADS output columns per workgroup
        return fail(c, -1, c->ks_mfma_ok ? "the scalar keyswitch kernel takes n <= 767; this parameter set needs the matrix-core form"
                                         : "no keyswitch kernel takes this parameter set: the scalar kernel takes n <= 767, and the matrix-core "
                                           "form takes at most 16 levels with int32 column sums (k N levels 2^(base_log + 6) < 2^31)");
    // Scalar form.  The row walk (k*N*levels rows) of one workgroup is the latency of a small batch, so it is split over
    // `slices` workgroups per tile of 8 ciphertexts (partial 128-bit sums + a reduce kernel) until the launch
    // has ~1024 workgroups; large batches fill the chip with one slice.
    const uint32_t tiles = (count + 7) / 8;
    uint32_t slices = 1;
    if (c->variant == 0 || c->variant == 2)
        while (slices < 64 && tiles * slices * 2 <= 1024) slices *= 2;
    // A workgroup stages the digits of its slice in dynamic LDS (ks_scalar_lds_bytes): whatever the batch size and the
    // pinned rotation variant, the coefficients are split until that fits the kernel's limit (64 KiB: 1024 x 8 levels unsplit).
    while (slices < 64 && ks_scalar_lds_bytes(c->big_n, c->P.ks_levels, slices) > BMI_KS_LDS_MAX) slices *= 2;
    if (ks_scalar_lds_bytes(c->big_n, c->P.ks_levels, slices) > BMI_KS_LDS_MAX)
        return fail(c, -1, "the scalar keyswitch kernel cannot stage this parameter set's digits: 8 x ceil(k N / 64) x levels bytes exceed "
                           "its 64 KiB of LDS");
    if (slices > 1)
        if (int rc = grow(c, c->ks_partial, (size_t)slices * count * c->ks_stride * 16, KS_PARTIAL_BYTES)) return rc;
    int rc = c->ops->keyswitch(d_in, c->ksk_padded.get(), c->ks_bias.get(), d_small, slices > 1 ? c->ks_partial.get() : nullptr, slices,
                               count, c->P.n, c->big_n, c->P.ks_levels, c->P.ks_base_log, c->ks_stride, (hipStream_t)stream);
    return launched(c, "keyswitch launch: ", rc);
}

// bmi_blind_rotate_batch (d_out = [count][N + 1] samples) and, with glwe, bmi_blind_rotate_glwe_batch (d_out = [count][2N] accumulators)
static int blind_rotate_batch(bmi_ctx *c, const uint64_t *d_small, const uint32_t *d_lut_ids, uint32_t count, uint64_t *d_out, bool glwe,
                              void *stream) {
    if (!c || (count && (!d_small || !d_lut_ids || !d_out))) return -1;
    if (glwe)
        if (int rc = shared_rotation_ok(c)) return rc;
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    HIP_OK(c, hipSetDevice(c->device));
    Rot rot;
    if (int rc = choose_rotation(c, count, &rot)) return rc;
    if (glwe && !rotplan::has_accumulator_form(rot))
        return fail(c, -1, "the accumulator form exists for the floating-point-transform kernels only: not for a pinned exact-transform variant "
                           "(1 / 3 / 4), nor for the unrolled key pinned at 48 bits of precision (the exact-transform unrolled kernel)");
    if (int rc = build_copies(c, rotplan::on_demand_copies(rot), c->bsk_std)) return rc;   // (a no-op once built)
    return launched(c, glwe ? "blind_rotate (accumulator form) launch: " : "blind_rotate launch: ",
                    launch_rotation(c, rot, d_small, d_lut_ids, count, d_out, nullptr, glwe, (hipStream_t)stream));
}

int bmi_blind_rotate_batch(bmi_ctx *c, const uint64_t *d_small, const uint32_t *d_lut_ids, uint32_t count,
                           uint64_t *d_out, void *stream) {
    return blind_rotate_batch(c, d_small, d_lut_ids, count, d_out, false, stream);
}

// The centred modulus switch of `count` small ciphertexts (modswitch_centre.hip): their bodies minus half the sum of the mask words'
// rounding errors.  Needs no keys; whatever the context's mode.
int bmi_modswitch_centre_batch(bmi_ctx *c, const uint64_t *d_small_in, uint32_t count, uint64_t *d_small_out, void *stream) {
    if (!c) return -1;
    if (count && (!d_small_in || !d_small_out)) return fail(c, -1, "bmi_modswitch_centre_batch: null ciphertext pointer");
    if (!c->t64() && !c->f64())
        return fail(c, -1, "the centred modulus switch exists on the 2^64 torus and the 49-bit field only (Goldilocks is a cross-check engine)");
    if (count == 0) return 0;
    HIP_OK(c, hipSetDevice(c->device));
    const int rc = bmi::launch_modswitch_centre(d_small_in, d_small_out, count, c->P.n, c->P.log_N, c->t64(), (hipStream_t)stream);
    return launched(c, "modswitch_centre launch: ", rc);
}

int bmi_pbs_batch(bmi_ctx *c, const uint64_t *d_in, const uint32_t *d_lut_ids, uint32_t count, uint64_t *d_out,
                  void *stream) {
    if (!c) return -1;
    HIP_OK(c, hipSetDevice(c->device));
    int rc = ensure_small(c, count);
    if (rc) return rc;
    rc = bmi_keyswitch_batch(c, d_in, count, c->small.get(), stream);
    if (!rc && c->modswitch == 1) rc = bmi_modswitch_centre_batch(c, c->small.get(), count, c->small.get(), stream);
    if (rc) return rc;
    return bmi_blind_rotate_batch(c, c->small.get(), d_lut_ids, count, d_out, stream);
}

int bmi_blind_rotate_glwe_batch(bmi_ctx *c, const uint64_t *d_small, const uint32_t *d_lut_ids, uint32_t count, uint64_t *d_glwe,
                                void *stream) {
    return blind_rotate_batch(c, d_small, d_lut_ids, count, d_glwe, true, stream);
}

int bmi_glwe_lookup_batch(bmi_ctx *c, const uint64_t *d_glwe, const uint32_t *d_group_ptr, const uint32_t *d_base_ids,
                          const uint32_t *d_lut_ids, uint32_t groups, uint32_t total, uint64_t *d_out, void *stream) {
    if (!c || (groups && (!d_glwe || !d_group_ptr || !d_base_ids)) || (total && (!d_lut_ids || !d_out))) return -1;
    if (int rc = shared_rotation_ok(c)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    const int rc = bmit::launch_glwe_lookup(d_glwe, d_group_ptr, d_base_ids, d_lut_ids, c->sparse_head.get(), c->sparse.get(), d_out, groups,
                                            total, c->N, (hipStream_t)stream);
    return launched(c, "glwe_lookup launch: ", rc);
}

int bmi_pbs_shared_batch(bmi_ctx *c, const uint64_t *d_in, const uint32_t *d_group_ptr, const uint32_t *d_base_ids,
                         const uint32_t *d_lut_ids, uint32_t groups, uint32_t total, uint64_t *d_out, void *stream) {
    if (!c) return -1;
    if (int rc = shared_rotation_ok(c)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    int rc = ensure_small(c, groups);
    if (!rc) rc = ensure_glwe(c, groups);
    if (!rc) rc = bmi_keyswitch_batch(c, d_in, groups, c->small.get(), stream);
    if (!rc && c->modswitch == 1) rc = bmi_modswitch_centre_batch(c, c->small.get(), groups, c->small.get(), stream);
    if (!rc) rc = bmi_blind_rotate_glwe_batch(c, c->small.get(), d_base_ids, groups, c->glwe.get(), stream);
    return rc ? rc : bmi_glwe_lookup_batch(c, c->glwe.get(), d_group_ptr, d_base_ids, d_lut_ids, groups, total, d_out, stream);
}

int bmi_lincomb_batch(bmi_ctx *c, const uint64_t *d_store, const uint32_t *d_row_ptr, const uint32_t *d_idx,
                      const int64_t *d_coef, const uint64_t *d_const_body, uint32_t count, uint64_t *d_out,
                      void *stream) {
    if (!c || (count && (!d_store || !d_row_ptr || !d_const_body || !d_out))) return -1;
    HIP_OK(c, hipSetDevice(c->device));
    int rc = c->ops->lincomb(d_store, d_row_ptr, d_idx, (const i64 *)d_coef, d_const_body, d_out, count, c->big_n + 1, (hipStream_t)stream);
    return launched(c, "lincomb launch: ", rc);
}

// phase (d_msgs null) or decryption of device-resident ciphertexts: the checks of bmi_phase, then one launch of k_lwe_phase
static int phase_decrypt_batch(bmi_ctx *c, const uint64_t *d_ct, uint32_t count, uint32_t delta_log, const int64_t *d_expected,
                               uint64_t *d_phase, int64_t *d_msgs, int64_t *d_err, void *stream) {
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    if (!c->have_secret) return fail(c, -1, "evaluation-only context: it holds no secret key");
    if (count == 0) return 0;
    HIP_OK(c, hipSetDevice(c->device));
    if (int rc = ensure_sk_mask(c)) return rc;
    const int rc = c->ops->lwe_phase(d_ct, c->sk_mask.get(), d_phase, (const i64 *)d_expected, (i64 *)d_msgs, (i64 *)d_err, count, c->big_n,
                                     delta_log, (hipStream_t)stream);
    return launched(c, "lwe_phase launch: ", rc);
}

int bmi_phase_batch(bmi_ctx *c, const uint64_t *d_ct, uint32_t count, uint64_t *d_phase, void *stream) {
    if (!c || (count && (!d_ct || !d_phase))) return -1;
    return phase_decrypt_batch(c, d_ct, count, 0, nullptr, d_phase, nullptr, nullptr, stream);
}

int bmi_decrypt_batch(bmi_ctx *c, const uint64_t *d_ct, uint32_t count, uint32_t delta_log, const int64_t *d_expected,
                      int64_t *d_msgs, int64_t *d_err, void *stream) {
    if (!c || (count && (!d_ct || !d_msgs))) return -1;
    if (delta_log == 0 || delta_log >= c->f.bits - 1) return fail(c, -1, "delta_log out of range");
    return phase_decrypt_batch(c, d_ct, count, delta_log, d_expected, nullptr, d_msgs, d_err, stream);
}

int bmi_scatter_rows(bmi_ctx *c, const uint64_t *d_src, uint32_t count, uint64_t *d_store, const uint32_t *d_rows,
                     void *stream) {
    if (!c || (count && (!d_src || !d_store || !d_rows))) return -1;
    HIP_OK(c, hipSetDevice(c->device));
    int rc = bmi::launch_scatter_rows(d_src, d_store, d_rows, count, c->big_n + 1, (hipStream_t)stream);
    return launched(c, "scatter_rows launch: ", rc);
}

int bmi_reserve(bmi_ctx *c, uint32_t max_count) {
    if (!c) return -1;
    HIP_OK(c, hipSetDevice(c->device));
    HIP_OK(c, hipDeviceSynchronize());
    if (int rc = grow(c, c->ks_partial, KS_PARTIAL_BYTES, KS_PARTIAL_BYTES)) return rc;
    if (c->ks_mfma_ok) {
        // the sums buffer peaks where the K-split is still active (small batches), not at max_count, and the slice
        // count is not monotonic in the batch size: take the largest need over every tile count up to max_count
        uint32_t worst = max_count;
        size_t worst_sums = 0;
        for (uint32_t tiles = 1; tiles <= (max_count + 31) / 32; tiles++) {
            const uint32_t cnt = std::min(tiles * 32, max_count);
            const size_t sums = (size_t)ks_mfma_slices(c, cnt) * cnt;
            if (sums > worst_sums) { worst_sums = sums; worst = cnt; }
        }
        int rc = ensure_ks_mfma(c, worst);
        if (rc) return rc;
        rc = ensure_ks_mfma(c, max_count);
        if (rc) return rc;
    }
    if (c->t64())
        if (int rc = ensure_glwe(c, max_count)) return rc;
    return ensure_small(c, max_count);
}

int bmi_sync(bmi_ctx *c, void *stream) {
    if (!c) return -1;
    HIP_OK(c, hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------- host-buffer convenience forms
// Each checks what can be checked on the host, names its regions and hands the device-pointer form to Stage::run.
int bmi_pbs_batch_host(bmi_ctx *c, const uint64_t *in, const uint32_t *lut_ids, uint32_t count, uint64_t *out) {
    if (!c || !in || !lut_ids || !out) return -1;
    if (int bad = check_lut_ids(c, lut_ids, count)) return bad;
    const size_t w = (size_t)c->big_n + 1;
    Stage s;
    const auto d_in = s.upload(in, count * w);
    const auto d_ids = s.upload(lut_ids, count);
    const auto d_out = s.download(out, count * w);
    return s.run(c, [&] { return bmi_pbs_batch(c, s[d_in], s[d_ids], count, s[d_out], c->stream); });
}

int bmi_keyswitch_batch_host(bmi_ctx *c, const uint64_t *in, uint32_t count, uint64_t *small_out) {
    if (!c || !in || !small_out) return -1;
    Stage s;
    const auto d_in = s.upload(in, (size_t)count * (c->big_n + 1));
    const auto d_small = s.download(small_out, (size_t)count * (c->P.n + 1));
    return s.run(c, [&] { return bmi_keyswitch_batch(c, s[d_in], count, s[d_small], c->stream); });
}

int bmi_modswitch_centre_batch_host(bmi_ctx *c, const uint64_t *small_in, uint32_t count, uint64_t *small_out) {
    if (!c) return -1;
    if (!small_in || !small_out) return fail(c, -1, "bmi_modswitch_centre_batch_host: null ciphertext pointer");
    Stage s;
    const auto d_small = s.region((size_t)count * (c->P.n + 1), small_in, small_out);   // switched in place
    return s.run(c, [&] { return bmi_modswitch_centre_batch(c, s[d_small], count, s[d_small], c->stream); });
}

// bmi_blind_rotate_batch_host (rows of N + 1 words) and, with glwe, bmi_blind_rotate_glwe_batch_host (rows of 2N words)
static int blind_rotate_batch_host(bmi_ctx *c, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count, uint64_t *out, bool glwe) {
    if (!c || !small_in || !lut_ids || !out) return -1;
    if (glwe)
        if (int rc = shared_rotation_ok(c)) return rc;
    if (int bad = check_lut_ids(c, lut_ids, count)) return bad;
    Stage s;
    const auto d_small = s.upload(small_in, (size_t)count * (c->P.n + 1));
    const auto d_ids = s.upload(lut_ids, count);
    const auto d_out = s.download(out, count * (glwe ? (size_t)2 * c->big_n : (size_t)c->big_n + 1));
    return s.run(c, [&] { return blind_rotate_batch(c, s[d_small], s[d_ids], count, s[d_out], glwe, c->stream); });
}

int bmi_blind_rotate_batch_host(bmi_ctx *c, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count,
                                uint64_t *out) {
    return blind_rotate_batch_host(c, small_in, lut_ids, count, out, false);
}

// Host-buffer forms of the shared look-ups.  They refuse what the device-pointer forms state as preconditions (check_groups).
int bmi_blind_rotate_glwe_batch_host(bmi_ctx *c, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count, uint64_t *glwe_out) {
    return blind_rotate_batch_host(c, small_in, lut_ids, count, glwe_out, true);
}

// the group description of a host-buffer form: group_ptr [groups + 1], base ids [groups], lut_ids [total]
struct GroupRefs {
    Stage::Ref<uint32_t> ptr, base, ids;
};
static GroupRefs stage_groups(Stage &s, const uint32_t *group_ptr, const uint32_t *base_ids, const uint32_t *lut_ids, uint32_t groups, uint32_t total) {
    return {s.upload(group_ptr, (size_t)groups + 1), s.upload(base_ids, groups), s.upload(lut_ids, total)};
}

int bmi_glwe_lookup_batch_host(bmi_ctx *c, const uint64_t *glwe_in, const uint32_t *group_ptr, const uint32_t *base_ids,
                               const uint32_t *lut_ids, uint32_t groups, uint32_t total, uint64_t *out) {
    if (!c || !glwe_in || !group_ptr || !base_ids || !lut_ids || !out) return -1;
    if (int rc = shared_rotation_ok(c)) return rc;
    if (int bad = check_groups(c, group_ptr, base_ids, lut_ids, groups, total)) return bad;
    Stage s;
    const auto d_glwe = s.upload(glwe_in, (size_t)groups * 2 * c->big_n);
    const GroupRefs g = stage_groups(s, group_ptr, base_ids, lut_ids, groups, total);
    const auto d_out = s.download(out, (size_t)total * (c->big_n + 1));
    return s.run(c, [&] { return bmi_glwe_lookup_batch(c, s[d_glwe], s[g.ptr], s[g.base], s[g.ids], groups, total, s[d_out], c->stream); });
}

int bmi_pbs_shared_batch_host(bmi_ctx *c, const uint64_t *in, const uint32_t *group_ptr, const uint32_t *base_ids,
                              const uint32_t *lut_ids, uint32_t groups, uint32_t total, uint64_t *out) {
    if (!c || !in || !group_ptr || !base_ids || !lut_ids || !out) return -1;
    if (int rc = shared_rotation_ok(c)) return rc;
    if (int bad = check_groups(c, group_ptr, base_ids, lut_ids, groups, total)) return bad;
    Stage s;
    const auto d_in = s.upload(in, (size_t)groups * (c->big_n + 1));
    const GroupRefs g = stage_groups(s, group_ptr, base_ids, lut_ids, groups, total);
    const auto d_out = s.download(out, (size_t)total * (c->big_n + 1));
    return s.run(c, [&] { return bmi_pbs_shared_batch(c, s[d_in], s[g.ptr], s[g.base], s[g.ids], groups, total, s[d_out], c->stream); });
}

int bmi_fft_margin_host(bmi_ctx *c, const uint64_t *small_in, const uint32_t *lut_ids, uint32_t count, uint64_t *out,
                        double *max_distance) {
    if (!c || !small_in || !lut_ids || !out || !max_distance) return -1;
    if (!c->have_keys) return fail(c, -1, "no keys: call bmi_keygen first");
    const rotplan::Choice ch = rotplan::margin_rotation(shape_of(c->P), settings_of(c), held_of(c), count);
    if (!ch.refusal.empty()) return fail(c, -1, ch.refusal);
    if (int bad = check_lut_ids(c, lut_ids, count)) return bad;
    unsigned long long bits = 0;   // the statistic word: zero on the device before the kernel, here after it
    Stage s;
    const auto d_small = s.upload(small_in, (size_t)count * (c->P.n + 1));
    const auto d_ids = s.upload(lut_ids, count);
    const auto d_out = s.download(out, (size_t)count * (c->big_n + 1));
    const auto d_stat = s.region<unsigned long long>(1, nullptr, &bits, true);
    const int rc = s.run(c, [&] {
        return launched(c, "bmi_fft_margin_host: ", launch_rotation(c, ch.rot, s[d_small], s[d_ids], count, s[d_out], s[d_stat], false, c->stream));
    });
    if (!rc) std::memcpy(max_distance, &bits, 8);
    return rc;
}

int bmi_negacyclic_mul_host(bmi_ctx *c, const uint64_t *a, const uint64_t *b, uint32_t count, uint64_t *out) {
    if (!c || !a || !b || !out) return -1;
    if (c->wide() || c->quad()) return fail(c, -1, "the transform test hook exists for N = 1024 only");
    if (c->t64()) return fail(c, -1, "no transform exists mod 2^64: the test hook covers the two prime fields");
    const size_t words = (size_t)count * c->N;
    Stage s;
    const auto da = s.upload(a, words), db = s.upload(b, words);
    const auto dc = s.download(out, words);
    const DevWords g_tw = c->table(c->f64() ? Table::tw_wave : Table::tw_gl);   // each field has its own twiddle table
    return s.run(c, [&] {
        return c->ops->negacyclic_mul(s[da], s[db], s[dc], g_tw, count, c->stream) ? fail(c, -2, "negacyclic_mul launch failed") : 0;
    });
}

// ------------------------------------------------------------------- seeded keys and ciphertexts (chacha_expand.hip)
// The specification of the seeded forms (hc::seeded_mask_words).  Context-free, host only.
int bmi_seeded_mask_words(const uint32_t pub_key[8], uint64_t nonce, uint64_t first_word, uint64_t count, uint64_t *out) {
    return seeded_mask_words_checked(pub_key, nonce, first_word, count, out);
}

// One seeded array -> its full standard-domain form in `full` ([rows][mask_w + body_w] host words): the compact bodies are uploaded
// and placed behind the masks (k_place_bodies), the masks are expanded on the device (k_chacha_expand, rows numbered from 0 in
// `domain`), and the host copy is filled from the device buffer.
static int expand_seeded_key(bmi_ctx *c, u64 domain, size_t rows, uint32_t mask_w, uint32_t body_w, const u64 *bodies, std::vector<u64> &full) {
    const size_t pitch = (size_t)mask_w + body_w;
    DevBuf<u64> d_bodies, d_full;
    HIP_OK(c, d_bodies.alloc(rows * body_w * 8));
    HIP_OK(c, d_full.alloc(rows * pitch * 8));
    HIP_OK(c, hipMemcpyAsync(d_bodies.get(), bodies, rows * body_w * 8, hipMemcpyHostToDevice, c->stream));
    int rc = bmi::launch_place_bodies(d_bodies.get(), d_full.get() + mask_w, pitch, body_w, rows, c->stream);
    if (!rc) rc = bmi::launch_chacha_expand(d_full.get(), pitch, mask_w, rows, c->rng_public.k, domain, 0, c->stream);
    if (rc) return launched(c, "chacha_expand launch: ", rc);
    full.resize(rows * pitch);
    HIP_OK(c, hipMemcpyAsync(full.data(), d_full.get(), rows * pitch * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int bmi_export_keys_seeded(const bmi_ctx *c, uint32_t pub_key[8], uint64_t *bsk_bodies, uint64_t *ksk_bodies) {
    return hc::export_keys_seeded(c, pub_key, bsk_bodies, ksk_bodies);
}

int bmi_import_keys_seeded(bmi_ctx *c, const uint32_t pub_key[8], const uint64_t *bsk_bodies, const uint64_t *ksk_bodies) {
    if (!c || !pub_key || !bsk_bodies || !ksk_bodies) return -1;
    if (!c->t64())
        return fail(c, -1, "bmi_import_keys_seeded: seeded forms exist on the 2^64 torus only - on the 49-bit field and Goldilocks the masks "
                           "are rejection-sampled, so a mask word's position in the stream depends on the words before it");
    HIP_OK(c, hipSetDevice(c->device));
    c->have_keys = false;
    drop_sk_mask(c);
    drop_compression_key(c, true);
    c->have_bsk3 = false;
    c->bsk3_from_stream = false;
    c->have_secret = false;   // evaluation-only: the secrets stay with the client
    c->sk_small.clear();
    c->sk_big.clear();
    c->mask_src = bmi_ctx::MaskSource::OTHER;   // until both arrays are expanded
    std::memcpy(c->rng_public.k, pub_key, sizeof(c->rng_public.k));
    c->secure_rng = true;
    if (int rc = expand_seeded_key(c, S_BSK_MASK, (size_t)c->P.n * c->rows, c->big_n, c->N, bsk_bodies, c->bsk_std)) return rc;
    if (int rc = expand_seeded_key(c, S_KSK_MASK, (size_t)c->big_n * c->P.ks_levels, c->P.n, 1, ksk_bodies, c->ksk)) return rc;
    // from here on the path of every key set: rounding to the key's precision, key conversions, keyswitch bias and limb form
    if (int rc = upload_eval_keys(c)) return rc;
    c->mask_src = bmi_ctx::MaskSource::SEEDED_IMPORT;
    return 0;
}

int bmi_export_bsk_unrolled_seeded(const bmi_ctx *c, uint64_t *bsk3_bodies) { return hc::export_bsk_unrolled_seeded(c, bsk3_bodies); }

int bmi_import_bsk_unrolled_seeded(bmi_ctx *c, const uint64_t *bsk3_bodies) {
    if (!c || !bsk3_bodies) return -1;
    if (!c->have_keys || c->mask_src != bmi_ctx::MaskSource::SEEDED_IMPORT)
        return fail(c, -1, "bmi_import_bsk_unrolled_seeded: the unrolled key's masks are expanded from the public key of a preceding "
                           "bmi_import_keys_seeded, and this context has none");
    const std::string refusal = rotplan::import_unrolled_seeded_refusal(shape_of(c->P), settings_of(c));
    if (!refusal.empty()) return fail(c, -1, refusal);
    HIP_OK(c, hipSetDevice(c->device));
    if (int rc = expand_seeded_key(c, S_BSK3_MASK, (size_t)c->pairs() * 3 * c->rows, c->big_n, c->N, bsk3_bodies, c->bsk3_std)) return rc;
    if (int rc = upload_bsk3(c)) return rc;
    c->bsk3_from_stream = true;
    return 0;
}

int bmi_encrypt_seeded(bmi_ctx *c, const int64_t *msgs, uint32_t count, uint32_t delta_log, uint64_t *first_counter, uint64_t *bodies) {
    return hc::encrypt_seeded(c, msgs, count, delta_log, first_counter, bodies);
}

int bmi_expand_seeded_batch(bmi_ctx *c, uint64_t first_counter, const uint64_t *d_bodies, uint32_t count, uint64_t *d_out, void *stream) {
    if (!c || (count && (!d_bodies || !d_out))) return -1;
    if (int rc = seeded_ok(c, "bmi_expand_seeded_batch")) return rc;
    if (count == 0) return 0;
    HIP_OK(c, hipSetDevice(c->device));
    const size_t pitch = (size_t)c->big_n + 1;
    int rc = bmi::launch_place_bodies(d_bodies, d_out + c->big_n, pitch, 1, count, (hipStream_t)stream);
    if (!rc) rc = bmi::launch_chacha_expand(d_out, pitch, c->big_n, count, c->rng_public.k, S_ENC_MASK, first_counter, (hipStream_t)stream);
    return launched(c, "chacha_expand launch: ", rc);
}

int bmi_expand_seeded_batch_host(bmi_ctx *c, uint64_t first_counter, const uint64_t *bodies, uint32_t count, uint64_t *out) {
    if (!c || (count && (!bodies || !out))) return -1;
    if (int rc = seeded_ok(c, "bmi_expand_seeded_batch_host")) return rc;
    if (count == 0) return 0;
    Stage s;
    const auto d_bodies = s.upload(bodies, count);
    const auto d_out = s.download(out, (size_t)count * (c->big_n + 1));
    return s.run(c, [&] { return bmi_expand_seeded_batch(c, first_counter, s[d_bodies], count, s[d_out], c->stream); });
}

// ------------------------------------------------------------------- compression of output ciphertexts (lwe_pack.hip)
// (what every compression entry point needs of a context, and of a (levels, base log) pair: key_set.hpp)
// the compression key (host copy in c->pksk, standard layout) -> device, with the bias vector of the unsigned-digit product:
// bias[col] = 2^(base_log - 1) * sum over all rows of key[row][col]
static int upload_compression_key(bmi_ctx *c, uint32_t levels, uint32_t base_log) {
    std::vector<u64> bias((size_t)2 * c->N);
    column_bias(c->f, c->pksk.data(), (size_t)c->N * levels, bias.size(), base_log, bias.data());
    c->pk_levels = 0;
    HIP_OK(c, upload(c->pksk_dev, c->pksk.data(), c->pksk.size()));
    HIP_OK(c, upload(c->pk_bias, bias.data(), bias.size()));
    c->pk_levels = levels;
    c->pk_base_log = base_log;
    return 0;
}

int bmi_compression_keygen(bmi_ctx *c, uint32_t levels, uint32_t base_log) {
    if (!c) return -1;
    if (int rc = compression_keygen_refusal(c, levels, base_log)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    drop_compression_key(c, false);
    gen_compression_key(c, levels, base_log);
    if (int rc = upload_compression_key(c, levels, base_log)) return rc;
    c->pksk_from_stream = compression_key_from_stream(c);
    return 0;
}

int bmi_compression_key_info(const bmi_ctx *c, uint32_t *levels, uint32_t *base_log, uint64_t *device_bytes) {
    if (!c) return -1;
    if (levels) *levels = c->pk_levels;
    if (base_log) *base_log = c->pk_base_log;
    if (device_bytes) *device_bytes = c->pk_levels ? c->pksk_dev.bytes() + c->pk_bias.bytes() : 0;
    return 0;
}

int bmi_export_compression_key(const bmi_ctx *c, uint64_t *key) { return hc::export_compression_key(c, key); }

int bmi_import_compression_key(bmi_ctx *c, uint32_t levels, uint32_t base_log, const uint64_t *key) {
    if (!c || !key) return -1;
    if (int rc = import_compression_key_refusal(c, levels, base_log)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    drop_compression_key(c, false);
    import_compression_key_store(c, levels, key);
    return upload_compression_key(c, levels, base_log);
}

int bmi_export_compression_key_seeded(const bmi_ctx *c, uint64_t *bodies) { return hc::export_compression_key_seeded(c, bodies); }

int bmi_import_compression_key_seeded(bmi_ctx *c, uint32_t levels, uint32_t base_log, const uint64_t *bodies) {
    if (!c || !bodies) return -1;
    if (int rc = compression_ok(c, "bmi_import_compression_key_seeded")) return rc;
    if (c->mask_src != bmi_ctx::MaskSource::SEEDED_IMPORT)
        return fail(c, -1, "bmi_import_compression_key_seeded: the compression key's masks are expanded from the public key of a preceding "
                           "bmi_import_keys_seeded, and this context has none");
    if (int rc = compression_shape_ok(c, "bmi_import_compression_key_seeded", levels, base_log)) return rc;
    HIP_OK(c, hipSetDevice(c->device));
    drop_compression_key(c, false);
    if (int rc = expand_seeded_key(c, S_PKSK_MASK, (size_t)c->N * levels, c->N, c->N, bodies, c->pksk)) return rc;
    if (int rc = upload_compression_key(c, levels, base_log)) return rc;
    c->pksk_from_stream = true;
    return 0;
}

int bmi_compressed_words(const bmi_ctx *c, uint32_t count, uint64_t *words) { return hc::compressed_words(c, count, words); }

int bmi_compress_batch(bmi_ctx *c, const uint64_t *d_in, uint32_t count, uint32_t log_modulus, uint32_t *d_out, void *stream) {
    if (!c || (count && (!d_in || !d_out))) return -1;
    if (int rc = compression_key_held(c, "bmi_compress_batch")) return rc;
    if (int rc = log_modulus_ok(c, "bmi_compress_batch", log_modulus)) return rc;
    if (count == 0) return 0;
    HIP_OK(c, hipSetDevice(c->device));
    const uint32_t N = c->N, slice = bmit::pack_slice(N), widest = std::min(std::min(count, N), slice);
    // scratch for the widest slice of this call, at least 64 ciphertexts' worth
    int rc = grow(c, c->pk_digits, (size_t)widest * N * c->pk_levels * 4, (size_t)64 * N * c->pk_levels * 4);
    if (!rc) rc = grow(c, c->pk_T, (size_t)widest * 2 * N * 8, (size_t)64 * 2 * N * 8);
    if (!rc) rc = grow(c, c->pk_acc, (size_t)2 * N * 8, (size_t)2 * N * 8);
    if (rc) return rc;
    const hipStream_t st = (hipStream_t)stream;
    for (uint32_t t0 = 0; t0 < count; t0 += N) {   // blocks of N ciphertexts, each in slices
        const uint32_t m = std::min(N, count - t0);
        for (uint32_t s0 = 0; s0 < m; s0 += slice) {
            const int e = bmit::launch_pack_slice(d_in + (size_t)(t0 + s0) * (N + 1), c->pksk_dev.get(), c->pk_bias.get(), c->pk_digits.get(),
                                                  c->pk_T.get(), c->pk_acc.get(), std::min(slice, m - s0), s0, N, c->pk_levels,
                                                  c->pk_base_log, st);
            if (e) return launched(c, "lwe_pack launch: ", e);
        }
        const int e = bmit::launch_pack_switch(c->pk_acc.get(), d_out + (size_t)(t0 / N) * 2 * N, m, N, log_modulus, st);
        if (e) return launched(c, "lwe_pack switch launch: ", e);
    }
    return 0;
}

int bmi_compress_batch_host(bmi_ctx *c, const uint64_t *in, uint32_t count, uint32_t log_modulus, uint32_t *out) {
    if (!c || (count && (!in || !out))) return -1;
    if (int rc = compression_key_held(c, "bmi_compress_batch_host")) return rc;
    if (int rc = log_modulus_ok(c, "bmi_compress_batch_host", log_modulus)) return rc;
    if (count == 0) return 0;
    u64 words = 0;
    (void)bmi_compressed_words(c, count, &words);
    Stage s;
    const auto d_in = s.upload(in, (size_t)count * (c->N + 1));
    const auto d_out = s.download(out, words);
    return s.run(c, [&] { return bmi_compress_batch(c, s[d_in], count, log_modulus, s[d_out], c->stream); });
}

int bmi_phase_compressed(const bmi_ctx *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint64_t *phase) {
    return hc::phase_compressed(c, data, count, log_modulus, phase);
}

int bmi_decrypt_compressed(const bmi_ctx *c, const uint32_t *data, uint32_t count, uint32_t log_modulus, uint32_t delta_log, int64_t *msgs) {
    return hc::decrypt_compressed(c, data, count, log_modulus, delta_log, msgs);
}

// Decompression (lwe_unpack.hip) needs no key of any kind: the modulus, the shape and the arguments are all it checks.
static int decompression_ok(const bmi_ctx *c, const char *what, uint32_t count, uint32_t log_modulus, bool has_index, uint32_t rows) {
    if (!c->t64())
        return fail(c, -1, std::string(what) + ": compression of output ciphertexts exists on the 2^64 torus only (not on the 49-bit field or "
                           "Goldilocks)");
    if (c->big_n != c->N) return fail(c, -1, std::string(what) + ": compressed ciphertexts exist for k = 1 only");
    if (int rc = log_modulus_ok(c, what, log_modulus)) return rc;
    if (!has_index && rows != count)
        return fail(c, -1, std::string(what) + ": without an index the rows are the positions 0 .. count - 1: rows must equal count (" +
                           std::to_string(rows) + " rows asked of " + std::to_string(count) + " ciphertexts)");
    if (rows && !count) return fail(c, -1, std::string(what) + ": rows asked of an empty compressed form");
    return 0;
}

int bmi_decompress_batch(bmi_ctx *c, const uint32_t *d_in, uint32_t count, uint32_t log_modulus, const uint32_t *d_index, uint32_t rows,
                         uint64_t *d_out, void *stream) {
    if (!c || (rows && (!d_in || !d_out))) return -1;
    if (int rc = decompression_ok(c, "bmi_decompress_batch", count, log_modulus, d_index != nullptr, rows)) return rc;
    if (rows == 0) return 0;
    if ((uintptr_t)d_out & 7) return fail(c, -1, "bmi_decompress_batch: d_out is not aligned to 8 bytes");
    HIP_OK(c, hipSetDevice(c->device));
    return launched(c, "lwe_unpack launch: ", bmit::launch_unpack(d_in, d_index, d_out, count, rows, c->N, log_modulus, (hipStream_t)stream));
}

int bmi_decompress_batch_host(bmi_ctx *c, const uint32_t *in, uint32_t count, uint32_t log_modulus, const uint32_t *index, uint32_t rows,
                              uint64_t *out) {
    if (!c || (rows && (!in || !out))) return -1;
    if (int rc = decompression_ok(c, "bmi_decompress_batch_host", count, log_modulus, index != nullptr, rows)) return rc;
    if (rows == 0) return 0;
    if (index)
        for (uint32_t r = 0; r < rows; r++)
            if (index[r] >= count)
                return fail(c, -1, "bmi_decompress_batch_host: index " + std::to_string(index[r]) + " (row " + std::to_string(r) +
                                   ") is not below the count of " + std::to_string(count) + " ciphertexts");
    u64 words = 0;
    (void)bmi_compressed_words(c, count, &words);
    if (log_modulus < 32)
        for (u64 x = 0; x < words; x++)
            if (in[x] >> log_modulus) return fail(c, -1, "bmi_decompress_batch_host: a value does not fit log_modulus bits");
    Stage s;
    const auto d_in = s.upload(in, words);
    const auto d_index = s.upload(index, index ? rows : 0);
    const auto d_out = s.download(out, (size_t)rows * (c->N + 1));
    return s.run(c, [&] {
        return bmi_decompress_batch(c, s[d_in], count, log_modulus, index ? s[d_index] : nullptr, rows, s[d_out], c->stream);
    });
}

}  // extern "C"
