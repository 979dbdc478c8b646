"""Wall-clock of key generation in one process: tfhe.Engine on the build BMI_TFHE_LIB names (default: the product build), or with
--client bmi_amd.client.ClientEngine (libbmi_client.so: the same host code without the uploads and key conversions).  Default torus
set; one untimed keygen(seed) (the code objects load), three timed ones, compression_keygen(1, 16), one CSPRNG keygen().  One line of
milliseconds; run parent build and client alternating, one process each (profiles/client_library_ab.txt, recipe of
profiles/host_crypto_ab.txt section 5).

    BMI_TFHE_LIB=/path/to/parent/libbmi_tfhe.so python tools/client_keygen_ab.py
    python tools/client_keygen_ab.py --client"""
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [HERE, os.path.join(HERE, "bounty-matrix-inversion_amd")]


def ms(f):
    t = time.perf_counter()
    f()
    return (time.perf_counter() - t) * 1e3


def main():
    if "--client" in sys.argv[1:]:
        from bmi_amd.client import ClientEngine
        label, e = "client", ClientEngine()
    else:
        from bmi_amd import tfhe
        if os.environ.get("BMI_TFHE_LIB"):
            tfhe.LIB_PATH = os.environ["BMI_TFHE_LIB"]
        label, e = "engine " + os.path.basename(os.path.dirname(os.path.dirname(tfhe.LIB_PATH))), tfhe.Engine()
    first = ms(lambda: e.keygen(0x5EED))
    timed = [ms(lambda: e.keygen(0x5EED)) for _ in range(3)]
    pk = ms(lambda: e.compression_keygen(1, 16))
    secure = ms(e.keygen)
    e.close()
    print(f"{label:24s} first {first:7.1f}   timed {timed[0]:7.1f} {timed[1]:7.1f} {timed[2]:7.1f}   compression_keygen(1, 16) {pk:7.1f}   "
          f"keygen() (CSPRNG) {secure:7.1f}", flush=True)


if __name__ == "__main__":
    main()
