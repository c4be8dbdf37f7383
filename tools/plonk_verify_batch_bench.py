"""Batch PLONK verification: ms and proofs/s of zk_bn254_plonk_verify_batch for an all-valid batch (the batched check) and for a batch with one bad proof
(the per-proof fallback), and the host verifier zk_bn254_plonk_verify in a loop on 1 and 16 Python threads (ctypes releases the GIL; the host loop is timed
on min(N, HOST_CAP) proofs and reported per proof).  The proof is the committed fixture of the reference's first demo circuit (one public input), tiled:
the work per proof does not depend on the data.  Prints one JSON line.
usage: python tools/plonk_verify_batch_bench.py [--sizes 1,64,1024,4096,16384] [--reps 3]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from noir_backend_using_gnark_amd import verify as zv  # noqa: E402
from oracle import bn254_ref as ref  # noqa: E402
from tests.helpers import h2i, mont_limbs  # noqa: E402

HOST_CAP = 128


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "plonk_golden.json")) as f:
        e = json.load(f)[0]
    g2 = np.stack([np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64) for P in (ref.G2_GEN, ref.g2_mul(ref.G2_GEN, h2i(e["srs_alpha"])))])
    return bytes.fromhex(e["vk_hex"]), g2, bytes.fromhex(e["proof"]), mont_limbs([h2i(v) for v in e["solution"][:e["n_public"]]])


def best_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def zshift_negated(proof):
    """the same proof with ZShiftH replaced by -ZShiftH (the sign flag flipped): a valid encoding, rejected by the shifted opening alone"""
    b = bytearray(proof)
    b[484] ^= 0x40
    return bytes(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    vk, g2, proof, pub = golden()
    out = {"batch": {}, "fallback": {}, "host_1t": {}, "host_16t": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        pr = proof * n
        pu = np.stack([pub] * n)
        assert zv.plonk_verify_batch(pr, vk, g2, pu).all()
        ms = best_ms(lambda: zv.plonk_verify_batch(pr, vk, g2, pu), a.reps)
        out["batch"][n] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
        k = n // 2
        bad = pr[:548 * k] + zshift_negated(proof) + pr[548 * (k + 1):]
        assert (~zv.plonk_verify_batch(bad, vk, g2, pu)).sum() == 1
        ms = best_ms(lambda: zv.plonk_verify_batch(bad, vk, g2, pu), a.reps)
        out["fallback"][n] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
        m = min(n, HOST_CAP)
        ms1 = best_ms(lambda: [zv.plonk_verify(proof, vk, g2, pub) for _ in range(m)], 1)
        out["host_1t"][n] = {"ms_per_proof": round(ms1 / m, 3), "proofs_per_s": round(m / ms1 * 1e3, 1)}
        with ThreadPoolExecutor(16) as ex:
            ms16 = best_ms(lambda: list(ex.map(lambda i: zv.plonk_verify(proof, vk, g2, pub), range(m))), 1)
        out["host_16t"][n] = {"ms_per_proof": round(ms16 / m, 3), "proofs_per_s": round(m / ms16 * 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
