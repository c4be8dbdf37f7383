"""Batch Groth16 verification and device pairings: ms and proofs/s of zk_bn254_groth16_verify_batch for an all-valid batch (the batched check) and for
a batch with one bad proof (the per-proof fallback), zk_bn254_pair for n = 1 and 64, and the host verifier zk_bn254_groth16_verify in a loop on 1 and 16
Python threads (ctypes releases the GIL; the host loop is timed on min(N, HOST_CAP) proofs and reported per proof).  Proofs are the committed golden
proofs of one key, tiled (the work is data-independent).  Prints one JSON line.
usage: python tools/verify_batch_bench.py [--sizes 1,64,1024,4096,16384] [--reps 3]"""
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
from tests.helpers import g1_points_from_scalars, g2_points_from_scalars, h2i, mont_limbs  # noqa: E402

HOST_CAP = 256


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "bn254_golden.json")) as f:
        g = json.load(f)
    with open(os.path.join(ROOT, "tests", "golden", "groth16_wire_golden.json")) as f:
        wire = {e["name"]: e for e in json.load(f)}
    items = [e for e in g["groth16"] if e["name"].startswith("seq_r1cs_13")]
    vk = bytes.fromhex(wire["seq_r1cs_13"]["vk_hex"])
    return vk, [bytes.fromhex(e["proof"]) for e in items], [mont_limbs([h2i(v) for v in e["w"][1:e["n_public"]]]) for e in items]


def best_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    vk, proofs, pubs = golden()
    out = {"batch": {}, "fallback": {}, "host_1t": {}, "host_16t": {}}
    for n in [int(x) for x in a.sizes.split(",")]:
        pr = [proofs[i % len(proofs)] for i in range(n)]
        pu = np.stack([pubs[i % len(pubs)] for i in range(n)])
        assert zv.groth16_verify_batch(pr, vk, pu).all()
        ms = best_ms(lambda: zv.groth16_verify_batch(pr, vk, pu), a.reps)
        out["batch"][n] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
        bad = list(pr)
        bad[n // 2] = krs_negated(pr[n // 2])
        assert (~zv.groth16_verify_batch(bad, vk, pu)).sum() == 1
        ms = best_ms(lambda: zv.groth16_verify_batch(bad, vk, pu), a.reps)
        out["fallback"][n] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
        m = min(n, HOST_CAP)
        ms1 = best_ms(lambda: [zv.groth16_verify(pr[i], vk, pu[i]) for i in range(m)], 1)
        out["host_1t"][n] = {"ms_per_proof": round(ms1 / m, 3), "proofs_per_s": round(m / ms1 * 1e3, 1)}
        with ThreadPoolExecutor(16) as ex:
            ms16 = best_ms(lambda: list(ex.map(lambda i: zv.groth16_verify(pr[i], vk, pu[i]), range(m))), 1)
        out["host_16t"][n] = {"ms_per_proof": round(ms16 / m, 3), "proofs_per_s": round(m / ms16 * 1e3, 1)}
    out["pair"] = {}
    for n in (1, 64):
        P, Q = g1_points_from_scalars(range(3, 3 + n)), g2_points_from_scalars(range(5, 5 + n))
        zv.pair(P, Q)
        out["pair"][n] = {"ms": round(best_ms(lambda: zv.pair(P, Q), a.reps), 3)}
    print(json.dumps(out))


def krs_negated(proof):
    """the same proof with Krs replaced by -Krs (the sign flag flipped): still a valid encoding, a rejected proof"""
    b = bytearray(proof)
    b[96] ^= 0x40
    return bytes(b)


if __name__ == "__main__":
    main()
