"""Batch Groth16 verification against many keys: N proofs spread evenly over K keys (blocks of N / K rows), wall-clock ms, best of --reps after a checked
warm-up call:
  keys        (a) ONE zk_bn254_groth16_verify_batch_keys call over the N rows and the K keys
  keys_fb     (a') the same with one "Krs + D" row in the middle: the chunk goes through the per-lane fallback
  loop        (b) K calls of zk_bn254_groth16_verify_batch, each on its key's N / K rows -- what a verifier serving K circuits had to do before
  one_key     (c) one zk_bn254_groth16_verify_batch call of N rows under a single key: the floor
  parse       the new entry with the K keys and NO rows: the keys are parsed and nothing is launched -- the host's share of (a) that grows with K
The keys and proofs are forged under known discrete logarithms as the tests forge them (tests/groth16_forge.py: one public input); the work per proof does not
depend on the data.  Every timed call is checked for its verdicts once, outside the timing.  Prints one JSON line.
usage: python tools/groth16_verify_keys_bench.py [--sizes 256,4096] [--keys 1,16,256] [--reps 3] [--modes keys,keys_fb,loop,one_key,parse] [--lib PATH]
(--modes: time only these, for a profiler run of one path; --lib: another build of libzkmi.so, e.g. the parent commit's for column (c))"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from noir_backend_using_gnark_amd import _lib  # noqa: E402
from noir_backend_using_gnark_amd import verify as zv  # noqa: E402
from tests import groth16_forge as gf  # noqa: E402


def best_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,4096")
    ap.add_argument("--keys", default="1,16,256")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--modes", default="keys,keys_fb,loop,one_key,parse")
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    if a.lib:
        import ctypes
        _lib.use_library(os.path.abspath(a.lib))
        probe = ctypes.CDLL(os.path.abspath(a.lib))
        _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s)]         # an earlier build lacks the entries added since
    modes = a.modes.split(",")
    sizes, counts = [int(x) for x in a.sizes.split(",")], [int(x) for x in a.keys.split(",")]
    f = gf._rng(0xBE7C)
    keys, good = [], []
    for j in range(max(counts)):
        k = gf.ToyKey(f(), f(), f(), f(), [f(), f()])
        w = [f()]
        keys.append(k)
        good.append(gf.Case("accept", k, k.forge(f(), f(), w), gf.limbs(w), 1))
    out = {"reps": a.reps, "lib": a.lib, "rows": []}
    for n in sizes:
        for K in counts:
            if n % K:
                continue
            per = n // K
            vks = [k.bytes for k in keys[:K]]
            key_of = np.repeat(np.arange(K, dtype=np.uint32), per)
            blob = b"".join(c.proof * per for c in good[:K])
            pubs = np.concatenate([np.stack([c.pub] * per) for c in good[:K]])
            row = {"n": n, "keys": K}
            if "keys" in modes:
                assert zv.groth16_verify_batch_keys(blob, vks, key_of, pubs).all()
                row["keys_ms"] = round(best_ms(lambda: zv.groth16_verify_batch_keys(blob, vks, key_of, pubs), a.reps), 3)
            if "keys_fb" in modes:
                at = n // 2
                rej = gf.reject_case(keys[key_of[at]])
                bad = blob[:128 * at] + rej.proof + blob[128 * (at + 1):]
                pubs_bad = pubs.copy()
                pubs_bad[at] = rej.pub
                assert list(np.flatnonzero(~zv.groth16_verify_batch_keys(bad, vks, key_of, pubs_bad))) == [at]
                row["keys_fb_ms"] = round(best_ms(lambda: zv.groth16_verify_batch_keys(bad, vks, key_of, pubs_bad), a.reps), 3)
            if "loop" in modes:
                parts = [(good[j].proof * per, vks[j], np.stack([good[j].pub] * per)) for j in range(K)]
                loop = lambda: [zv.groth16_verify_batch(p, vk, pu) for p, vk, pu in parts]  # noqa: E731
                assert all(v.all() for v in loop())
                row["loop_ms"] = round(best_ms(loop, a.reps), 3)
            if "one_key" in modes:
                one = (good[0].proof * n, vks[0], np.stack([good[0].pub] * n))
                assert zv.groth16_verify_batch(one[0], one[1], one[2]).all()
                row["one_key_ms"] = round(best_ms(lambda: zv.groth16_verify_batch(one[0], one[1], one[2]), a.reps), 3)
            if "parse" in modes:
                none = np.zeros((0, 1, 4), np.uint64)
                row["parse_ms"] = round(best_ms(lambda: zv.groth16_verify_batch_keys(b"", vks, [], none), a.reps + 1), 3)
            if "keys_ms" in row and "one_key_ms" in row:
                row["keys_over_one_key"] = round(row["keys_ms"] / row["one_key_ms"], 3)
            if "keys_ms" in row and "loop_ms" in row:
                row["loop_over_keys"] = round(row["loop_ms"] / row["keys_ms"], 2)
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
