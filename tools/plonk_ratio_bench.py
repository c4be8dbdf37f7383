#!/usr/bin/env python3
"""Round 2 of PLONK for many witnesses against the loop it replaces, on data resident in HBM: for every (log_n, rows) the wall ms of ONE
zk_bn254_iop_ratio_copy_batch_dev call over all rows and of a loop of `rows` one-row calls of the same entry -- which launches the five kernels
zk_bn254_plonk_prove launches for its round 2 (and, being a call with workspace, ends in a synchronise, as a caller of that entry gets it) -- best of --reps
windows of --inner calls after one untimed run.  The rows are uniform canonical images, the permutation is uniformly random, every row has its own
challenges; the bytes of the two are compared before anything is timed.  Prints one JSON line.
usage: python tools/plonk_ratio_bench.py [--shapes 10:256,12:64,16:16] [--reps 5] [--inner 10]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import noir_backend_using_gnark_amd as zk  # noqa: E402
from noir_backend_using_gnark_amd import _lib  # noqa: E402


def best_ms(fn, reps, inner):
    fn()  # untimed: tables, code objects, the arena at its size
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        t.append((time.perf_counter() - t0) * 1e3 / inner)
    return min(t)


def launches(log_n, rows):
    """kernel launches of one call: (batched, loop of one-row calls)"""
    n = 1 << log_n
    K = max(8, (n + 256 * 1024 - 1) // (256 * 1024))
    nb = ((n + K - 1) // K + 255) // 256
    return (5 if rows == 1 else 3 if nb == 1 else 5), 5 * rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:256,12:64,16:16", help="log_n:rows, comma-separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    out = {"reps": a.reps, "inner": a.inner, "entry": "zk_bn254_iop_ratio_copy_batch_dev", "shapes": []}
    for log_n, rows in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        n = 1 << log_n
        l, r, o = (_random(L, rows * n, 11 + k) for k in range(3))
        beta, gamma = _random(L, rows, 21), _random(L, rows, 22)
        sigma = zk.permutation_sigma(np.random.default_rng(log_n).permutation(3 * n).astype(np.uint32))
        z = [_lib.DeviceBuffer(rows * n * 32) for _ in range(2)]
        p = lambda b, off=0: C.c_void_p(b.ptr + off)

        def batch():
            _lib.check(L.zk_bn254_iop_ratio_copy_batch_dev(p(l), p(r), p(o), C.c_size_t(n), C.c_uint32(log_n), C.c_size_t(rows), p(sigma), p(beta), p(gamma), p(z[0]),
                                                           C.c_size_t(n), None))

        def loop():
            for i in range(rows):
                at = i * n * 32
                _lib.check(L.zk_bn254_iop_ratio_copy_batch_dev(p(l, at), p(r, at), p(o, at), C.c_size_t(n), C.c_uint32(log_n), C.c_size_t(1), p(sigma), p(beta, 32 * i),
                                                               p(gamma, 32 * i), p(z[1], at), C.c_size_t(n), None))

        batch()
        loop()
        same = bool((z[0].to_numpy(np.uint64, (rows * n, 4)) == z[1].to_numpy(np.uint64, (rows * n, 4))).all())
        assert same, (log_n, rows)
        nl = launches(log_n, rows)
        row = {"log_n": log_n, "rows": rows, "bytes_equal": same, "launches": {"batch": nl[0], "loop": nl[1]}}
        for name, fn in (("batch", batch), ("loop", loop)):
            row[name] = {"ms": round(best_ms(fn, a.reps, a.inner), 4)}
        row["loop_over_batch"] = round(row["loop"]["ms"] / row["batch"]["ms"], 2)
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        for b in [l, r, o, beta, gamma, sigma] + z:
            b.free()
    print(json.dumps(out))


def _random(L, cnt, seed):
    b = _lib.DeviceBuffer(cnt * 32)
    _lib.check(L.zk_bn254_fr_random_dev(C.c_void_p(b.ptr), C.c_size_t(cnt), C.c_uint64(seed), C.c_int(1), C.c_int(0), None))
    return b


if __name__ == "__main__":
    main()
