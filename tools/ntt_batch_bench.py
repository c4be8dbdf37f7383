#!/usr/bin/env python3
"""Row-batched transforms against the loop they replace, on data resident in HBM: for every (log_n, rows) the wall ms of ONE zk_bn254_ntt_batch_dev call over all
rows and of a loop of `rows` zk_bn254_ntt_dev calls (default stream: each call ends in its synchronise, as a caller of that entry gets it), best of --reps after
one untimed run, and the algorithmic bytes per second of both (64 B per element per transform: read + write once).  The bytes of the two are compared before
anything is timed.  Prints one JSON line.
usage: python tools/ntt_batch_bench.py [--log-n 10,12,14,16] [--rows 16,256] [--reps 5] [--inner 20]"""
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
    fn()  # untimed: tables, code objects
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        t.append((time.perf_counter() - t0) * 1e3 / inner)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="10,12,14,16")
    ap.add_argument("--rows", default="16,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    out = {"reps": a.reps, "inner": a.inner, "mode": "FFT, DIF, no coset", "shapes": []}
    for log_n in [int(x) for x in a.log_n.split(",")]:
        n = 1 << log_n
        for rows in [int(x) for x in a.rows.split(",")]:
            d = [_lib.DeviceBuffer(rows * n * 32) for _ in range(2)]
            for b in d:  # the same canonical images in both
                _lib.check(L.zk_bn254_fr_random_dev(C.c_void_p(b.ptr), C.c_size_t(rows * n), C.c_uint64(7), C.c_int(1), C.c_int(0), None))

            def batch(p=d[0].ptr):
                _lib.check(L.zk_bn254_ntt_batch_dev(C.c_void_p(p), C.c_uint32(log_n), C.c_size_t(rows), C.c_size_t(n), C.c_int(0), C.c_int(zk.DIF), C.c_int(0), None))

            def loop(p=d[1].ptr):
                for i in range(rows):
                    _lib.check(L.zk_bn254_ntt_dev(C.c_void_p(p + i * n * 32), C.c_uint32(log_n), C.c_int(0), C.c_int(zk.DIF), C.c_int(0), None))

            batch()
            loop()
            same = bool((d[0].to_numpy(np.uint64, (rows * n, 4)) == d[1].to_numpy(np.uint64, (rows * n, 4))).all())
            assert same, (log_n, rows)
            row = {"log_n": log_n, "rows": rows, "bytes_equal": same}
            for name, fn in (("batch", batch), ("loop", loop)):
                ms = best_ms(fn, a.reps, a.inner)
                row[name] = {"ms": round(ms, 4), "algorithmic_GBps": round(64 * n * rows / ms / 1e6, 1)}
            row["batch_over_loop"] = round(row["loop"]["ms"] / row["batch"]["ms"], 2)
            out["shapes"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            for b in d:
                b.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
