#!/usr/bin/env python3
"""Rounds 4 and 5 of PLONK for many witnesses against the loops they replace, on data resident in HBM: for every (log_n, rows) and each of
zk_bn254_plonk_linearize_batch_dev and zk_bn254_plonk_open_batch_dev the wall ms of ONE call over all rows and of a loop of `rows` one-row calls of the same
entry (the same kernels with one row in the grid; being calls with workspace, each ends in a synchronise, as a caller of that entry gets it) -- best of --reps
windows of --inner calls after one untimed run.  The key is tools/plonk_quotient_bench.py's synthetic circuit; the rows are uniform canonical images with their
own challenges -- no witness: the launches and their work do not depend on it.  Round 5 reads the fh and lin that round 4 wrote.  The bytes of batch and loop
are compared before anything is timed.  Prints one JSON line.
usage: python tools/plonk_open_bench.py [--shapes 10:256,12:64,16:16] [--npub 4] [--reps 5] [--inner 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noir_backend_using_gnark_amd import _lib  # noqa: E402
from tools.plonk_quotient_bench import _random, best_ms, synthetic_key  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:256,12:64,16:16", help="log_n:rows, comma-separated")
    ap.add_argument("--npub", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    out = {"reps": a.reps, "inner": a.inner, "npub": a.npub, "entries": ["zk_bn254_plonk_linearize_batch_dev", "zk_bn254_plonk_open_batch_dev"], "shapes": []}
    for log_n, rows in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        n = 1 << log_n
        keep, stride = 3 * (n + 2), n + 3
        pk, srs = synthetic_key(L, log_n, a.npub)
        l, r, o, z = (_random(L, rows * stride, 11 + k) for k in range(4))
        h = _random(L, rows * keep, 20)
        alpha, beta, gamma, zeta, kg = (_random(L, rows, 21 + k) for k in range(5))
        new = lambda elems: [_lib.DeviceBuffer(elems * 32) for _ in range(2)]
        values, zquot, lin, fh, q, value = new(rows * 8), new(rows * stride), new(rows * stride), new(rows * stride), new(rows * (n + 2)), new(rows)
        p = lambda b, off=0: C.c_void_p(b.ptr + off)

        def linearize(k, first, cnt):
            at, c = first * stride * 32, first * 32
            _lib.check(L.zk_bn254_plonk_linearize_batch_dev(pk.handle, p(l, at), p(r, at), p(o, at), p(z, at), C.c_size_t(stride), p(h, first * keep * 32),
                                                            C.c_size_t(keep), C.c_size_t(cnt), p(alpha, c), p(beta, c), p(gamma, c), p(zeta, c), p(values[k], 8 * c),
                                                            p(zquot[k], at), p(lin[k], at), p(fh[k], at), C.c_size_t(stride), None))

        def open_(k, first, cnt):
            at, c = first * stride * 32, first * 32
            _lib.check(L.zk_bn254_plonk_open_batch_dev(pk.handle, p(fh[0], at), p(lin[0], at), p(l, at), p(r, at), p(o, at), C.c_size_t(stride), C.c_size_t(cnt),
                                                       p(zeta, c), p(kg, c), p(q[k], first * (n + 2) * 32), C.c_size_t(n + 2), p(value[k], c), None))

        def loop_of(fn):
            def run():
                for i in range(rows):
                    fn(1, i, 1)
            return run

        row = {"log_n": log_n, "rows": rows}
        for name, fn, outs in (("linearize", linearize, ((values, rows * 8), (zquot, rows * stride), (lin, rows * stride), (fh, rows * stride))),
                               ("open", open_, ((q, rows * (n + 2)), (value, rows)))):
            batch, loop = (lambda fn=fn: fn(0, 0, rows)), loop_of(fn)
            for pair, _ in outs:          # the elements between rows are not written: the same bytes there in both
                for b in pair:
                    _lib.check(L.zk_bn254_fr_random_dev(C.c_void_p(b.ptr), C.c_size_t(b.nbytes // 32), C.c_uint64(99), C.c_int(1), C.c_int(0), None))
            batch()
            loop()
            same = all(bool((pair[0].to_numpy(np.uint64, (cnt, 4)) == pair[1].to_numpy(np.uint64, (cnt, 4))).all()) for pair, cnt in outs)
            assert same, (log_n, rows, name)
            e = {"bytes_equal": same, "batch": {"ms": round(best_ms(batch, a.reps, a.inner), 4)}, "loop": {"ms": round(best_ms(loop, a.reps, a.inner), 4)}}
            e["loop_over_batch"] = round(e["loop"]["ms"] / e["batch"]["ms"], 2)
            row[name] = e
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        for b in [l, r, o, z, h, alpha, beta, gamma, zeta, kg] + values + zquot + lin + fh + q + value:
            b.free()
        pk.free()
        srs.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
