#!/usr/bin/env python3
"""Round 3 of PLONK for many witnesses against the loop it replaces, on data resident in HBM: for every (log_n, rows) the wall ms of ONE
zk_bn254_plonk_quotient_batch_dev call over all rows and of a loop of `rows` one-row calls of the same entry (the same kernels with one row in the grid; being
calls with workspace, each ends in a synchronise, as a caller of that entry gets it) -- best of --reps windows of --inner calls after one untimed run.  The key
is a synthetic circuit's (random wiring and selectors, --npub public inputs); the rows are uniform canonical images with their own public inputs and challenges
-- no witness, so every verdict is 1: the launches and their work do not depend on it.  The bytes of the two, verdicts included, are compared before anything
is timed.  Prints one JSON line.
usage: python tools/plonk_quotient_bench.py [--shapes 10:256,12:64,16:16] [--npub 4] [--reps 5] [--inner 5]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noir_backend_using_gnark_amd import _lib  # noqa: E402
from noir_backend_using_gnark_amd import bn254 as zb  # noqa: E402
from noir_backend_using_gnark_amd import plonk as zp  # noqa: E402

R_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def best_ms(fn, reps, inner):
    fn()  # untimed: tables, code objects, the arena at its size
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        t.append((time.perf_counter() - t0) * 1e3 / inner)
    return min(t)


def _random(L, cnt, seed):
    b = _lib.DeviceBuffer(max(cnt, 1) * 32)
    _lib.check(L.zk_bn254_fr_random_dev(C.c_void_p(b.ptr), C.c_size_t(cnt), C.c_uint64(seed), C.c_int(1), C.c_int(0), None))
    return b


def synthetic_key(L, log_n, npub):
    """plonk.Setup of a circuit that fills the domain of 2^log_n rows: random wiring over n / 2 variables, random selectors and constants"""
    n = 1 << log_n
    nc, nvars = n - npub, max(n // 2, npub + 1)
    d_srs = _lib.DeviceBuffer((n + 3) * 64)
    a_m = np.frombuffer((0xA1FA0123456789ABCDEF * (1 << 256) % R_FR).to_bytes(32, "little"), dtype=np.uint64).copy()
    _lib.check(L.zk_bn254_kzg_new_srs_dev(C.c_void_p(d_srs.ptr), C.c_size_t(n + 3), _lib.vp(a_m), None, None))
    srs = zb.ResidentBases(d_srs, n=n + 3)
    rng = np.random.default_rng(log_n)
    xa, xb, xc = (rng.integers(0, nvars, nc, dtype=np.uint32) for _ in range(3))
    coef = [_random(L, nc, sd) for sd in (1, 2, 3, 4, 5)]
    pk = zp.setup(zp.Circuit(npub, nvars, *coef, xa, xb, xc), srs)
    for b in coef:
        b.free()
    return pk, srs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:256,12:64,16:16", help="log_n:rows, comma-separated")
    ap.add_argument("--npub", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    out = {"reps": a.reps, "inner": a.inner, "npub": a.npub, "entry": "zk_bn254_plonk_quotient_batch_dev", "shapes": []}
    for log_n, rows in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        n = 1 << log_n
        keep, stride = 3 * (n + 2), n + 3
        pk, srs = synthetic_key(L, log_n, a.npub)
        l, r, o, z = (_random(L, rows * stride, 11 + k) for k in range(4))
        pub = _random(L, rows * a.npub, 20)
        alpha, beta, gamma = (_random(L, rows, 21 + k) for k in range(3))
        h = [_lib.DeviceBuffer(rows * keep * 32) for _ in range(2)]
        st = [_lib.DeviceBuffer(rows * 4) for _ in range(2)]
        p = lambda b, off=0: C.c_void_p(b.ptr + off)

        def call(k, first, cnt):
            at, c = first * stride * 32, first * 32
            _lib.check(L.zk_bn254_plonk_quotient_batch_dev(pk.handle, p(l, at), p(r, at), p(o, at), p(z, at), C.c_size_t(stride), p(pub, first * a.npub * 32),
                                                           C.c_size_t(a.npub), C.c_size_t(cnt), p(alpha, c), p(beta, c), p(gamma, c), p(h[k], first * keep * 32),
                                                           C.c_size_t(keep), p(st[k], first * 4), None))

        def batch():
            call(0, 0, rows)

        def loop():
            for i in range(rows):
                call(1, i, 1)

        batch()
        loop()
        same = bool((h[0].to_numpy(np.uint64, (rows * keep, 4)) == h[1].to_numpy(np.uint64, (rows * keep, 4))).all()
                    and (st[0].to_numpy(np.int32, (rows,)) == st[1].to_numpy(np.int32, (rows,))).all())
        assert same, (log_n, rows)
        row = {"log_n": log_n, "rows": rows, "bytes_equal": same, "workspace_mib": round(min(rows * 5 * 4 * n * 32, 1 << 30) / 2 ** 20, 1)}
        for name, fn in (("batch", batch), ("loop", loop)):
            row[name] = {"ms": round(best_ms(fn, a.reps, a.inner), 4)}
        row["loop_over_batch"] = round(row["loop"]["ms"] / row["batch"]["ms"], 2)
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        for b in [l, r, o, z, pub, alpha, beta, gamma] + h + st:
            b.free()
        pk.free()
        srs.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
