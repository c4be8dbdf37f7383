#!/usr/bin/env python3
"""Row-batched commitments against the loops they replace, on scalars resident in HBM: for every (log_n, rows) and for dense (uniform Montgomery images) and
wire-like (0 / 1 / small, regular form) rows the wall ms of
    rows    ONE call of zk_bn254_msm_bases_rows_dev over all rows (points and compressed digests stay on the device)
    single  a loop of `rows` calls of zk_bn254_msm_bases_dev
    threes  a loop of zk_bn254_msm_bases_batch_dev over threes of rows (the widest batch that entry shares one preparation among)
-- best of --reps windows of --inner calls after one untimed run.  The bases are a KZG SRS of 2^log_n points with the window table the planner picks for that
size (below 4,096 bases none is built by default; the width is asked for here, so that all three run against the same table).  The bytes of all three are compared
before anything is timed.  Prints one JSON line.
usage: python tools/msm_rows_bench.py [--shapes 10:256,12:64,16:16] [--reps 5] [--inner 5]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from noir_backend_using_gnark_amd import _lib  # noqa: E402
from noir_backend_using_gnark_amd import bn254 as zb  # noqa: E402
from tools.plonk_quotient_bench import R_FR, _random, best_ms  # noqa: E402


def wire_like(rows, n, seed):
    """regular-form scalars: half zeros, a quarter ones, the rest 16- and 40-bit words"""
    g = np.random.default_rng(seed)
    kind = g.integers(0, 8, size=(rows, n))
    m = np.zeros((rows, n, 4), np.uint64)
    m[:, :, 0] = np.where(kind < 4, 0, np.where(kind < 6, 1, np.where(kind < 7, g.integers(0, 1 << 16, size=(rows, n)), g.integers(0, 1 << 40, size=(rows, n))))).astype(np.uint64)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:256,12:64,16:16", help="log_n:rows, comma-separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_device()
    out = {"reps": a.reps, "inner": a.inner, "entries": ["zk_bn254_msm_bases_rows_dev", "zk_bn254_msm_bases_dev", "zk_bn254_msm_bases_batch_dev"], "shapes": []}
    for log_n, rows in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        n = 1 << log_n
        d_srs = _lib.DeviceBuffer(n * 64)
        alpha = np.frombuffer((0xA1FA0123456789ABCDEF * (1 << 256) % R_FR).to_bytes(32, "little"), dtype=np.uint64).copy()
        _lib.check(L.zk_bn254_kzg_new_srs_dev(C.c_void_p(d_srs.ptr), C.c_size_t(n), _lib.vp(alpha), None, None))
        c, digits = C.c_uint32(0), C.c_uint32(0)
        _lib.check(L.zk_bn254_msm_plan_info(C.c_size_t(n), C.c_int(1), C.byref(c), C.byref(digits)))
        srs = zb.ResidentBases(d_srs, n=n, table_window_bits=int(c.value))
        d_srs.free()
        info = zb.msm_rows_info(srs, n)
        row = {"log_n": log_n, "rows": rows, "table_window_bits": int(c.value), "chunk_rows": info["chunk_rows"], "batched": info["batched"]}
        d_out, d_enc = _lib.DeviceBuffer(rows * 64), _lib.DeviceBuffer(rows * 32)
        for kind in ("dense", "wire_like"):
            if kind == "dense":
                sc, cfg, flags = _random(L, rows * n, 7 + log_n), _lib.MsmCfg(0, 1, 0, 0), 0
            else:
                sc, cfg, flags = _lib.DeviceBuffer.from_numpy(wire_like(rows, n, 9 + log_n)), _lib.MsmCfg(0, 0, 0, 0), zb.MSM_ROWS_SPARSE
            at = lambda v: C.c_void_p(sc.ptr + v * n * 32)  # noqa: E731
            one, three = np.zeros((rows, 8), np.uint64), np.zeros((rows, 8), np.uint64)

            def batched():
                _lib.check(L.zk_bn254_msm_bases_rows_dev(srs.handle, C.c_size_t(0), at(0), C.c_size_t(n), C.c_size_t(n), C.c_size_t(rows), C.byref(cfg), C.c_uint32(flags),
                                                         C.c_void_p(d_out.ptr), C.c_void_p(d_enc.ptr)))

            def single():
                for v in range(rows):
                    _lib.check(L.zk_bn254_msm_bases_dev(srs.handle, C.c_size_t(0), at(v), C.c_size_t(n), C.byref(cfg), C.c_void_p(one[v].ctypes.data)))

            def threes():
                for v in range(0, rows, 3):
                    k = min(3, rows - v)
                    ptrs = (C.c_void_p * k)(*[sc.ptr + (v + j) * n * 32 for j in range(k)])
                    _lib.check(L.zk_bn254_msm_bases_batch_dev(srs.handle, C.c_size_t(0), ptrs, C.c_uint32(k), C.c_size_t(n), C.byref(cfg), C.c_void_p(three[v].ctypes.data)))

            batched()
            single()
            threes()
            got = d_out.to_numpy(np.uint64, (rows, 8))
            same = bool((got == one).all() and (got == three).all())
            assert same, (log_n, rows, kind)
            e = {"bytes_equal": same}
            for name, fn in (("rows", batched), ("single", single), ("threes", threes)):
                e[name] = {"ms": round(best_ms(fn, a.reps, a.inner), 4)}
            e["single_over_rows"] = round(e["single"]["ms"] / e["rows"]["ms"], 2)
            e["threes_over_rows"] = round(e["threes"]["ms"] / e["rows"]["ms"], 2)
            row[kind] = e
            sc.free()
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        for b in (d_out, d_enc):
            b.free()
        srs.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
