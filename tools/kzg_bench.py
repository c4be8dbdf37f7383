"""KZG openings: ms of SRS.open against SRS.commit of the same length (the commit path is the yardstick: an opening is one scan set plus one commitment),
open_many with 2 and 3 rows against as many single calls, batch_open_single_point of seven polynomials, and zk_bn254_kzg_verify_batch for an all-true batch
(the combined check) and a batch with one wrong opening (the per-opening fallback) against the host zk_bn254_kzg_verify in a loop on 1 and 16 Python threads
(ctypes releases the GIL; the host loop is timed on min(N, HOST_CAP) openings and reported per opening).  Polynomials are device-resident random field
elements; the verified opening is one true opening over a 64-point SRS, tiled: the work per opening does not depend on the data.  Prints one JSON line.
usage: python tools/kzg_bench.py [--logs 20,22] [--sizes 1,64,1024,4096,16384] [--reps 3]"""
import argparse
import ctypes as C
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from noir_backend_using_gnark_amd import _lib, kzg  # noqa: E402
from oracle import bn254_ref as ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import plonk_ref as pl  # noqa: E402

HOST_CAP = 128
ALPHA = 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % ref.R
M = pl.ints_to_mont_np


def best_ms(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def random_poly_dev(n, seed):
    b = _lib.DeviceBuffer(n * 32)
    _lib.check(_lib.lib().zk_bn254_fr_random_dev(C.c_void_p(b.ptr), C.c_size_t(n), C.c_uint64(seed), C.c_int(1), C.c_int(0), None))
    _lib.check(_lib.lib().zk_dev_sync())
    return b


def true_opening():
    rng = random.Random(5)
    srs = pl.kzg_new_srs(64, ALPHA, fast=True)
    g1 = np.ascontiguousarray(srs["g1"])
    p, z = [rng.randrange(ref.R) for _ in range(33)], rng.randrange(ref.R)
    v = pl.poly_eval(p, z)
    q = pl.divide_by_x_minus_a(p, v, z)
    g2 = np.stack([np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64) for P in srs["g2"]])
    return orc.g1_msm(g1[:33], M(p)), orc.g1_msm(g1[:32], M(q)), M([v])[0], M([z])[0], g2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="20,22")
    ap.add_argument("--sizes", default="1,64,1024,4096,16384")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    _lib.require_device()
    out = {"open": {}, "verify_batch": {"batch": {}, "fallback": {}, "host_1t": {}, "host_16t": {}}}
    logs = [int(x) for x in a.logs.split(",") if x]
    if logs:
        nmax = 1 << max(logs)
        srs = kzg.new_srs(nmax, M([ALPHA])[0])
        polys = [random_poly_dev(nmax, 40 + k) for k in range(7)]
        pts = M([0x1234567 + 977 * k for k in range(7)])
        for lg in logs:
            n = 1 << lg
            srs.commit(polys[0], n)
            srs.open(polys[0], pts[0], n)  # warm-up: arenas, streams
            r = {"commit_ms": round(best_ms(lambda: srs.commit(polys[0], n), a.reps), 3),
                 "open_ms": round(best_ms(lambda: srs.open(polys[0], pts[0], n), a.reps), 3)}
            r["open_over_commit"] = round(r["open_ms"] / r["commit_ms"], 3)
            for cnt in (2, 3):
                srs.open_many(polys[:cnt], pts[:cnt], [n] * cnt)
                r["open_many_%d_ms" % cnt] = round(best_ms(lambda: srs.open_many(polys[:cnt], pts[:cnt], [n] * cnt), a.reps), 3)
                r["open_x%d_ms" % cnt] = round(best_ms(lambda: [srs.open(polys[k], pts[k], n) for k in range(cnt)], a.reps), 3)
            digests = np.zeros((7, 8), np.uint64)  # (the digests only enter the folding challenge)
            srs.batch_open_single_point(polys, digests, pts[0], [n] * 7)
            r["batch_open_7_ms"] = round(best_ms(lambda: srs.batch_open_single_point(polys, digests, pts[0], [n] * 7), a.reps), 3)
            out["open"]["2^%d" % lg] = r
        for b in polys:
            b.free()
        srs.free()
    d, h, v, z, g2 = true_opening()
    assert kzg.verify(d, h, v, z, g2)
    vb = out["verify_batch"]
    for n in [int(x) for x in a.sizes.split(",") if x]:
        D, H, V, Z = (np.ascontiguousarray(np.tile(x, (n, 1))) for x in (d, h, v, z))
        assert kzg.batch_verify_multi_points(D, H, V, Z, g2).all()
        ms = best_ms(lambda: kzg.batch_verify_multi_points(D, H, V, Z, g2), a.reps)
        vb["batch"][n] = {"ms": round(ms, 3), "openings_per_s": round(n / ms * 1e3, 1)}
        Vb = V.copy()
        Vb[n // 2] = M([7])[0]
        assert (1 - kzg.batch_verify_multi_points(D, H, Vb, Z, g2)).sum() == 1
        ms = best_ms(lambda: kzg.batch_verify_multi_points(D, H, Vb, Z, g2), a.reps)
        vb["fallback"][n] = {"ms": round(ms, 3), "openings_per_s": round(n / ms * 1e3, 1)}
        m = min(n, HOST_CAP)
        ms1 = best_ms(lambda: [kzg.verify(d, h, v, z, g2) for _ in range(m)], 1)
        vb["host_1t"][n] = {"ms_per_opening": round(ms1 / m, 3), "openings_per_s": round(m / ms1 * 1e3, 1)}
        with ThreadPoolExecutor(16) as ex:
            ms16 = best_ms(lambda: list(ex.map(lambda i: kzg.verify(d, h, v, z, g2), range(m))), 1)
        vb["host_16t"][n] = {"ms_per_opening": round(ms16 / m, 3), "openings_per_s": round(m / ms16 * 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
