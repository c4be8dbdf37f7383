"""Batch PLONK proving against the loop it replaces: for every (log_n, rows) the wall ms and proofs/s of ONE plonk.prove_batch call and of the loop of
plonk.prove over the same rows, on one key.  The solutions are resident in HBM (one satisfying solution of a random circuit that fills its domain, tiled: the
work does not depend on the rows being different; every row has blinders of its own, so every proof differs); the key is Setup's, on valid random bases with
a window table of the planner's width at every size.  The bytes of batch and loop are compared before anything is timed; every timing is the best of --reps windows after one untimed run.
Prints one JSON line and writes it to --out.
usage: python tools/plonk_batch_bench.py [--shapes 10:256,12:64,16:16] [--reps 5] [--out profiles/plonk_prove_batch.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from noir_backend_using_gnark_amd import _lib  # noqa: E402
from noir_backend_using_gnark_amd import bn254 as zb  # noqa: E402
from noir_backend_using_gnark_amd import plonk as zp  # noqa: E402
from oracle import bn254_ref as ref  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from oracle import plonk_ref as pl  # noqa: E402
from tests import plonk_shapes as ps  # noqa: E402

M = pl.ints_to_mont_np


def best_ms(fn, reps):
    fn()  # untimed: arenas, plans, streams
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10:256,12:64,16:16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plonk_prove_batch.json"))
    a = ap.parse_args()
    _lib.require_device()
    out = {"reps": a.reps, "entries": ["zk_bn254_plonk_prove_batch", "zk_bn254_plonk_prove"], "shapes": []}
    for shape in a.shapes.split(","):
        log_n, rows = (int(x) for x in shape.split(":"))
        n = 1 << log_n
        spr, sol = ps.circuit("random", n, 3, "full", 0xBE0 + log_n)
        g = spr.constraints
        col = lambda k: M([c[k] for c in g])  # noqa: E731
        # below 4,096 bases no window table is built by default and the commitments would run row after row: the planner's width is asked for, for both sides
        c, digits = C.c_uint32(0), C.c_uint32(0)
        _lib.check(_lib.lib().zk_bn254_msm_plan_info(C.c_size_t(n + 3), C.c_int(1), C.byref(c), C.byref(digits)))
        rb = zb.ResidentBases(orc.g1_gen_points(0x9E0, n + 3), table_window_bits=int(c.value))
        pk = zp.setup(zp.Circuit(spr.n_public, spr.n_vars, col(0), col(1), col(2), col(3), col(4), [c[5] for c in g], [c[6] for c in g], [c[7] for c in g]), rb)
        dev = _lib.DeviceBuffer.from_numpy(np.tile(M(sol), (rows, 1, 1)))
        bl = np.stack([M(ref.rand_felts(0xB11D + v, 9)) for v in range(rows)])
        one = _lib.DeviceBuffer.from_numpy(M(sol))
        batch = lambda: zp.prove_batch(pk, dev, bl, on_device=True)  # noqa: E731
        loop = lambda: [zp.prove(pk, one, bl[v]) for v in range(rows)]  # noqa: E731
        assert batch() == loop(), shape
        info = zp.prove_batch_info(pk)
        row = {"log_n": log_n, "rows": rows, "table_window_bits": int(c.value), **info}
        for name, fn in (("batch", batch), ("loop", loop)):
            ms = best_ms(fn, a.reps)
            row[name] = {"ms": round(ms, 3), "proofs_per_s": round(rows / ms * 1e3, 1)}
        row["batch_over_loop"] = round(row["batch"]["proofs_per_s"] / row["loop"]["proofs_per_s"], 3)
        out["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        dev.free()
        one.free()
        pk.free()
        rb.free()
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
