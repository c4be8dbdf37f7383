"""Batch Groth16 proving against the loop it replaces: for every (log_n, n_proofs) the wall ms and proofs/s of zk_bn254_groth16_prove_batch, of a loop of
n_proofs zk_bn254_groth16_prove calls on the same key and inputs, and of that loop on 16 Python threads (ctypes releases the GIL).  Inputs are resident in
HBM (a, b, c uniform, w witness-like, n_constraints = N); the key is a random valid one with its window tables.  Every timing is the best of --reps runs
after one untimed run; the batch's bytes are checked against the loop's before anything is timed.  Prints one JSON line.
usage: python tools/groth16_batch_bench.py [--log-n 10,12,14,16] [--n-proofs 1,16,64,256] [--reps 3]"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import noir_backend_using_gnark_amd as zk  # noqa: E402
from noir_backend_using_gnark_amd import _lib  # noqa: E402
from noir_backend_using_gnark_amd import groth16 as g16  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def best_ms(fn, reps):
    fn()  # untimed: arenas, plans, streams
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def key(log_n):
    N = 1 << log_n
    nw, npub = N - 3, 5
    g1, g2 = orc.g1_gen_points, orc.g2_gen_points
    return zk.ProvingKey(log_domain=log_n, n_wires=nw, n_public=npub, g1_alpha=g1(1, 1)[0], g1_beta=g1(2, 1)[0], g1_delta=g1(3, 1)[0], g1_a=g1(4, nw),
                         g1_b=g1(5, nw), g1_k=g1(6, nw - npub), g1_z=g1(7, N), g2_beta=g2(8, 1)[0], g2_delta=g2(9, 1)[0], g2_b=g2(10, nw))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="10,12,14,16")
    ap.add_argument("--n-proofs", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    sizes = [int(x) for x in a.n_proofs.split(",")]
    out = {"reps": a.reps, "shapes": []}
    for log_n in [int(x) for x in a.log_n.split(",")]:
        N = 1 << log_n
        pk = key(log_n)
        nw, nmax = pk.n_wires, max(sizes)
        pool = 8  # distinct rows, tiled: the work depends on the digits' distribution, not on the rows being different
        mats = [np.stack([orc.rand_fr(100 + 10 * k + i, N) for i in range(pool)])[np.arange(nmax) % pool] for k in range(3)]
        mats.append(np.stack([orc.rand_fr(200 + i, nw, witness_like=True) for i in range(pool)])[np.arange(nmax) % pool])
        dev = [_lib.DeviceBuffer.from_numpy(m) for m in mats]
        r, s = orc.rand_fr(300, nmax), orc.rand_fr(301, nmax)
        info = g16.batch_info(pk)

        def one(i):
            return zk.prove(pk, dev[0].ptr + i * N * 32, dev[1].ptr + i * N * 32, dev[2].ptr + i * N * 32, dev[3].ptr + i * nw * 32, r[i], s[i], n_constraints=N,
                            on_device=True)

        for n in sizes:
            batch = lambda: g16.prove_batch(pk, *dev, r[:n], s[:n], on_device=True, n_constraints=N)  # noqa: E731
            loop = lambda: [one(i) for i in range(n)]  # noqa: E731
            assert batch() == loop(), (log_n, n)
            row = {"log_n": log_n, "n_proofs": n, "batched_path": bool(info["batched"] and n >= 2), "chunk_rows": info["chunk_rows"]}
            for name, fn in (("batch", batch), ("loop", loop)):
                ms = best_ms(fn, a.reps)
                row[name] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
            with ThreadPoolExecutor(16) as ex:
                ms = best_ms(lambda: list(ex.map(one, range(n))), a.reps)
            row["loop_16_threads"] = {"ms": round(ms, 3), "proofs_per_s": round(n / ms * 1e3, 1)}
            row["batch_over_loop"] = round(row["batch"]["proofs_per_s"] / row["loop"]["proofs_per_s"], 3)
            out["shapes"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        for d in dev:
            d.free()
        pk.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
