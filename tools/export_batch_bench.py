"""The batch entries of the export path against the loops they replace: for every shape the wall ms and proofs/s of ONE zk_plonk_prove_batch_with_pk
(zk_groth16_prove_batch_with_pk) call and of the loop of warm zk_plonk_prove_with_pk (zk_groth16_prove_with_pk) calls over the same rows -- circuit text
resident, key by handle, pinned blinders / (r, s); PLONK on an SRS with a window table of the planner's width, Groth16 on a key with its window tables.  The
rows are satisfying assignments of one synthetic circuit (tools/synth_acir.py, tools/synth_raw_r1cs.py; four different ones, tiled: the work does not depend on
the rows being different, and every row has randomness of its own, so every proof differs).  The characters of batch and loop are compared before anything is
timed; every timing is the best of --reps windows after one untimed run.  `witness_share` is the part of one further, profiled batch call (zk_profile_*) spent
in upload + decode + assembly (the host section export.batch_witness_rows).  Prints one JSON line and writes it to --out.
usage: python tools/export_batch_bench.py [--plonk 10:256,12:64,16:16] [--groth16 10:256,16:16] [--reps 5] [--out profiles/export_batch.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from noir_backend_using_gnark_amd import _lib, kzg  # noqa: E402
from noir_backend_using_gnark_amd import frontend as fe  # noqa: E402
from oracle import bn254_ref as ref  # noqa: E402
from oracle import plonk_ref as pl  # noqa: E402
from tools import synth_acir as sa  # noqa: E402
from tools import synth_raw_r1cs as sr  # noqa: E402

M = pl.ints_to_mont_np
DISTINCT = 4


def best_ms(fn, reps):
    fn()  # untimed: arenas, plans, streams
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


def measure(row, rows, batch, loop, reps):
    got, status = batch()
    assert status == [0] * rows and got == loop(), row
    for name, fn in (("batch", batch), ("loop", loop)):
        ms = best_ms(fn, reps)
        row[name] = {"ms": round(ms, 3), "proofs_per_s": round(rows / ms * 1e3, 1)}
    row["batch_over_loop"] = round(row["batch"]["proofs_per_s"] / row["loop"]["proofs_per_s"], 3)
    _lib.profile(True)
    _lib.profile_reset()
    t0 = time.perf_counter()
    batch()
    wall = (time.perf_counter() - t0) * 1e3
    _, host = _lib.split_profile(_lib.profile_read())
    _lib.profile(False)
    sections = {k[len("export."):]: round(v[1], 3) for k, v in host.items() if k.startswith("export.")}
    row["profiled_call"] = {"ms": round(wall, 3), "sections_ms": sections, "witness_share": round(sections.get("batch_witness_rows", 0.0) / wall, 4)}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def plonk_shape(log_n, rows, reps):
    n = 1 << log_n
    firsts = [None] + [(0x1111 * k, 0x2222 * k + 1) for k in range(1, DISTINCT)]
    acir, _ = sa.synth(n - 3, 3)
    acir = acir.encode()
    texts = [sa.felts_wire_hex(sa.synth(n - 3, 3, first=f)[1]) for f in firsts]
    texts = [texts[v % DISTINCT].encode() for v in range(rows)]  # (as bytes: the mirrors then pass them on as they are)
    # below 4,096 bases no window table is built by default and the batch prover's commitments would run row after row: the planner's width is asked for
    c, digits = C.c_uint32(0), C.c_uint32(0)
    _lib.check(_lib.lib().zk_bn254_msm_plan_info(C.c_size_t(n + 3), C.c_int(1), C.byref(c), C.byref(digits)))
    srs = kzg.new_srs(n + 3, M([0x5EED0 + log_n])[0], table_window_bits=int(c.value))
    _, _, h = fe.plonk_preprocess(acir, texts[0], srs, keep_resident=True)
    bl = np.stack([M(ref.rand_felts(0xB11D + v, 9)) for v in range(rows)])
    batch = lambda: fe.plonk_prove_batch_with_pk(acir, texts, None, srs, blinders=bl, pk_handle=h)  # noqa: E731
    loop = lambda: [fe.plonk_prove_with_pk(acir, texts[v], None, srs, blinders=bl[v], pk_handle=h) for v in range(rows)]  # noqa: E731
    chunk, batched = C.c_size_t(0), C.c_int(0)
    _lib.check(_lib.lib().zk_bn254_plonk_prove_batch_info(C.c_uint64(h), C.byref(chunk), C.byref(batched), None))
    row = measure({"system": "plonk", "log_n": log_n, "rows": rows, "table_window_bits": int(c.value), "chunk_rows": int(chunk.value), "commits_batched": int(batched.value),
                   "values_text_bytes": len(texts[0])}, rows, batch, loop, reps)
    _lib.check(_lib.lib().zk_bn254_plonk_pk_free(C.c_uint64(h)))
    srs.free()
    fe.export_cache_clear()
    return row


def groth16_shape(log_c, rows, reps):
    gates = (1 << log_c) // 2  # two constraints per gate
    firsts = [None] + [(0x1111 * k, 0x2222 * k + 1) for k in range(1, DISTINCT)]
    raw, _ = sr.synth(gates, 3)
    values = [sr.synth(gates, 3, first=f)[1] for f in firsts]
    texts = [sa.felts_wire_hex(values[v % DISTINCT]).encode() for v in range(rows)]  # (as bytes: the mirrors then pass them on as they are)
    raws = [sr.with_values(raw, w).encode() for w in values]
    raw = raw.encode()
    _, _, h = fe.groth16_preprocess(raw, M(ref.rand_felts(0xE2, 5)), keep_resident=True)
    built = C.c_int(0)
    _lib.check(_lib.lib().zk_bn254_groth16_pk_build_tables(C.c_uint64(h), C.c_int(0), C.byref(built)))
    rs = np.stack([M(ref.rand_felts(0xE100 + v, 2)) for v in range(rows)])
    batch = lambda: fe.groth16_prove_batch_with_pk(raw, texts, None, rs, pk_handle=h)  # noqa: E731
    loop = lambda: [fe.groth16_prove_with_pk(raws[v % DISTINCT], None, rs[v], pk_handle=h) for v in range(rows)]  # noqa: E731
    chunk, batched = C.c_size_t(0), C.c_int(0)
    _lib.check(_lib.lib().zk_bn254_groth16_batch_info(C.c_uint64(h), C.byref(chunk), C.byref(batched)))
    row = measure({"system": "groth16", "log_constraints": log_c, "rows": rows, "chunk_rows": int(chunk.value), "batched": int(batched.value),
                   "values_text_bytes": len(texts[0])}, rows, batch, loop, reps)
    _lib.check(_lib.lib().zk_bn254_groth16_pk_free(C.c_uint64(h)))
    fe.export_cache_clear()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plonk", default="10:256,12:64,16:16")
    ap.add_argument("--groth16", default="10:256,16:16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_batch.json"))
    a = ap.parse_args()
    _lib.require_device()
    out = {"reps": a.reps, "entries": ["zk_plonk_prove_batch_with_pk", "zk_plonk_prove_with_pk", "zk_groth16_prove_batch_with_pk", "zk_groth16_prove_with_pk"], "shapes": []}
    for spec, fn in ((a.plonk, plonk_shape), (a.groth16, groth16_shape)):
        for shape in filter(None, spec.split(",")):
            log_n, rows = (int(x) for x in shape.split(":"))
            out["shapes"].append(fn(log_n, rows, a.reps))
    line = json.dumps(out)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
