"""The verifying batch entries of the export path against what they replace: for every shape the wall ms and proofs/s of
  batch      ONE zk_plonk_verify_batch_with_vk (zk_groth16_verify_batch_with_vk) call over N proof texts and N values texts;
  loop       the single sequence over the same texts, row by row: hex-decode the proof, take the public values (PLONK: the felts at zk_acir_public_witnesses'
             positions, converted to Montgomery form; Groth16: zk_groth16_public_inputs), zk_bn254_plonk_verify / zk_bn254_groth16_verify on the host;
  host_rows  verify.plonk_verify_batch / verify.groth16_verify_batch on proof bytes and public inputs decoded beforehand -- the device verifier alone, so that
             batch - host_rows is what the texts cost: their upload, both decoders and the rows' digests (`text_share` of the batch call).
The proofs come from the prove-batch entries (four satisfying assignments of one synthetic circuit, tiled; every row has randomness of its own, so every proof
differs).  All three must accept every row before anything is timed.  batch and host_rows: the best of --reps windows after one untimed run; the loop, at about
10 ms per proof, is timed once (after one untimed pass over its first 32 rows).  Prints one JSON line and writes it to --out.
usage: python tools/export_verify_bench.py [--plonk 10:256,10:4096] [--groth16 10:256,10:4096] [--reps 5] [--out profiles/export_verify_batch.json]"""
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
from noir_backend_using_gnark_amd import verify as zv  # noqa: E402
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


def measure(row, rows, batch, loop_row, host_rows, reps):
    acc, status = batch()
    assert status == [0] * rows and all(acc), row
    assert all(host_rows()), row
    assert all(loop_row(v) for v in range(min(rows, 32))), row
    for name, fn in (("batch", batch), ("host_rows", host_rows)):
        ms = best_ms(fn, reps)
        row[name] = {"ms": round(ms, 3), "proofs_per_s": round(rows / ms * 1e3, 1)}
    t0 = time.perf_counter()
    ok = [loop_row(v) for v in range(rows)]
    ms = (time.perf_counter() - t0) * 1e3
    assert all(ok), row
    row["loop"] = {"ms": round(ms, 3), "proofs_per_s": round(rows / ms * 1e3, 1)}
    row["batch_over_loop"] = round(row["batch"]["proofs_per_s"] / row["loop"]["proofs_per_s"], 2)
    row["text_share"] = round(max(0.0, 1.0 - row["host_rows"]["ms"] / row["batch"]["ms"]), 4)
    _lib.profile(True)
    _lib.profile_reset()
    t0 = time.perf_counter()
    batch()
    wall = (time.perf_counter() - t0) * 1e3
    _, host = _lib.split_profile(_lib.profile_read())
    _lib.profile(False)
    row["profiled_call"] = {"ms": round(wall, 3), "sections_ms": {k[len("export."):]: round(v[1], 3) for k, v in host.items() if k.startswith("export.")}}
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def plonk_shape(log_n, rows, reps):
    n = 1 << log_n
    firsts = [None] + [(0x1111 * k, 0x2222 * k + 1) for k in range(1, DISTINCT)]
    acir, _ = sa.synth(n - 3, 3)
    acir = acir.encode()
    values = [sa.synth(n - 3, 3, first=f)[1] for f in firsts]
    texts = [sa.felts_wire_hex(values[v % DISTINCT]).encode() for v in range(rows)]
    c, digits = C.c_uint32(0), C.c_uint32(0)
    _lib.check(_lib.lib().zk_bn254_msm_plan_info(C.c_size_t(n + 3), C.c_int(1), C.byref(c), C.byref(digits)))
    srs = kzg.new_srs(n + 3, M([0x5EED0 + log_n])[0], table_window_bits=int(c.value))
    _, vk_hex, h = fe.plonk_preprocess(acir, texts[0], srs, keep_resident=True)
    bl = np.stack([M(ref.rand_felts(0xB11D + v, 9)) for v in range(rows)])
    proofs, status = fe.plonk_prove_batch_with_pk(acir, texts, None, srs, blinders=bl, pk_handle=h)
    assert status == [0] * rows
    _lib.check(_lib.lib().zk_bn254_plonk_pk_free(C.c_uint64(h)))
    proofs = [p.encode() for p in proofs]
    where, n_public = np.zeros(16, np.uint32), C.c_size_t(0)
    _lib.check(_lib.lib().zk_acir_public_witnesses(C.c_char_p(acir), C.c_size_t(len(acir)), C.c_size_t(len(values[0])), C.c_int(0), _lib.vp(where), C.c_size_t(16),
                                                   C.byref(n_public)))
    where = [int(x) for x in where[:n_public.value]]
    g2 = srs.g2

    def public_of(text):
        return M([int(text[8 + 64 * k:8 + 64 * (k + 1)], 16) for k in where]).reshape(len(where), 4)

    def batch():
        acc, st = fe.plonk_verify_batch_with_vk(acir, proofs, texts, vk_hex, g2)
        return list(acc), st

    loop_row = lambda v: zv.plonk_verify(bytes.fromhex(proofs[v].decode()), vk_hex, g2, public_of(texts[v]))  # noqa: E731
    blob = [bytes.fromhex(p.decode()) for p in proofs]
    pubs = np.stack([public_of(t) for t in texts])
    host_rows = lambda: zv.plonk_verify_batch(blob, vk_hex, g2, pubs)  # noqa: E731
    row = measure({"system": "plonk", "log_n": log_n, "rows": rows, "n_public": len(where), "values_text_bytes": len(texts[0])}, rows, batch, loop_row, host_rows, reps)
    srs.free()
    fe.export_cache_clear()
    return row


def groth16_shape(log_c, rows, reps):
    gates = (1 << log_c) // 2  # two constraints per gate
    firsts = [None] + [(0x1111 * k, 0x2222 * k + 1) for k in range(1, DISTINCT)]
    raw, _ = sr.synth(gates, 3)
    values = [sr.synth(gates, 3, first=f)[1] for f in firsts]
    texts = [sa.felts_wire_hex(values[v % DISTINCT]).encode() for v in range(rows)]
    raws = [sr.with_values(raw, w).encode() for w in values]
    raw = raw.encode()
    _, vk_hex, h = fe.groth16_preprocess(raw, M(ref.rand_felts(0xE2, 5)), keep_resident=True)
    built = C.c_int(0)
    _lib.check(_lib.lib().zk_bn254_groth16_pk_build_tables(C.c_uint64(h), C.c_int(0), C.byref(built)))
    rs = np.stack([M(ref.rand_felts(0xE100 + v, 2)) for v in range(rows)])
    proofs, status = fe.groth16_prove_batch_with_pk(raw, texts, None, rs, pk_handle=h)
    assert status == [0] * rows
    _lib.check(_lib.lib().zk_bn254_groth16_pk_free(C.c_uint64(h)))
    proofs = [p.encode() for p in proofs]

    def batch():
        acc, st = fe.groth16_verify_batch_with_vk(raw, proofs, texts, vk_hex)
        return list(acc), st

    loop_row = lambda v: zv.groth16_verify(bytes.fromhex(proofs[v].decode()), vk_hex, fe.groth16_public_inputs(raws[v % DISTINCT]))  # noqa: E731
    blob = [bytes.fromhex(p.decode()) for p in proofs]
    pubs = np.stack([fe.groth16_public_inputs(raws[v % DISTINCT]) for v in range(rows)])
    host_rows = lambda: zv.groth16_verify_batch(blob, vk_hex, pubs)  # noqa: E731
    row = measure({"system": "groth16", "log_constraints": log_c, "rows": rows, "n_public": int(pubs.shape[1]), "values_text_bytes": len(texts[0])}, rows, batch, loop_row,
                  host_rows, reps)
    fe.export_cache_clear()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plonk", default="10:256,10:4096")
    ap.add_argument("--groth16", default="10:256,10:4096")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "export_verify_batch.json"))
    a = ap.parse_args()
    _lib.require_device()
    out = {"reps": a.reps, "entries": ["zk_plonk_verify_batch_with_vk", "zk_bn254_plonk_verify", "zk_bn254_plonk_verify_batch", "zk_groth16_verify_batch_with_vk",
                                       "zk_bn254_groth16_verify", "zk_bn254_groth16_verify_batch"], "shapes": []}
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
