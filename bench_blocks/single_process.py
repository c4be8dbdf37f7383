"""bench.py --gpus N --single-process: N device entries in ONE process behind the unchanged C ABI (csrc/multidev.hip)."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

from .common import *  # noqa: F401,F403
from .common import ROOT, N_PUBLIC, HBM_PEAK_GBS, R_FR, seed_at, dump_outputs


def single_process_main(args, zk, lib):
    """bench.py --gpus N --single-process: the multi-GPU path a caller of the C ABI gets WITHOUT becoming one process per GPU (the reference is one process:
    gnark_backend_ffi/main.go:24-37) -- zk_init_devices + a proving key with device_mask, then the ordinary zk_bn254_groth16_prove."""
    L = lib.lib()
    N = args.gpus
    real = max(1, int(L.zk_device_count()))
    devs = [i % real for i in range(N)]
    lib.check(L.zk_init_devices((C.c_int * N)(*devs), C.c_size_t(N)))
    lib.check(L.zk_set_default_devices(C.c_uint32(0)))
    log_n = args.log_n if args.log_n is not None else 20
    witness = 1 if args.scalars == "witness" else 0
    t0 = time.time()
    inst = Instance(L, lib, zk, log_n, 0, N_PUBLIC, witness, not args.no_tables)
    # --full: the single-entry proof the multi-device one is compared with
    single = zk.prove(inst.pk, inst.d_a, inst.d_b, inst.d_c, inst.d_w, inst.r, inst.s, n_constraints=inst.N, on_device=True) if args.full else None
    inst.pk.free()
    pk = zk.ProvingKey(log_n, inst.N, N_PUBLIC, inst.small["alpha"], inst.small["beta"], inst.small["delta"], inst.g1_a, inst.g1_b, inst.g1_k.ptr + N_PUBLIC * 64, inst.g1_z,
                       inst.small2["beta"], inst.small2["delta"], inst.g2_b, bases_on_device=True, precompute_tables=not args.no_tables, device_mask=(1 << N) - 1)
    setup_s = time.time() - t0
    step = lambda: zk.prove(pk, inst.d_a, inst.d_b, inst.d_c, inst.d_w, inst.r, inst.s, n_constraints=inst.N, on_device=True)
    proof = None
    for _ in range(args.warmup):
        proof = step()
    lib.check(L.zk_dev_sync())
    t0 = time.perf_counter()
    for _ in range(args.steps):
        proof = step()
    lib.check(L.zk_dev_sync())
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, proof)
    metric = "Groth16 prove ms + BN254 G1 MSM scalar-muls/sec at 2^20 / 2^24 constraints"
    try:
        metric = json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    except Exception:
        pass
    out = {"metric": metric, "value": round(inst.g1_units() / (ms * 1e-3), 1), "unit": "G1 scalar-muls/s (whole prove: 4 G1 MSMs + G2 MSM + 7 NTTs per step)",
           "n_gpus": N, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms, 3), "prove_ms": round(ms, 3), "higher_is_better": True, "scaling": "strong",
           "vs_baseline": None, "dtype": "u32", "data": "synthetic",
           "config": {"workload": "groth16_prove_bn254_synthetic_r1cs_2^%d" % log_n, "constraints": inst.N, "wires": inst.N, "n_public": N_PUBLIC, "scalars": args.scalars,
                      "parallelism": "ONE process, %d device entries behind zk_bn254_groth16_prove (composite key by wire range, block-sharded computeH, peer-copy "
                                     "transposes, 768-byte records combined on the host)" % N,
                      "devices": devs, "real_gpus": real, "virtual_entries": real < N},
           "proof_equals_single_entry": bool(proof == single) if args.full else None, "proof_sha": hashlib.sha256(proof).hexdigest()[:16], "setup_s": round(setup_s, 2),
           "roofline": None, "cpu_baseline": None,
           "note": "virtual entries share one GPU: this line shows that the path runs and gives the single-GPU bytes, not how it scales" if real < N else None}
    if args.full and proof != single:
        out["parity_error"] = "the proof over %d device entries differs from the single-entry proof" % N
    pk.free()
    print(json.dumps(out))
