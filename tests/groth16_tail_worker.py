"""Worker of tests/test_gpu_groth16_tail.py (a subprocess: zk_init_devices changes process-wide state).  The same device is listed 8 times (virtual device
entries, as tests/multidev_worker.py does), a key is loaded over two of them -- a composite handle -- and the batched finalize is asked of it: the host form
goes row by row through the composite key's own combine step and writes the single-entry bytes, the _dev form refuses the handle.  Prints one JSON object."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import noir_backend_using_gnark_amd as zk  # noqa: E402
from noir_backend_using_gnark_amd import _lib, groth16 as g16, parallel  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from tests import groth16_tail_cases as tc  # noqa: E402

L = _lib.lib()


def main():
    devs = [0] * 8
    _lib.check(L.zk_init_devices((C.c_int * 8)(*devs), C.c_size_t(8)))
    _lib.check(L.zk_set_default_devices(C.c_uint32(0)))
    log_n = 12
    N = 1 << log_n
    g1, g2 = orc.g1_gen_points, orc.g2_gen_points
    pkd = dict(log_domain=log_n, n_wires=N, n_public=3, g1_alpha=g1(1, 1)[0], g1_beta=g1(2, 1)[0], g1_delta=g1(3, 1)[0], g1_a=g1(4, N), g1_b=g1(5, N),
               g1_k=g1(6, N - 3), g1_z=g1(7, N), g2_beta=g2(8, 1)[0], g2_delta=g2(9, 1)[0], g2_b=g2(10, N))
    single = zk.ProvingKey(**pkd)
    comp = zk.ProvingKey(**pkd, device_mask=0b11)
    n, n_partials = 5, 2
    parts, r, s = tc.bulk_rows(n, n_partials, 0xC0)
    want = [parallel.groth16_finalize(single, parts[i], r[i], s[i]) for i in range(n)]
    out = {"composite_handle": (comp.handle.value >> 56) == 0xff}
    out["host_form_on_composite"] = g16.finalize_batch(comp, parts, r, s) == want
    out["host_form_on_single"] = g16.finalize_batch(single, parts, r, s) == want
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (parts, r, s)]
    d_out = _lib.DeviceBuffer(128 * n)
    rc = L.zk_bn254_groth16_finalize_batch_dev(comp.handle, C.c_void_p(dev[0].ptr), C.c_size_t(n_partials), C.c_void_p(dev[1].ptr), C.c_void_p(dev[2].ptr),
                                               C.c_size_t(n), C.c_void_p(d_out.ptr), None)
    out["dev_form_refuses_composite"] = rc == _lib.ZK_ERR_ARG
    comp.free()
    single.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
