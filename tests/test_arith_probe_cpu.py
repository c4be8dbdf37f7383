"""CPU suite: the test-only probe library (csrc/probe.hip -> libzkmi_probe.so) is built beside libzkmi.so without leaking into it, and every
vector tests/arith_edges.py generates for tests/test_gpu_arith_edges.py satisfies the precondition of the function it is fed to -- so a device
mismatch there always points at the kernel, never at the generator."""
import os
import random
import subprocess

import pytest

from tests import arith_edges as E

PKG = os.path.join(E.ROOT, "noir_backend_using_gnark_amd")
M, MR, P, R = E.M, E.MR, E.P, E.R


def _defined(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, lib)], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_probe_library_is_built_and_separate():
    syms = _defined("libzkmi_probe.so")
    assert {"zk_probe", "zk_probe_op", "zk_probe_shape"} <= syms
    assert not any(s.startswith("zk_probe") for s in _defined("libzkmi.so"))
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    srcs = [ln for ln in mk.splitlines() if ln.startswith("SRCS :=")][0]
    assert "probe.hip" not in srcs


def test_probe_op_table():
    from tests import probe
    names = ["FP_MUL", "FR_FROM_MONT", "F12_FROB2", "G2_SCALAR_MUL", "U29_MUL4", "U29_NEG80", "U29R_PACK1", "ACC29_MADD_CHAIN", "SHA256"]
    for n in names:
        op, iw, ow = probe.shape(n)
        assert op >= 0 and iw > 0 and ow > 0
    with pytest.raises(KeyError):
        probe.shape("NO_SUCH_OP")


def test_u29_generators_meet_preconditions():
    rng = random.Random(7)
    vin, exp, pre = E.u29_mul_vectors(rng, 2048)
    for a, b in pre:
        assert E.is_weak(a, E.TAIL_BOUND) and E.is_weak(b, E.TAIL_BOUND)
        assert max(a) < 1 << 31                                   # u29_sqr: limbs < 2^31
        assert E.mul_pre(a, b)
    assert E.weak_max(E.TAIL_BOUND) in [a for a, _ in pre]
    for N in (2, 3, 4):
        _, _, pre = E.mulN_vectors(random.Random(8 + N), 512, N, E.TAIL_BOUND)
        for ops in pre:
            assert E.mul_pre(*ops) and all(E.is_weak(o, E.TAIL_BOUND) for o in ops)
    for K in E.FP_KS:
        _, _, pre = E.sub_vectors(random.Random(100 + K), 2048, K)
        for a, b in pre:
            assert E.sub_pre(a, b, K), K
        # the largest subtrahend is within one top-limb unit of K p
        assert K * P - E.val(pre[0][1]) < 1 << 233
    for K in E.FR_KS:
        for b in E.dominated(random.Random(K), MR.bias_limbs(K), 512):
            assert E.sub_pre([0] * 9, b, K, MR)


def test_lazy_edges_follow_the_model():
    b = E.G1_MADD_BOUNDS
    assert 13 * P < b[0] < 14 * P and all(x <= 2 * P + 1 for x in b[1:])
    assert all(x <= 2.3 * P for x in E.G2_MADD_BOUNDS)
    rng = random.Random(3)
    for _ in range(200):
        x = rng.randrange(P)
        for bound in (b[0], 2 * P, E.TAIL_BOUND):
            l = E.lazy29(x, bound, rng)
            assert E.is_weak(l, bound) and E.from29(l) == x
        l = E.lazy29(x, E.TAIL_BOUND)
        assert E.val(l) >= E.TAIL_BOUND - P                        # at the class bound
    for x in E.store_inputs(random.Random(10), 4096):
        assert E.is_weak(x, E.STORE_MAX + 1) and E.mul_pre(x, [0] * 8 + [1 << 24])
    vals = E.lazy_vals(E.STORE_MAX + 1)
    assert max(vals) == E.STORE_MAX and all(k * P in vals for k in range(1, 32))


def test_zero_filter_edges_are_product_outputs():
    # a direct product output has limbs 0..7 < 2^29 and the value bound of its filter: multiples of p are normalised limbs
    for k in range(16):
        l = E.limbs(k * P)
        assert all(v <= M.MASK for v in l[:8]) and E.val(l) == k * P
    # the model's exact product reaches p itself (x * 2^261 for x == p)
    assert E.val(M.mul_exact(E.limbs(P), list(M.limbs((1 << 2 * M.RBITS) % P)))) % P == 0


def test_tower_helpers():
    rng = random.Random(4)
    a = E.rand_f12(rng)
    g = E.cyclotomic(a)
    assert E.f12_mul(g, E.f12_conj(g)) == E.F12_1                 # cyclotomic: the conjugate is the inverse
    assert E.f12_inv(a) and E.f12_mul(a, E.f12_inv(a)) == E.F12_1


def test_sha_generator_against_hashlib():
    import hashlib
    recs, exp, lab = E.sha_vectors()
    assert len({r[1] for r in recs if r[0] == 0}) == 301
    data = bytes(range(256)) * 2
    for cut in (64, 128, 192):
        mid = E.sha256_midstate(data[:cut])
        assert len(mid) == 8 and mid != E.SHA_IV
    assert E.sha_words(hashlib.sha256(b"").digest())[0] == 0xe3b0c442
