"""The public KZG entries at K = 9 coefficients per lane (csrc/scan.hpp scan_plan: K = max(8, ceil(len / 2^18)), so 2^21 + 3 coefficients give K = 9 and 911
workgroups): zk_bn254_kzg_open fixes the K of the call's longest polynomial for every row, so the short rows next to the long one are scanned under a K that is
not their own (2304 coefficients are one workgroup exactly; 9 are one lane); zk_bn254_kzg_batch_open_single_point evaluates every row with the long row's nb and
divides the fold at K = 9.  tests/test_gpu_kzg.py stops at 2^16 + 8 coefficients: K = 8 everywhere.

The SRS secret is known (ALPHA), so an expected opening needs no multi-exponentiation: Commit(q) = [q(ALPHA)] G1 and q(ALPHA) = (f(ALPHA) - f(z)) / (ALPHA - z) --
two Horner evaluations in Python integers and one scalar multiplication with the reference curve code (oracle/bn254_ref.py), compared as bytes.

A sibling of tests/test_gpu_kzg.py rather than a part of it: the fixture holds an SRS of 2^21 + 3 points and a polynomial of that length, which go when this module
is done.  The long polynomial is drawn as its Montgomery image (random limbs below 2^252 < r): the canonical coefficients are those times 2^-256, which the Horner
evaluation applies once at the end instead of two million times."""
import random
import time

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import hscan_ref as hr
from tests.plonk_shapes import scan_plan

pytestmark = pytest.mark.gpu

R = ref.R
M = pl.ints_to_mont_np
ALPHA = 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % R  # the SRS secret of tests/test_gpu_kzg.py
BIG = (1 << 21) + 3
SHORT = (1, 2, 9, 10, 2303, 2304, 2305)  # under K = 9: a constant, less than a lane, one lane, a tail lane of one, and 2304 = 256 * 9: one workgroup exactly
RINV = pow(1 << 256, -1, R)


def g1_img(P):
    return np.frombuffer(ref.g1_affine_mont_bytes(P), dtype=np.uint64).copy()


def horner(coeffs, z):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * z + c) % R
    return acc


class Poly:
    """coefficients as the device takes them (`image`) and a way to evaluate them on the host"""

    def __init__(self, image, words, scale):
        self.image, self.words, self.scale, self.n = image, words, scale, image.shape[0]
        self.at_alpha = self(ALPHA)

    @classmethod
    def of(cls, coeffs):
        return cls(M(coeffs), list(coeffs), 1)

    @classmethod
    def random_image(cls, seed, n):
        limbs = np.frombuffer(random.Random(seed).randbytes(32 * n), dtype=np.uint64).reshape(n, 4).copy()
        limbs[:, 3] &= np.uint64((1 << 60) - 1)  # below 2^252 < r
        raw = limbs.tobytes()
        return cls(limbs, [int.from_bytes(raw[i:i + 32], "little") for i in range(0, 32 * n, 32)], RINV)

    def __call__(self, z):
        return horner(self.words, z) * self.scale % R


def opening(value_at_alpha, value_at_z, z):
    """[(f(ALPHA) - f(z)) / (ALPHA - z)] G1 as the device returns a point"""
    k = (value_at_alpha - value_at_z) * pow(ALPHA - z, -1, R) % R
    return g1_img(ref.g1_mul(ref.G1_GEN, k) if k else None)


@pytest.fixture(scope="module")
def env():
    assert scan_plan(BIG) == (9, 911) and hr.scan_blocks(2304, 9) == 1 and hr.scan_blocks(2305, 9) == 2
    t0 = time.perf_counter()
    srs = kzg.new_srs(BIG, M([ALPHA])[0])  # the planner's default: window tables
    t1 = time.perf_counter()
    big = Poly.random_image(99, BIG)
    rng = random.Random(98)
    short = {n: Poly.of([rng.randrange(R) for _ in range(n)]) for n in SHORT}
    print("fixture: SRS of %d points %.2f s, polynomials %.2f s" % (BIG, t1 - t0, time.perf_counter() - t1))
    yield dict(srs=srs, big=big, short=short)
    srs.free()


def check_open_many(env, polys, on_device):
    rng = random.Random(17 * len(polys) + on_device)
    zs = [rng.randrange(R) for _ in polys]
    bufs = [_lib.DeviceBuffer.from_numpy(p.image) for p in polys] if on_device else None
    h, v = env["srs"].open_many(bufs if on_device else [p.image for p in polys], M(zs), [p.n for p in polys] if on_device else None)
    for k, (p, z) in enumerate(zip(polys, zs)):
        at_z = p(z)
        assert v[k].tobytes() == M([at_z])[0].tobytes(), "row %d (%d coefficients): claimed value" % (k, p.n)
        assert h[k].tobytes() == opening(p.at_alpha, at_z, z).tobytes(), "row %d (%d coefficients): H" % (k, p.n)
        if p.n == 1:
            assert not h[k].any()
    for b, p in zip(bufs or [], polys):  # the caller's buffers are not written
        assert b.to_numpy(np.uint64, p.image.shape).tobytes() == p.image.tobytes(), "device polynomial of %d coefficients was written" % p.n
        b.free()


@pytest.mark.parametrize("on_device", [False, True])
def test_open_many_short_rows_under_the_long_rows_k(env, on_device):
    """eight rows in one chunk: every one of them scanned with K = 9 and nb = 911"""
    check_open_many(env, [env["big"]] + [env["short"][n] for n in SHORT], on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_open_many_long_row_alone_in_the_second_chunk(env, on_device):
    """nine rows: the first chunk of eight runs K = 9 -- the call's -- at the small nb of its own longest row (2305 coefficients: two workgroups)"""
    first = [env["short"][n] for n in SHORT] + [env["short"][9]]
    check_open_many(env, first + [env["big"]], on_device)


@pytest.mark.parametrize("root", [False, True])
def test_batch_open_single_point_at_k9(env, root):
    """the evaluation scan over the long row and four short ones with the long row's nb for every row, then the division of their fold at K = 9; the point random,
    or a root of the 2304-coefficient row.  Fold and gamma as tests/test_gpu_kzg.py's check_batch has them; H from the fold's two values."""
    rng = random.Random(500 + root)
    z = rng.randrange(R)
    polys = [env["short"][10], env["big"], env["short"][2304], env["short"][2], env["short"][2305]]
    if root:
        polys[2] = Poly.of(hr.poly_with_root(rng, 2304, z))
    claimed = [p(z) for p in polys]
    assert (claimed[2] == 0) == root
    digests = [ref.g1_mul(ref.G1_GEN, p.at_alpha) for p in polys]
    gamma = pl.kzg_derive_gamma(z, digests, claimed)
    fold_alpha, fold_z, acc = 0, 0, 1
    for p, c in zip(polys, claimed):
        fold_alpha, fold_z, acc = (fold_alpha + p.at_alpha * acc) % R, (fold_z + c * acc) % R, acc * gamma % R
    want_h = opening(fold_alpha, fold_z, z)
    dg = np.stack([g1_img(d) for d in digests])
    for on_device in (False, True):
        bufs = [_lib.DeviceBuffer.from_numpy(p.image) for p in polys] if on_device else None
        h, v = env["srs"].batch_open_single_point(bufs if on_device else [p.image for p in polys], dg, M([z])[0], [p.n for p in polys] if on_device else None)
        assert v.tobytes() == M(claimed).tobytes(), "claimed values (on_device = %s)" % on_device
        assert h.tobytes() == want_h.tobytes(), "H (on_device = %s)" % on_device
        for b, p in zip(bufs or [], polys):
            assert b.to_numpy(np.uint64, p.image.shape).tobytes() == p.image.tobytes()
            b.free()
