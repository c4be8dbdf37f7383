"""Rows for the Groth16 proof tail (zk_bn254_groth16_finalize / _finalize_batch): five un-normalised MSM sums + (r, s) -> 128 proof bytes.  No GPU, no library:
python integers and oracle/bn254_ref.py only.

The key is tiny (log_n = 2) and its alpha, beta, delta, beta2, delta2 are KNOWN multiples of the generators, and so is every sum a row carries, so the
cancellations the tail's branches need can be constructed: a sum at infinity, A = -alpha, Bs or Ar or Krs at infinity, K = +-Z, r or s at 0 / 1 / r_mod - 1.
A row's expectation is computed with bn254_ref's affine arithmetic from gnark's own form

    Ar = A + alpha + r delta,  Bs1 = B1 + beta + s delta,  Bs = B2 + beta2 + s delta2,  Krs = K + Z + s Ar + r Bs1 - rs delta

which is NOT the arrangement the library uses (K + Z + s (A + alpha) + r (B1 + beta) + rs delta: library_arrangement below).  Pure-python scalar
multiplications are slow, so only the tagged rows and two random ones carry an expectation; bulk rows (bulk_rows) are made from a small pool of points and are
checked against the host tail by the GPU tests.

Records are XYZZ images of affine points, (x l^2, y l^3, l^2, l^3) with a random l != 1 (in Fp2 for G2): a kernel that assumes zz = 1 fails.  A point at
infinity is any record with zz = 0; some rows give it a non-zero x and y on purpose."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import bn254_ref as ref

Q, R = ref.Q, ref.R
LOG_N = 2
N_WIRES, N_PUBLIC = 3, 1
# discrete logarithms of the key's five elements
KEY_SCALARS = dict(alpha=0x1234567, beta=0x89ABCDE, delta=0xF00DF00D5, beta2=0x31415926, delta2=0x27182818)
KEY_SCALARS_OTHER_DELTA = dict(KEY_SCALARS, delta=0xBADC0FFEE, delta2=0x5EED5EED)


class Row(NamedTuple):
    partials: np.ndarray            # (n_partials, 96) uint64
    r: np.ndarray                   # (4,) uint64, Montgomery
    s: np.ndarray
    expected: Optional[bytes]       # gnark's form through bn254_ref, or None
    tag: str
    pre: dict                       # what the tag promises: the affine sums, r and s as integers, and `inf`: the names that must be the point at infinity


def _limbs(x: int) -> list:
    return [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def _fp(x: int) -> list:
    return _limbs(ref.to_mont(x % Q, Q))


def fr_mont(x: int) -> np.ndarray:
    return np.array(_limbs(ref.to_mont(x % R, R)), dtype=np.uint64)


class _Rng:
    def __init__(self, seed):
        self.sm = ref.SplitMix64(seed)

    def below(self, m):
        v = 0
        for _ in range(5):
            v = (v << 64) | self.sm.next()
        return v % m

    def lam(self):  # a projective factor that is neither 0 nor 1
        while True:
            v = self.below(Q)
            if v > 1:
                return v


def g1(k: int):
    return ref.g1_mul(ref.G1_GEN, k) if k % R else None


def g2(k: int):
    return ref.g2_mul(ref.G2_GEN, k) if k % R else None


def xyzz_g1(P, lam: int, junk=None) -> list:
    """16 limbs.  P None: zz = zzz = 0 and x, y = junk (default 0)"""
    if P is None:
        jx, jy = junk if junk else (0, 0)
        return _fp(jx) + _fp(jy) + [0] * 8
    l2 = lam * lam % Q
    l3 = l2 * lam % Q
    return _fp(P[0] * l2) + _fp(P[1] * l3) + _fp(l2) + _fp(l3)


def xyzz_g2(P, lam, junk=None) -> list:
    """32 limbs; lam in Fp2"""
    def f2(v):
        return _fp(v[0]) + _fp(v[1])
    if P is None:
        jx, jy = junk if junk else ((0, 0), (0, 0))
        return f2(jx) + f2(jy) + [0] * 16
    l2 = ref.f2_sqr(lam)
    l3 = ref.f2_mul(l2, lam)
    return f2(ref.f2_mul(P[0], l2)) + f2(ref.f2_mul(P[1], l3)) + f2(l2) + f2(l3)


def record(points, rng: _Rng, junk_inf=False) -> np.ndarray:
    """one 96-limb record from the affine points (A, B1, K, Z in G1, B2 in G2)"""
    A, B1, K, Z, B2 = points
    jg1 = (rng.below(Q) | 1, rng.below(Q) | 1) if junk_inf else None
    jg2 = ((rng.below(Q) | 1, rng.below(Q)), (rng.below(Q), rng.below(Q) | 1)) if junk_inf else None
    out = []
    for P in (A, B1, K, Z):
        out += xyzz_g1(P, rng.lam(), jg1)
    out += xyzz_g2(B2, (rng.lam(), rng.lam()), jg2)
    return np.array(out, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def key(which: str = "base"):
    """(pkd for zk.ProvingKey, the five key elements as affine bn254_ref points)"""
    from tests.helpers import g1_points_from_scalars, g2_points_from_scalars
    ks = KEY_SCALARS if which == "base" else KEY_SCALARS_OTHER_DELTA
    N = 1 << LOG_N
    pkd = dict(log_domain=LOG_N, n_wires=N_WIRES, n_public=N_PUBLIC,
               g1_alpha=g1_points_from_scalars([ks["alpha"]])[0], g1_beta=g1_points_from_scalars([ks["beta"]])[0],
               g1_delta=g1_points_from_scalars([ks["delta"]])[0], g1_a=g1_points_from_scalars([11, 12, 13]), g1_b=g1_points_from_scalars([21, 22, 23]),
               g1_k=g1_points_from_scalars([31, 32]), g1_z=g1_points_from_scalars([41, 42, 43, 44][:N]), g2_beta=g2_points_from_scalars([ks["beta2"]])[0],
               g2_delta=g2_points_from_scalars([ks["delta2"]])[0], g2_b=g2_points_from_scalars([51, 52, 53]))
    pts = dict(alpha=g1(ks["alpha"]), beta=g1(ks["beta"]), delta=g1(ks["delta"]), beta2=g2(ks["beta2"]), delta2=g2(ks["delta2"]))
    return pkd, pts


def gnark_form(pts, sums, r: int, s: int):
    """(Ar, Bs, Krs), affine, as gnark's prover arranges them"""
    A, B1, K, Z, B2 = sums
    ar = ref.g1_add(ref.g1_add(A, pts["alpha"]), ref.g1_mul(pts["delta"], r))
    bs1 = ref.g1_add(ref.g1_add(B1, pts["beta"]), ref.g1_mul(pts["delta"], s))
    bs = ref.g2_add(ref.g2_add(B2, pts["beta2"]), ref.g2_mul(pts["delta2"], s))
    krs = ref.g1_add(ref.g1_add(K, Z), ref.g1_add(ref.g1_mul(ar, s), ref.g1_mul(bs1, r)))
    krs = ref.g1_add(krs, ref.g1_neg(ref.g1_mul(pts["delta"], r * s % R)))
    return ar, bs, krs


def library_arrangement(pts, sums, r: int, s: int):
    """(Ar, Bs, Krs), affine, as the library arranges them: Krs = K + Z + s (A + alpha) + r (B1 + beta) + rs delta"""
    A, B1, K, Z, B2 = sums
    a_alpha, b_beta = ref.g1_add(A, pts["alpha"]), ref.g1_add(B1, pts["beta"])
    ar = ref.g1_add(a_alpha, ref.g1_mul(pts["delta"], r))
    bs = ref.g2_add(ref.g2_add(B2, pts["beta2"]), ref.g2_mul(pts["delta2"], s))
    krs = ref.g1_add(ref.g1_add(K, Z), ref.g1_add(ref.g1_mul(a_alpha, s), ref.g1_mul(b_beta, r)))
    krs = ref.g1_add(krs, ref.g1_mul(pts["delta"], r * s % R))
    return ar, bs, krs


def _row(which, tag, logs, r, s, rng, inf=(), junk_inf=False, split=None, expect=True, extra=None):
    """logs: discrete logarithms (a, b1, k, z, b2) of the row's five sums.  split: None = one record; "eq_eq_opp" = three records P, P, -P"""
    _, pts = key(which)
    sums = tuple(g1(v) for v in logs[:4]) + (g2(logs[4]),)
    if split is None:
        parts = record(sums, rng, junk_inf)[None, :]
    else:
        neg = tuple(ref.g1_neg(P) for P in sums[:4]) + (ref.g2_neg(sums[4]),)
        parts = np.stack([record(sums, rng, junk_inf), record(sums, rng, junk_inf), record(neg, rng, junk_inf)])
    exp = ref.groth16_proof_bytes(*gnark_form(pts, sums, r, s)) if expect else None
    pre = dict(sums=sums, r=r, s=s, inf=tuple(inf), key=which)
    pre.update(extra or {})
    return Row(parts, fr_mont(r), fr_mont(s), exp, tag, pre)


@functools.lru_cache(maxsize=None)
def tagged_rows(which: str = "base"):
    """every tagged case (one record per row) and two random rows, each with its expectation"""
    ks = KEY_SCALARS if which == "base" else KEY_SCALARS_OTHER_DELTA
    al, be, de, be2, de2 = (ks[k] for k in ("alpha", "beta", "delta", "beta2", "delta2"))
    rng = _Rng(0x7A11 + (which != "base"))
    rnd = lambda: rng.below(R - 2) + 1  # noqa: E731
    rows = []

    def add(tag, logs, r=None, s=None, **kw):
        rows.append(_row(which, tag, tuple(v % R for v in logs), rnd() if r is None else r, rnd() if s is None else s, rng, **kw))

    a, b, k, z, b2 = rnd(), rnd(), rnd(), rnd(), rnd()
    add("random_0", (a, b, k, z, b2))
    add("all_sums_at_infinity", (0, 0, 0, 0, 0), inf=("A", "B1", "K", "Z", "B2"))
    add("A_at_infinity", (0, b, k, z, b2), inf=("A",))
    add("B1_at_infinity", (a, 0, k, z, b2), inf=("B1",))
    add("K_at_infinity_junk_xy", (a, b, 0, z, b2), inf=("K",), junk_inf=True)
    add("Z_at_infinity", (a, b, k, 0, b2), inf=("Z",))
    add("B2_at_infinity_junk_xy", (a, b, k, z, 0), inf=("B2",), junk_inf=True)
    add("A_is_minus_alpha", (-al, b, k, z, b2), inf=("A+alpha",))
    add("B1_is_minus_beta", (a, -be, k, z, b2), inf=("B1+beta",))
    r, s = rnd(), rnd()
    add("Bs_at_infinity", (a, b, k, z, -be2 - s * de2), r, s, inf=("Bs",))
    add("Ar_at_infinity", (-al - r * de, b, k, z, b2), r, s, inf=("Ar",))
    add("K_equals_Z", (a, b, k, k, b2), extra=dict(k_equals_z=True))
    add("K_is_minus_Z", (a, b, k, -k, b2), inf=("K+Z",))
    add("Krs_at_infinity", (a, b, -(z + s * (a + al) + r * (b + be) + r * s * de), z, b2), r, s, inf=("Krs",))
    add("r_zero", (a, b, k, z, b2), r=0)
    add("s_zero", (a, b, k, z, b2), s=0)
    add("r_and_s_zero", (a, b, k, z, b2), r=0, s=0)
    add("r_one", (a, b, k, z, b2), r=1)
    add("s_is_r_mod_minus_1", (a, b, k, z, b2), s=R - 1)
    add("random_1", (rnd(), rnd(), rnd(), rnd(), rnd()))
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def tagged_rows_3(which: str = "base"):
    """n_partials = 3: every sum arrives as two equal records and one opposite record (an addition that doubles, then one that meets the opposite of a
    summand); the second row has every sum at infinity three times over"""
    rng = _Rng(0x3333)
    rnd = lambda: rng.below(R - 2) + 1  # noqa: E731
    return (_row(which, "np3_equal_equal_opposite", (rnd(), rnd(), rnd(), rnd(), rnd()), rnd(), rnd(), rng, split="eq_eq_opp"),
            _row(which, "np3_all_at_infinity_junk_xy", (0, 0, 0, 0, 0), rnd(), rnd(), rng, split="eq_eq_opp", junk_inf=True, inf=("A", "B1", "K", "Z", "B2")))


@functools.lru_cache(maxsize=None)
def _pool(n_points=12):
    return [g1(0xC0FFEE + 977 * i) for i in range(n_points)], [g2(0xBEEF + 131 * i) for i in range(4)]


def bulk_rows(n: int, n_partials: int, seed: int):
    """(partials (n, n_partials, 96), r (n, 4), s (n, 4)) without expectations: records drawn from a small pool of points under fresh projective factors, uniform
    r and s.  Every tenth record is a point at infinity in one of its five places."""
    p1, p2 = _pool()
    rng = _Rng(seed)
    parts = np.zeros((n, n_partials, 96), dtype=np.uint64)
    for i in range(n):
        for j in range(n_partials):
            pts = [p1[rng.below(len(p1))] for _ in range(4)] + [p2[rng.below(len(p2))]]
            if (i * n_partials + j) % 10 == 9:
                pts[rng.below(5)] = None
            parts[i, j] = record(tuple(pts), rng)
    r = np.stack([fr_mont(rng.below(R)) for _ in range(n)])
    s = np.stack([fr_mont(rng.below(R)) for _ in range(n)])
    return parts, r, s


def assemble(n: int, n_partials: int, seed: int, tagged, positions):
    """bulk rows with the tagged rows written over the given positions (cycling through `tagged`): (partials, r, s, {position: Row})"""
    parts, r, s = bulk_rows(n, n_partials, seed)
    placed = {}
    for t, pos in enumerate(p for p in positions if 0 <= p < n):
        row = tagged[t % len(tagged)]
        assert row.partials.shape[0] == n_partials
        parts[pos], r[pos], s[pos] = row.partials, row.r, row.s
        placed[pos] = row
    return parts, r, s, placed
