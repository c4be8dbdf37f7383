"""The Lagrange-form transform of a base array (csrc/lagrange.hip: k_lag_scale_in, k_lag_dif_stage, k_lag_finish) as a discrete-log model in Python integers.

Every base is [k_j] G with k_j = 0 for the point at infinity, so every entry of every stage is an integer mod r and the group law's special cases are plain facts
about integers: a butterfly's operands are EQUAL when a == b, OPPOSITE when a + b == 0, one is INFINITE when it is 0.  stages() replays the kernels' own order --
scale by 1 / n, decimation-in-frequency stages m = n / 2 ... 1 with a' = a + b, b' = (a - b) w^(-k n / 2m), bit reversal, the two blinding differences -- and
walk() counts, stage by stage, the butterflies that meet each special case, so that a test says of its own input which branches it takes.

tests/test_lagrange_ref_cpu.py holds the model against the definition, the oracle's FFTInverse and bn254_ref's EC arithmetic; tests/test_gpu_lagrange_stages.py holds
zk_bn254_lagrange_inspect against it."""
import random

import numpy as np

from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import helpers

R = ref.R
SIZES = (0, 1, 2, 8, 9, 10)  # the smallest log_n at which each launch shape occurs (tests/test_gpu_lagrange_stages.py says which)


def omega(log_n: int) -> int:
    return ref.Domain(1 << log_n).gen


def bitrev(i: int, log_n: int) -> int:
    return ref.bitrev(i, log_n)


def twiddle_exponent(k: int, n: int, m: int) -> int:
    """the butterfly (blk 2m + k, blk 2m + k + m) multiplies its difference by w^(-e), e = k n / (2 m)"""
    return k * (n // (2 * m))


def stages(ks, log_n: int) -> dict:
    """ks: at least n + 2 integers mod r (the bases' discrete logs) -> work: log_n + 1 lists of n integers, the array after the scale-in and after every stage in
    the device's order; final: n + 2 integers, the transform in natural order followed by k_n - k_0 and k_(n+1) - k_1"""
    n = 1 << log_n
    assert len(ks) >= n + 2
    ninv, winv = ref.inv(n, R), ref.inv(omega(log_n), R)
    tw = [1] * max(n // 2, 1)
    for e in range(1, n // 2):
        tw[e] = tw[e - 1] * winv % R
    a = [k % R * ninv % R for k in ks[:n]]
    work = [list(a)]
    m = n // 2
    while m >= 1:
        blocks = n // (2 * m)
        for blk in range(blocks):
            for k in range(m):
                i = blk * 2 * m + k
                x, y = a[i], a[i + m]
                a[i], a[i + m] = (x + y) % R, (x - y) * tw[k * blocks] % R
        work.append(list(a))
        m //= 2
    final = [a[bitrev(i, log_n)] for i in range(n)] + [(ks[n] - ks[0]) % R, (ks[n + 1] - ks[1]) % R]
    return dict(work=work, final=final)


KINDS = ("equal", "opposite", "inf_operand", "inf_into_mul")


def pair_kinds(x: int, y: int) -> set:
    """what the group law sees in the pair (x, y) of an addition x + y and a subtraction x - y"""
    out = set()
    if x % R == 0 or y % R == 0:
        out.add("inf_operand")
    elif x % R == y % R:
        out.add("equal")          # x + y doubles, x - y is infinite
    elif (x + y) % R == 0:
        out.add("opposite")       # x + y is infinite, x - y doubles
    return out


def walk(ks, log_n: int) -> dict:
    """counts of the special cases: inf_in (bases at infinity among the first n), stage[s - 1] for stage s = 1 .. log_n: {equal, opposite, inf_operand: butterflies
    with such operands; inf_into_mul: butterflies whose a - b is infinite AND meets the scalar multiplication (e != 0)}, blind[0 / 1]: the kinds of the pair
    (P_n, P_0) / (P_(n+1), P_1) plus inf_hi / inf_lo, and inf_out: entries of the transform that are infinite"""
    n = 1 << log_n
    st = stages(ks, log_n)
    per = []
    m = n // 2
    for s in range(1, log_n + 1):
        before, c = st["work"][s - 1], dict.fromkeys(KINDS, 0)
        blocks = n // (2 * m)
        for blk in range(blocks):
            for k in range(m):
                x, y = before[blk * 2 * m + k], before[blk * 2 * m + k + m]
                for kind in pair_kinds(x, y):
                    c[kind] += 1
                if (x - y) % R == 0 and twiddle_exponent(k, n, m) != 0:
                    c["inf_into_mul"] += 1
        per.append(c)
        m //= 2
    blind = []
    for lane in (0, 1):
        hi, lo = ks[n + lane] % R, ks[lane] % R
        blind.append(dict(kinds=pair_kinds(hi, lo), inf_hi=hi == 0, inf_lo=lo == 0))
    return dict(inf_in=sum(1 for k in ks[:n] if k % R == 0), stage=per, blind=blind, inf_out=sum(1 for v in st["final"][:n] if v == 0))


def special_total(w: dict) -> int:
    return w["inf_in"] + sum(sum(c.values()) for c in w["stage"]) + sum(len(b["kinds"]) for b in w["blind"])


# ---- expected points
def points(ks) -> np.ndarray:
    """[k] G for every k as gnark's affine image ((0, 0) for k = 0): tests.helpers.g1_points_from_scalars -- bn254_ref's own double-and-add -- for up to 16
    distinct scalars, the oracle's fixed-base multiplication beyond (test_lagrange_ref_cpu.py holds the two against each other)"""
    ks = [k % R for k in ks]
    uniq = sorted(set(ks))
    if len(uniq) <= 16:
        img = helpers.g1_points_from_scalars(uniq)
    else:
        img = orc.g1_mul_gen_many(orc.ints_to_limbs(uniq), scalars_mont=False)
    at = {k: i for i, k in enumerate(uniq)}
    return img[[at[k] for k in ks]]


# ---- input families: n + 2 discrete logs each
def _nonzero(rng):
    return rng.randrange(1, R)


def fam_random(rng, log_n):
    return [_nonzero(rng) for _ in range((1 << log_n) + 2)]


def fam_all_equal(rng, log_n):
    n, k = 1 << log_n, _nonzero(rng)
    return [k] * n + [_nonzero(rng), _nonzero(rng)]


def fam_alternating(rng, log_n):
    n, k = 1 << log_n, _nonzero(rng)
    return [k if j % 2 == 0 else R - k for j in range(n)] + [_nonzero(rng), _nonzero(rng)]


def fam_half_negated(rng, log_n):
    n = 1 << log_n
    half = [_nonzero(rng) for _ in range(n // 2)]
    return half + [R - k for k in half] + [_nonzero(rng), _nonzero(rng)]


def fam_one_hot(rng, log_n, i0):
    """the forward transform of c delta_(i0): k_j = c w^(i0 j), whose inverse transform is c at i0 and 0 elsewhere"""
    n, c, w = 1 << log_n, _nonzero(rng), omega(log_n)
    return [c * pow(w, i0 * j, R) % R for j in range(n)] + [_nonzero(rng), _nonzero(rng)]


def fam_third_infinite(rng, log_n):
    n = 1 << log_n
    ks = fam_random(rng, log_n)
    for j in rng.sample(range(n), max(n // 3, 1)):
        ks[j] = 0
    return ks


def fam_all_infinite(rng, log_n):
    return [0] * ((1 << log_n) + 2)


def fam_pairs_at_stage(rng, log_n, s):
    """an input whose first equal pair AND first opposite pair sit in front of stage s (1-based), none earlier: the array in front of stage s is drawn at random
    with one equal and one opposite butterfly planted in it, and the stages before it are undone (a = (a' + b' / t) / 2, b = (a' - b' / t) / 2), the scale-in
    last"""
    n = 1 << log_n
    assert 1 <= s <= log_n and n >= 4
    m = n >> s
    a = [_nonzero(rng) for _ in range(n)]
    blocks = n // (2 * m)
    pairs = [(blk * 2 * m + k, blk * 2 * m + k + m) for blk in range(blocks) for k in range(m)]
    (i, j), (u, v) = rng.sample(pairs, 2)
    a[j] = a[i]
    a[v] = R - a[u]
    w, half = omega(log_n), ref.inv(2, R)
    for back in range(s - 1, 0, -1):  # undo stage `back`
        mb = n >> back
        bl = n // (2 * mb)
        for blk in range(bl):
            for k in range(mb):
                p = blk * 2 * mb + k
                x, y = a[p], a[p + mb] * pow(w, k * bl, R) % R
                a[p], a[p + mb] = (x + y) * half % R, (x - y) * half % R
    return [v * n % R for v in a] + [_nonzero(rng), _nonzero(rng)]


BLINDING = ("equal", "opposite", "hi_infinite", "lo_infinite", "both_infinite")


def fam_blinding(rng, log_n, lane, case):
    """random bases with the pair (P_(n + lane), P_lane) of blinding lane `lane` made equal, opposite, or infinite"""
    n = 1 << log_n
    ks = fam_random(rng, log_n)
    hi, lo = n + lane, lane
    if case == "equal":
        ks[hi] = ks[lo]
    elif case == "opposite":
        ks[hi] = R - ks[lo]
    elif case == "hi_infinite":
        ks[hi] = 0
    elif case == "lo_infinite":
        ks[lo] = 0
    elif case == "both_infinite":
        ks[hi] = ks[lo] = 0
    else:
        raise ValueError(case)
    return ks


def rng_for(*key) -> random.Random:
    return random.Random("lagrange/" + "/".join(str(k) for k in key))
