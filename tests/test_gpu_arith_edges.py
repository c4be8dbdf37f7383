"""GPU suite: the device field and curve arithmetic, one production inline function at a time (libzkmi_probe.so, tests/probe.py), against big
integers at the edges of its proven bounds.  Three levels: the value (== the big-integer result mod p or r), the bound the function's header
documents, and -- where tools/u29_model.py / u29_ntt_model.py have an exact limb algorithm -- the raw limbs bit for bit."""
import random

import pytest

from oracle import bn254_ref as ref
from tests import arith_edges as E
from tests import probe

pytestmark = pytest.mark.gpu

P, R, M, MR = E.P, E.R, E.M, E.MR
N29 = 8192   # vectors per 29-bit op


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from noir_backend_using_gnark_amd import _lib
    _lib.require_device()


def rows(a):
    return [[int(v) for v in r] for r in a]


def assert_rows(name, got, exp, labels=None):
    got = rows(got)
    for k, (g, e) in enumerate(zip(got, exp)):
        if g != list(e):
            raise AssertionError("%s vector %d%s: got %s, expected %s" % (name, k, " (%s)" % labels[k] if labels else "", g, list(e)))


# ------------------------------------------------------------------------------------------------------------ saturated Fp / Fr
@pytest.mark.parametrize("field", ["FP", "FR"])
def test_saturated_field_ops(field):
    m = P if field == "FP" else R
    rinv = pow(1 << 256, -1, m)
    rng = random.Random(1 if field == "FP" else 2)
    a = E.canon_vals(rng, m, 2048)
    b = E.canon_vals(rng, m, 2048)
    rng.shuffle(b)
    edges = E.canon_edges(m)
    a += [x for x in edges for _ in edges]   # every edge against every edge
    b += [y for _ in edges for y in edges]
    expect = {
        "MUL": lambda x, y: x * y * rinv % m, "SQR": lambda x, y: x * x * rinv % m, "ADD": lambda x, y: (x + y) % m,
        "SUB": lambda x, y: (x - y) % m, "NEG": lambda x, y: (-x) % m, "TO_MONT": lambda x, y: x * (1 << 256) % m,
        "FROM_MONT": lambda x, y: x * rinv % m,
    }
    vin = [E.words(x) + E.words(y) for x, y in zip(a, b)]
    for op, f in expect.items():
        got = probe.run("%s_%s" % (field, op), vin)
        assert_rows("%s_%s" % (field, op), got, [E.words(f(x, y)) for x, y in zip(a, b)])
    # inversion: the Montgomery image of x^-1, inv(0) = 0 (a few hundred: 256 squarings and products per lane)
    xs = a[:384]
    got = probe.run("%s_INV" % field, [E.words(x) for x in xs])
    assert_rows("%s_INV" % field, got, [E.words(0 if x == 0 else pow(x * rinv, -1, m) * (1 << 256) % m) for x in xs])
    # reduce_once: every t < 2m, including t == m and t == 2m - 1
    ts = [0, 1, m - 1, m, m + 1, 2 * m - 1, 2 * m - 2] + [rng.randrange(2 * m) for _ in range(2000)]
    got = probe.run("%s_REDUCE_ONCE" % field, [E.words(t) for t in ts])
    assert_rows("%s_REDUCE_ONCE" % field, got, [E.words(t - m if t >= m else t) for t in ts])
    # from_mont of NON-canonical images in [m, 2^256): the batch verifiers pass caller-supplied public inputs through it
    ts = [m, m + 1, 2 * m - 1, 2 * m, 5 * m - 1, (1 << 256) - 1, (1 << 256) - m] + [rng.randrange(m, 1 << 256) for _ in range(2000)]
    got = probe.run("%s_FROM_MONT" % field, [E.words(t) for t in ts])
    assert_rows("%s_FROM_MONT (non-canonical)" % field, got, [E.words(t * rinv % m) for t in ts])


def test_fp2_ops():
    rng = random.Random(3)
    edges = [(0, 0), (1, 0), (0, 1), (P - 1, P - 1), (P - 1, 0), (0, P - 1), (1, P - 1)]
    a = edges + [E.rand_f2(rng) for _ in range(1024)]
    b = edges[::-1] + [E.rand_f2(rng) for _ in range(1024)]
    vin = [E.img2(x) + E.img2(y) for x, y in zip(a, b)]
    assert_rows("FP2_MUL", probe.run("FP2_MUL", vin), [E.img2(E.f2m(x, y)) for x, y in zip(a, b)])
    assert_rows("FP2_SQR", probe.run("FP2_SQR", vin), [E.img2(E.f2m(x, x)) for x in a])
    vin = vin[:256]
    assert_rows("FP2_INV", probe.run("FP2_INV", vin), [E.img2((0, 0) if x == (0, 0) else E.f2i(x)) for x in a[:256]])


def test_f6_f12_tower():
    rng = random.Random(4)
    n = 192
    a6, b6 = [E.rand_f6(rng) for _ in range(n)], [E.rand_f6(rng) for _ in range(n)]
    a6[0], b6[0] = E.F6_1, E.F6_0
    got = probe.run("F6_MUL", [E.img6(x) + E.img6(y) for x, y in zip(a6, b6)])
    assert_rows("F6_MUL", got, [E.img6(E.f6_mul(x, y)) for x, y in zip(a6, b6)])
    got = probe.run("F6_INV", [E.img6(x) for x in a6[:64]])
    assert_rows("F6_INV", got, [E.img6(E.f6_inv(x)) for x in a6[:64]])

    a, b = [E.rand_f12(rng) for _ in range(n)], [E.rand_f12(rng) for _ in range(n)]
    a[0], b[0] = E.F12_1, E.F12_1
    vin = [E.img12(x) + E.img12(y) for x, y in zip(a, b)]
    assert_rows("F12_MUL", probe.run("F12_MUL", vin), [E.img12(E.f12_mul(x, y)) for x, y in zip(a, b)])
    assert_rows("F12_SQR", probe.run("F12_SQR", vin), [E.img12(E.f12_mul(x, x)) for x in a])
    assert_rows("F12_CONJ", probe.run("F12_CONJ", vin), [E.img12(E.f12_conj(x)) for x in a])
    # inverse: the device result times the input is one (checked independently of the formula) and equals the Python tower's
    got = probe.run("F12_INV", vin[:64])
    for k in range(64):
        inv = E.unimg12([int(v) for v in got[k]])
        assert E.f12_mul(a[k], inv) == E.F12_1, k
    # a D-twist line l0 + l1 w + l3 w^3 = (l0, 0, 0) + (l1, l3, 0) w
    lines = [(E.rand_f2(rng), E.rand_f2(rng), E.rand_f2(rng)) for _ in range(n)]
    got = probe.run("F12_MUL_LINE", [E.img12(x) + E.img2(l[0]) + E.img2(l[1]) + E.img2(l[2]) for x, l in zip(a, lines)])
    assert_rows("F12_MUL_LINE", got, [E.img12(E.f12_mul(x, ((l[0], E.F2_0, E.F2_0), (l[1], l[2], E.F2_0)))) for x, l in zip(a, lines)])
    # Frobenius: f^p and f^(p^2) by exponentiation, with the constants gnark's tower implies
    nf = 6
    g1 = sum((E.img2(g) for g in E.FROB_G1), [])
    g2 = sum((E.img(g[0]) for g in E.FROB_G2), [])
    got = probe.run("F12_FROB", [E.img12(x) + g1 for x in a[:nf]])
    assert_rows("F12_FROB", got, [E.img12(E.f12_pow(x, P)) for x in a[:nf]])
    got = probe.run("F12_FROB2", [E.img12(x) + g2 for x in a[:nf]])
    assert_rows("F12_FROB2", got, [E.img12(E.f12_pow(x, P * P)) for x in a[:nf]])
    # cyclotomic squaring on elements of the cyclotomic subgroup
    cyc = [E.F12_1] + [E.cyclotomic(x) for x in a[1:17]]
    got = probe.run("F12_CYC_SQR", [E.img12(x) for x in cyc])
    assert_rows("F12_CYC_SQR", got, [E.img12(E.f12_mul(x, x)) for x in cyc])


# ------------------------------------------------------------------------------------------------------------ saturated curve (curve.hpp)
def _curve_case(F, pts, rng, randz):
    """(A, B) pairs: random, A == B, A == -B, infinity on either side"""
    out = []
    for i in range(len(pts) - 1):
        p1, p2 = pts[i], pts[i + 1]
        for q1, q2 in ((p1, p2), (p1, p1), (p1, ref.ec_neg(F, p1)), (None, p2), (p1, None), (None, None)):
            out.append((q1, q2, E.xyzz_of(F, q1, randz()), E.xyzz_of(F, q2, randz())))
    return out


@pytest.mark.parametrize("g", ["G1", "G2"])
def test_saturated_xyzz_ops(g):
    rng = random.Random(6)
    if g == "G1":
        F, pts, randz = ref.FP, [E.g1_point(rng) for _ in range(24)], lambda: rng.randrange(1, P)
        im = lambda c: sum((E.img(v) for v in c), [])
        un = lambda w, k: E.unimg(w[8 * k:8 * k + 8])
        W = 8
    else:
        F, pts, randz = ref.FP2, E.g2_points(8, 1234567), lambda: (rng.randrange(1, P), rng.randrange(P))
        im = lambda c: sum((E.img2(v) for v in c), [])
        un = lambda w, k: E.unimg2(w[16 * k:16 * k + 16])
        W = 16
    cases = _curve_case(F, pts, rng, randz)
    aff = lambda w: None if F.is_zero(un(w, 2)) else (F.mul(un(w, 0), F.inv(un(w, 2))), F.mul(un(w, 1), F.inv(un(w, 3))))
    def check(op, exp_fn, inp):
        got = rows(probe.run("%s_%s" % (g, op), inp))
        for k, (c, w) in enumerate(zip(cases, got)):
            assert aff(w) == exp_fn(c), (op, k)
            assert all(unwords_lt(w[W * i:W * i + W]) for i in range(4)), (op, k)   # every saturated output canonical
    def unwords_lt(w):
        return all(E.unwords(w[j:j + 8]) < P for j in range(0, len(w), 8))
    zero_k = [0] * 8
    inp = [im(c[2]) + im(c[3]) + zero_k for c in cases]
    check("ADD", lambda c: ref.ec_add(F, c[0], c[1]), inp)
    check("DBL", lambda c: ref.ec_add(F, c[0], c[0]), inp)
    # madd / dbl_affine / scalar_mul read affine points: (x, y, 1, 1), infinity (0, 0)
    affx = lambda p: im((F.zero, F.zero, F.zero, F.zero) if p is None else (p[0], p[1], F.zero, F.zero))
    inp = [im(c[2]) + affx(c[1]) + zero_k for c in cases]
    check("MADD", lambda c: ref.ec_add(F, c[0], c[1]), inp)
    inp = [affx(c[0]) + affx(c[1]) + zero_k for c in cases]
    check("DBL_AFFINE", lambda c: ref.ec_add(F, c[0], c[0]), inp)
    got = rows(probe.run("%s_TO_AFFINE" % g, [im(c[2]) + im(c[3]) + zero_k for c in cases]))
    for k, (c, w) in enumerate(zip(cases, got)):
        exp = (F.zero, F.zero) if c[0] is None else c[0]
        assert (un(w, 0), un(w, 1)) == exp and unwords_lt(w[:2 * W]), ("TO_AFFINE", k)
    # scalar_mul: k = 0, 1, 2, r - 1 (-P), r (infinity), 2^128 - 1 (the verifiers' coefficient width), random
    ks = [0, 1, 2, R - 1, R, (1 << 128) - 1, rng.randrange(R), rng.randrange(1 << 128)]
    sp = pts[:4]
    inp = [affx(p) + im((F.zero,) * 4) + E.words(kv) for p in sp for kv in ks]
    got = rows(probe.run("%s_SCALAR_MUL" % g, inp))
    for k, w in enumerate(got):
        p, kv = sp[k // len(ks)], ks[k % len(ks)]
        assert aff(w) == ref.ec_mul(F, p, kv), ("SCALAR_MUL", kv)
    assert aff(got[3]) == ref.ec_neg(F, sp[0]) and aff(got[4]) is None


# ------------------------------------------------------------------------------------------------------------ 29-bit Fp ops
def _u29_mul_bounds(a, b, r):
    """u29_mul's header: limbs 0..7 < 2^29, value < a b / 2^261 + p"""
    assert all(v <= M.MASK for v in r[:8]) and E.val(r) < E.val(a) * E.val(b) // (1 << 261) + P + 1


def test_u29_mul_sqr_exact():
    rng = random.Random(7)
    vin, exp, pre = E.u29_mul_vectors(rng, N29)
    got = probe.run("U29_MUL", vin)
    assert_rows("U29_MUL", got, exp)
    for (a, b), r in zip(pre, rows(got)):
        _u29_mul_bounds(a, b, r)
        assert (E.val(r) - E.val(a) * E.val(b) * E.R29INV) % P == 0
    got = probe.run("U29_SQR", vin)
    assert_rows("U29_SQR", got, [M.sqr_exact(a) for a, _ in pre])
    # the interleaved pair forms are the same instructions: bit-identical to two single products
    x2 = [a + b + b + a for a, b in pre[:2048]]
    assert_rows("U29_MUL_X2", probe.run("U29_MUL_X2", x2), [M.mul_exact(a, b) + M.mul_exact(b, a) for a, b in pre[:2048]])
    s2 = [a + [0] * 9 + b for a, b in pre[:2048]]
    assert_rows("U29_SQR_X2", probe.run("U29_SQR_X2", s2), [M.sqr_exact(a) + M.sqr_exact(b) for a, b in pre[:2048]])


@pytest.mark.parametrize("N", [2, 3, 4])
def test_u29_mulN_exact(N):
    rng = random.Random(8 + N)
    vin, exp, pre = E.mulN_vectors(rng, 4096, N, E.TAIL_BOUND)
    got = probe.run("U29_MUL%d" % N, vin)
    assert_rows("U29_MUL%d" % N, got, exp)
    for ops, r in zip(pre, rows(got)):
        s = sum(E.val(ops[2 * t]) * E.val(ops[2 * t + 1]) for t in range(N))
        assert (E.val(r) - s * E.R29INV) % P == 0 and all(v <= M.MASK for v in r[:8])


@pytest.mark.parametrize("K", E.FP_KS)
def test_u29_sub_neg_exact(K):
    rng = random.Random(100 + K)
    vin, exp, pre = E.sub_vectors(rng, 2048, K)
    got = probe.run("U29_SUB%d" % K, vin)
    assert_rows("U29_SUB%d" % K, got, exp)
    for (a, b), r in zip(pre, rows(got)):
        assert E.val(r) == E.val(a) - E.val(b) + K * P
    got = probe.run("U29_NEG%d" % K, [b for _, b in pre])
    assert_rows("U29_NEG%d" % K, got, [E.neg_expect(b, K) for _, b in pre])
    for (_, b), r in zip(pre, rows(got)):
        assert E.val(r) == K * P - E.val(b) and all(v < M.MASK + 8 for v in r[:8])


def test_u29_add_norm_load_exact():
    rng = random.Random(9)
    ops = E.u29_operands(rng, E.TAIL_BOUND, 4096)
    big = [[rng.randrange(1 << 31) for _ in range(8)] + [rng.randrange(1 << 30)] for _ in range(2048)] + [[0xffffffff] * 8 + [0xf0000000]]
    pairs = list(zip(ops, ops[::-1]))
    assert_rows("U29_ADD", probe.run("U29_ADD", [a + b for a, b in pairs]), [M.add_exact(a, b) for a, b in pairs])
    for name in ("U29_WNORM", "U29_WNORM_FWD"):
        got = probe.run(name, big)
        assert_rows(name, got, [M.wnorm_exact(a) for a in big])
        assert all(v < M.MASK + 8 for r in rows(got) for v in r[:8])
    rip = big[:-1]
    got = probe.run("U29_RIPPLE", rip)
    assert_rows("U29_RIPPLE", got, [E.ripple(a) for a in rip])
    vs = E.canon_vals(rng, P, 2048)
    assert_rows("U29_LOAD", probe.run("U29_LOAD", [E.words(v) for v in vs]), [E.limbs(v << 5) for v in vs])
    us = vs + [(1 << 256) - 1, rng.randrange(1 << 256)]
    assert_rows("U29_UNPACK", probe.run("U29_UNPACK", [E.words(v) for v in us]), [E.limbs(v) for v in us])


def test_u29_store_and_pack_canonical():
    rng = random.Random(10)
    # u29_store: any lazily reduced value < 2^260 -> the canonical image x / 2^5 mod p
    xs = E.store_inputs(rng, 4096)
    got = probe.run("U29_STORE", xs)
    inv32 = pow(32, -1, P)
    assert_rows("U29_STORE", got, [E.words(E.val(x) * inv32 % P) for x in xs])
    # u29p_reduce: < 2.01 p with limbs 0..7 < 2^29, exactly the model's chain; u29p_pack: the value itself, canonical
    ws = xs + [[M.MASK + 8] * 8 + [t] for t in (0xffffffff - (1 << 11), 1 << 31, 0x0fffffff)]
    ws = [w for w in ws if all(v + (1 << 11) < 1 << 32 for v in w)]
    got = probe.run("U29P_REDUCE", ws)
    assert_rows("U29P_REDUCE", got, [M.reduce_exact_p(w) for w in ws])
    assert all(E.val(r) < 2.01 * P and all(v <= M.MASK for v in r[:8]) for r in rows(got))
    got = probe.run("U29P_PACK", ws)
    assert_rows("U29P_PACK", got, [E.words(E.val(w) % P) for w in ws])


def test_u29_zero_filters_never_miss():
    rng = random.Random(11)
    def run(name, vals):
        return [int(r[0]) for r in probe.run(name, [E.limbs(v) for v in vals])]
    # u29_mulout_is_zero: a product output < 2 p -- exact: true for 0 and p only
    for name, k in (("U29_MULOUT_IS_ZERO", 2), ("U29_MULOUT3_IS_ZERO", 3)):
        zeros = [j * P for j in range(k)]
        near = [z + d for z in zeros for d in (-16, -1, 1, 16) if 0 <= z + d < k * P] + [k * P - 1]
        rnd = [rng.randrange(k * P) for _ in range(4096)]
        got = run(name, zeros + near + rnd)
        exp = [1] * len(zeros) + [0] * len(near) + [int(v % P == 0) for v in rnd]
        assert got == exp, name
    # u29_maybe_zero16: a product output < 16 p -- never misses a multiple of p; false positives at the documented 2^-25 rate
    zeros = [j * P for j in range(16)]
    near = [z + d for z in zeros for d in (-16, -1, 1, 16) if 0 <= z + d < 16 * P]
    got = run("U29_MAYBE_ZERO16", zeros + near)
    assert got[:16] == [1] * 16
    rnd = [rng.randrange(16 * P) for _ in range(N29 * 4)]
    fp = sum(run("U29_MAYBE_ZERO16", rnd))
    assert fp <= 2, "false positives %d in %d (documented rate 2^-25)" % (fp, len(rnd))
    pinv = pow(P, -1, 1 << 29)
    assert got[16:] == [int((v & M.MASK) * pinv % (1 << 29) < 16) for v in near]


# ------------------------------------------------------------------------------------------------------------ 29-bit Fp2 / Fr ops
def test_f2_29_ops_exact():
    rng = random.Random(12)
    n = 2048
    A = [(a, b) for a, b in zip(E.u29_operands(rng, E.TAIL_BOUND, n), E.u29_operands(rng, E.TAIL_BOUND, n)[::-1])]
    B = A[1:] + A[:1]
    sub = lambda a, b, K: M.wnorm_exact(M.sub_exact(a, b, M.bias_limbs(K)))
    def mul29(a, b):
        v0, v1 = M.mul_exact(a[0], b[0]), M.mul_exact(a[1], b[1])
        s = M.mul_exact(M.add_exact(a[0], a[1]), M.add_exact(b[0], b[1]))
        return sub(v0, v1, 4) + M.wnorm_exact(M.sub_exact(M.sub_exact(s, v0, M.bias_limbs(4)), v1, M.bias_limbs(4)))
    # f2_mul29's subtrahends are product outputs: operands of the madd class (< 2 p) keep them inside the 4 p bias
    A2 = [(E.limbs(rng.randrange(2 * P)), E.limbs(rng.randrange(2 * P))) for _ in range(n)]
    B2 = A2[1:] + A2[:1]
    vin = [a[0] + a[1] + b[0] + b[1] for a, b in zip(A2, B2)]
    got = probe.run("F2_MUL29", vin)
    assert_rows("F2_MUL29", got, [mul29(a, b) for a, b in zip(A2, B2)])
    for a, b, r in zip(A2, B2, rows(got)):
        ea, eb = (E.from29(a[0]), E.from29(a[1])), (E.from29(b[0]), E.from29(b[1]))
        assert (E.from29(r[:9]), E.from29(r[9:])) == E.f2m(ea, eb)
    # f2_sqr29<8>: subtrahend a.c1 < 8 p
    S = [(E.limbs(rng.randrange(8 * P)), b) for b in E.dominated(rng, M.bias_limbs(8), n)]
    got = probe.run("F2_SQR29_8", [a[0] + a[1] for a in S])
    exp = []
    for a in S:
        m = M.mul_exact(a[0], a[1])
        exp.append(M.mul_exact(M.add_exact(a[0], a[1]), sub(a[0], a[1], 8)) + M.add_exact(m, m) + m)
    assert_rows("F2_SQR29_8", got, exp)
    # fused products: c0 = a0 b0 + na1 b1, c1 = a0 b1 + a1 b0, one reduction each
    fused = lambda a, b, na1: M.mulN_exact([(a[0], b[0]), (na1, b[1])]) + M.mulN_exact([(a[0], b[1]), (a[1], b[0])])
    for K in (4, 16, 40):
        AK = [(a[0], b) for a, b in zip(A, E.dominated(rng, M.bias_limbs(K), n))]
        got = probe.run("F2_MULFK29_%d" % K, [a[0] + a[1] + b[0] + b[1] for a, b in zip(AK, B)])
        assert_rows("F2_MULFK29_%d" % K, got, [fused(a, b, E.neg_expect(a[1], K)) for a, b in zip(AK, B)])
    na = [E.neg_expect(b, 40) for b in E.dominated(rng, M.bias_limbs(40), n)]
    got = probe.run("F2_MULF29", [a[0] + a[1] + b[0] + b[1] + x for a, b, x in zip(A, B, na)])
    assert_rows("F2_MULF29", got, [fused(a, b, x) for a, b, x in zip(A, B, na)])
    one = list(M.limbs((1 << M.RBITS) % P))
    got = probe.run("F2_CONTRACT29", [a[0] + a[1] for a in A])
    assert_rows("F2_CONTRACT29", got, [M.mul_exact(a[0], one) + M.mul_exact(a[1], one) for a in A])


def test_u29r_ops_exact():
    rng = random.Random(13)
    n = 4096
    lim = MR.limbs
    # operands of the NTT model's classes: data < 4 r (after a butterfly sum), twiddles canonical
    xs = [lim(v) for v in (0, 1, R - 1, R, 2 * R - 1, 4 * R - 1)] + [lim(rng.randrange(4 * R)) for _ in range(n)]
    ws = [lim(rng.randrange(R)) for _ in xs[:-1]] + [lim(R - 1)]
    got = probe.run("U29R_MUL", [x + w for x, w in zip(xs, ws)])
    assert_rows("U29R_MUL", got, [MR.mul_exact(x, w) for x, w in zip(xs, ws)])
    for K in E.FR_KS:
        bs = E.dominated(rng, MR.bias_limbs(K), n)
        as_ = [lim(rng.randrange(4 * R)) for _ in bs]
        got = probe.run("U29R_SUB%d" % K, [a + b for a, b in zip(as_, bs)])
        assert_rows("U29R_SUB%d" % K, got, [MR.sub_exact(a, b, K) for a, b in zip(as_, bs)])
    # u29r_reduce: x weakly normalised -> < 2.01 r, the model's chain bit for bit
    rs = [E.weak_rand(rng, 64 * R) for _ in range(n)] + [E.weak_max(64 * R), lim(64 * R - 1), lim(R), lim(2 * R)]
    got = probe.run("U29R_REDUCE", rs)
    assert_rows("U29R_REDUCE", got, [MR.reduce_exact(x) for x in rs])
    assert all(MR.val(r) < 2.01 * R and all(v <= MR.MASK for v in r[:8]) for r in rows(got))
    # pack: the reduce output, as 8 words; canonical = two conditional subtractions of r
    red = rows(got)
    got0, got1 = probe.run("U29R_PACK0", red), probe.run("U29R_PACK1", red)
    assert_rows("U29R_PACK0", got0, [E.words(MR.pack_exact(x, False)) for x in red])
    assert_rows("U29R_PACK1", got1, [E.words(MR.pack_exact(x, True)) for x in red])
    edge = [lim(v) for v in (R - 1, R, R + 1, 2 * R - 1, 2 * R, int(2.01 * R))]
    assert_rows("U29R_PACK1 edges", probe.run("U29R_PACK1", edge), [E.words(MR.val(x) % R) for x in edge])
    vs = E.canon_vals(rng, R, 1024)
    assert_rows("U29R_LOAD5", probe.run("U29R_LOAD5", [E.words(v) for v in vs]), [lim(v << 5) for v in vs])


# ------------------------------------------------------------------------------------------------------------ 29-bit points
def _acc_rec(c, inf=False):
    return sum((list(v) for v in c), []) + [1 if inf else 0]


def _acc_affine(w, F=ref.FP, comps=1):
    if w[9 * 4 * comps]:
        return None
    if comps == 1:
        c = [E.from29(w[9 * i:9 * i + 9]) for i in range(4)]
    else:
        c = [(E.from29(w[18 * i:18 * i + 9]), E.from29(w[18 * i + 9:18 * i + 18])) for i in range(4)]
    return E.affine_of(F, c)


def _acc_bounds(w, bounds, comps=1):
    if w[9 * 4 * comps]:
        return True
    for i in range(4 * comps):
        l = w[9 * i:9 * i + 9]
        if not (E.val(l) < bounds[i // comps] and all(v <= E.WMAX for v in l[:8])):
            return False
    return True


def _lazy_acc(pt, rng, bounds, F=ref.FP):
    """the accumulator of `pt` with a random z, every coordinate x + k p at its class bound"""
    if F is ref.FP:
        c = E.xyzz_of(F, pt, rng.randrange(1, P))
        return [E.lazy29(v, b, rng) for v, b in zip(c, bounds)]
    c = E.xyzz_of(F, pt, (rng.randrange(1, P), rng.randrange(P)))
    return sum(([E.lazy29(v[0], b, rng), E.lazy29(v[1], b, rng)] for v, b in zip(c, bounds)), [])


def test_acc29_g1_madd_edges():
    rng = random.Random(14)
    B = E.G1_MADD_BOUNDS
    vin, exp = [], []
    for _ in range(512):
        p1, p2 = E.g1_point(rng), E.g1_point(rng)
        for q2 in (p2, p1, ref.g1_neg(p1), None):
            vin.append(_acc_rec(_lazy_acc(p1, rng, B)) + E.img(q2[0] if q2 else 0) + E.img(q2[1] if q2 else 0))
            exp.append(ref.g1_add(p1, q2))
        vin.append(_acc_rec([[0] * 9] * 4, inf=True) + E.img(p2[0]) + E.img(p2[1]))
        exp.append(p2)
    got = rows(probe.run("ACC29_MADD", vin))
    for k, w in enumerate(got):
        assert _acc_affine(w) == exp[k], k
        assert _acc_bounds(w, B), (k, w)


def test_acc29_g1_madd_chain_reaches_fixed_point():
    """1000 madds onto one accumulator per lane, lazily reduced throughout, checked every 100; doublings and cancellations mid-chain"""
    rng = random.Random(15)
    lanes = 32
    accs = [E.g1_point(rng) for _ in range(lanes)]
    state = [_acc_rec([E.lazy29(v, b) for v, b in zip(E.xyzz_of(ref.FP, a, 1), [2 * P] * 4)]) for a in accs]
    for rnd in range(10):
        vin = []
        for ln in range(lanes):
            rec = list(state[ln])
            for s in range(100):
                if s == 37 and accs[ln] is not None and rnd % 3 == 1:
                    q = accs[ln]                           # == accumulator: doubling
                elif s == 71 and accs[ln] is not None and rnd % 3 == 2:
                    q = ref.g1_neg(accs[ln])               # == -accumulator: infinity
                else:
                    q = E.g1_point(rng)
                rec += E.img(q[0]) + E.img(q[1])
                accs[ln] = ref.g1_add(accs[ln], q)
            vin.append(rec)
        got = rows(probe.run("ACC29_MADD_CHAIN", vin))
        for ln, w in enumerate(got):
            assert _acc_affine(w) == accs[ln], (rnd, ln)
            assert _acc_bounds(w, E.G1_MADD_BOUNDS), (rnd, ln)
        state = got


def test_acc29_g2_madd_chain():
    rng = random.Random(16)
    lanes = 8
    F = ref.FP2
    rp = lambda: (E.rand_f2(rng), E.rand_f2(rng))   # the chord rule is an identity: points need not lie on the twist
    accs = [rp() for _ in range(lanes)]
    state = [_acc_rec(sum(([E.lazy29(v[0], 2 * P), E.lazy29(v[1], 2 * P)] for v in E.xyzz_of(F, a, (1, 0))), [])) for a in accs]
    for rnd in range(3):
        vin = []
        for ln in range(lanes):
            rec = list(state[ln])
            for s in range(100):
                q = accs[ln] if (s == 50 and rnd == 1) else rp()
                rec += E.img2(q[0]) + E.img2(q[1])
                accs[ln] = ref.ec_add(F, accs[ln], q)
            vin.append(rec)
        got = rows(probe.run("ACC29G2_MADD_CHAIN", vin))
        for ln, w in enumerate(got):
            assert _acc_affine(w, F, 2) == accs[ln], (rnd, ln)
            assert _acc_bounds(w, E.G2_MADD_BOUNDS, 2), (rnd, ln)
        state = got


def test_acc29_g1_add_dbl_tail_class():
    rng = random.Random(17)
    T = [E.TAIL_BOUND] * 4
    cases = []
    for _ in range(256):
        p1, p2 = E.g1_point(rng), E.g1_point(rng)
        for q2 in (p2, p1, ref.g1_neg(p1), None):
            cases.append((p1, q2))
        cases.append((None, p2))
    rec = lambda p: _acc_rec([[0] * 9] * 4, True) if p is None else _acc_rec(_lazy_acc(p, rng, T))
    vin = [rec(a) + rec(b) for a, b in cases]
    add, dbl = rows(probe.run("ACC29_ADD", vin)), rows(probe.run("ACC29_DBL", vin))
    for k, (a, b) in enumerate(cases):
        assert _acc_affine(add[k]) == ref.g1_add(a, b), ("add", k)
        assert _acc_affine(dbl[k]) == ref.g1_add(a, a), ("dbl", k)
        assert _acc_bounds(add[k], T) and _acc_bounds(dbl[k], T), k
    # the quad forms: four lanes, identical operands.  X3, ZZ3 and ZZZ3 are the same product sequence as the single-lane forms, so bit-identical;
    # Y3 is not (two products and a subtraction instead of one fused product): the same value mod p, inside the class
    quad = [v for v in vin for _ in range(4)]
    for name, single in (("ACC29_ADD_QUAD", add), ("ACC29_DBL_QUAD", dbl)):
        got = rows(probe.run(name, quad))
        for k in range(len(got)):
            s1, g1 = single[k // 4], got[k]
            assert g1 == got[k - k % 4], (name, k)                                  # the four lanes agree
            assert g1[36] == s1[36], (name, k)
            if s1[36]:
                continue
            assert g1[0:9] == s1[0:9] and g1[18:36] == s1[18:36], (name, k)
            assert (E.val(g1[9:18]) - E.val(s1[9:18])) % P == 0 and _acc_bounds(g1, T), (name, k)
    # interchange round trip: acc29_to_packed (canonical words of the value itself) -> acc29_load
    got = rows(probe.run("ACC29_PACK_LOAD", vin))
    for k, w in enumerate(got):
        src = vin[k]
        if src[36]:
            assert w[36] == 1
            continue
        packed = [E.unwords(w[37 + 8 * i:45 + 8 * i]) for i in range(4)]
        assert packed == [E.val(src[9 * i:9 * i + 9]) % P for i in range(4)], k
        assert w[:36] == sum((E.limbs(v) for v in packed), []) and w[36] == 0, k


def test_acc29_g2_add_dbl_tail_class():
    rng = random.Random(18)
    F = ref.FP2
    T = [E.TAIL_BOUND] * 4
    pts = E.g2_points(12, 777)
    cases = []
    for i in range(len(pts) - 1):
        p1, p2 = pts[i], pts[i + 1]
        cases += [(p1, p2), (p1, p1), (p1, ref.g2_neg(p1)), (p1, None), (None, p2)]
    rec = lambda p: _acc_rec([[0] * 9] * 8, True) if p is None else _acc_rec(_lazy_acc(p, rng, T, F))
    vin = [rec(a) + rec(b) for a, b in cases]
    add, dbl = rows(probe.run("ACC29G2_ADD", vin)), rows(probe.run("ACC29G2_DBL", vin))
    for k, (a, b) in enumerate(cases):
        assert _acc_affine(add[k], F, 2) == ref.g2_add(a, b), ("add", k)
        assert _acc_affine(dbl[k], F, 2) == ref.g2_add(a, a), ("dbl", k)
        assert _acc_bounds(add[k], T, 2) and _acc_bounds(dbl[k], T, 2), k
    # madd with the accumulator at the fused madd's class bounds
    B = E.G2_MADD_BOUNDS
    vin, exp = [], []
    for i in range(len(pts) - 1):
        p1, p2 = pts[i], pts[i + 1]
        for q in (p2, p1, ref.g2_neg(p1)):
            vin.append(_acc_rec(_lazy_acc(p1, rng, B, F)) + E.img2(q[0]) + E.img2(q[1]))
            exp.append(ref.g2_add(p1, q))
    got = rows(probe.run("ACC29G2_MADD", vin))
    for k, w in enumerate(got):
        assert _acc_affine(w, F, 2) == exp[k], k
        assert _acc_bounds(w, B, 2), k


# ------------------------------------------------------------------------------------------------------------ SHA-256
def test_sha256_dev_every_length():
    recs, exp, lab = E.sha_vectors()
    got = probe.run("SHA256", recs)
    assert_rows("SHA256", got, exp, lab)
