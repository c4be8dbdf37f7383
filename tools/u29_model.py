#!/usr/bin/env python3
"""Exact + worst-case model of the unsaturated 9 x 29-bit-limb Montgomery arithmetic (radix R' = 2^261) used by the
gfx950 accumulate kernels (csrc/ff29.hpp).  Two jobs:

  1. static bound propagation: every value carries (max value, max limb); `mul` asserts that no 64-bit column
     accumulator can overflow and `sub` that its bias dominates the subtrahend limb-wise -- run over the XYZZ formulas
     for G1 (Fp) and G2 (Fp2), iterated to a fixed point, this PROVES the schedule overflow-free for any input;
  2. randomized exact simulation of the same limb algorithms against Python big ints.

It also prints the constants the C++ needs (p limbs, -p^-1 mod 2^29, bias vectors).
"""
import random
import sys

Q = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47
W, NL = 29, 9
MASK = (1 << W) - 1
RBITS = W * NL  # 261
NINV = (-pow(Q, -1, 1 << W)) % (1 << W)


def limbs(x):
    return [(x >> (W * i)) & MASK for i in range(NL - 1)] + [x >> (W * (NL - 1))]


def val(l):
    return sum(v << (W * i) for i, v in enumerate(l))


PL = limbs(Q)


def bias_limbs(k):
    """k*p written with every limb >= 2^30 (top limb: whatever is left), so that a + bias - b never goes negative limb-wise
    for a weakly normalised b."""
    d = limbs(k * Q)
    out = [d[0] + (1 << 30)] + [d[i] + (1 << 30) - 2 for i in range(1, NL - 1)] + [d[NL - 1] - 2]
    assert val(out) == k * Q and all(v >= 0 for v in out)
    return out


# ----------------------------------------------------------------------------------------------- exact limb algorithms
def mul_exact(a, b):
    acc = 0
    m = [0] * NL
    r = [0] * NL
    for k in range(NL):
        for i in range(k + 1):
            acc += a[i] * b[k - i]
        for j in range(k):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        m[k] = ((acc & 0xffffffff) * NINV) & MASK
        acc += m[k] * PL[0]
        assert acc < 1 << 64 and acc & MASK == 0
        acc >>= W
    for k in range(NL, 2 * NL - 1):
        for i in range(k - NL + 1, NL):
            acc += a[i] * b[k - i]
        for j in range(k - NL + 1, NL):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        r[k - NL] = acc & MASK
        acc >>= W
    assert acc < 1 << 32
    r[NL - 1] = acc
    return r


def sqr_exact(a):
    """a * a with the cross products taken once against d = 2a (the ZKMI_MONT_SQR29_ASM schedule)."""
    d = [2 * x for x in a]
    assert all(x < 1 << 32 for x in d)
    acc = 0
    m = [0] * NL
    r = [0] * NL
    def column(k):
        s = 0
        for i in range(max(0, k - NL + 1), min(k, NL - 1) + 1):
            j = k - i
            if i < j:
                s += a[i] * d[j]
            elif i == j:
                s += a[i] * a[i]
        return s
    for k in range(NL):
        acc += column(k)
        for j in range(k):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        m[k] = ((acc & 0xffffffff) * NINV) & MASK
        acc += m[k] * PL[0]
        assert acc < 1 << 64 and acc & MASK == 0
        acc >>= W
    for k in range(NL, 2 * NL - 1):
        acc += column(k)
        for j in range(k - NL + 1, NL):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        r[k - NL] = acc & MASK
        acc >>= W
    assert acc < 1 << 32
    r[NL - 1] = acc
    return r


def mulN_exact(pairs):
    """(sum_t a_t * b_t) / 2^261 mod p, one reduction for all products (column accumulators shared)."""
    acc = 0
    m = [0] * NL
    r = [0] * NL
    for k in range(NL):
        for a, b in pairs:
            for i in range(k + 1):
                acc += a[i] * b[k - i]
        for j in range(k):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        m[k] = ((acc & 0xffffffff) * NINV) & MASK
        acc += m[k] * PL[0]
        assert acc < 1 << 64 and acc & MASK == 0
        acc >>= W
    for k in range(NL, 2 * NL - 1):
        for a, b in pairs:
            for i in range(k - NL + 1, NL):
                acc += a[i] * b[k - i]
        for j in range(k - NL + 1, NL):
            acc += m[j] * PL[k - j]
        assert acc < 1 << 64, "column overflow"
        r[k - NL] = acc & MASK
        acc >>= W
    assert acc < 1 << 32
    r[NL - 1] = acc
    return r


def add_exact(a, b):
    r = [x + y for x, y in zip(a, b)]
    assert all(v < 1 << 32 for v in r)
    return r


def sub_exact(a, b, bias):
    r = [x + z - y for x, y, z in zip(a, b, bias)]
    assert all(0 <= v < 1 << 32 for v in r), "limb underflow/overflow in sub"
    return r


def wnorm_exact(a):
    r = [a[0] & MASK] + [(a[i] & MASK) + (a[i - 1] >> W) for i in range(1, NL - 1)] + [a[NL - 1] + (a[NL - 2] >> W)]
    assert all(v < 1 << 32 for v in r)
    return r


# ----------------------------------------------------------------------------------------------- bound tracking
class B:
    """worst-case bounds of a value: vmax (integer, exclusive) and per-limb max (inclusive-ish upper bounds)"""

    def __init__(self, vmax, lmax):
        self.vmax, self.lmax = vmax, list(lmax)

    @staticmethod
    def fresh(k=1):  # loaded canonical value shifted by 5 bits (< 32 p), normalised limbs
        return B(32 * Q, [MASK] * (NL - 1) + [(32 * Q) >> (W * (NL - 1))])

    def kp(self):
        return self.vmax / Q


def b_mul(a, b):
    for k in range(2 * NL - 1):
        s = sum(a.lmax[i] * b.lmax[k - i] for i in range(NL) if 0 <= k - i < NL)
        s += NL * MASK * MASK + (1 << 36)
        assert s < 1 << 64, "possible column overflow: limbs %s x %s" % ([x.bit_length() for x in a.lmax], [x.bit_length() for x in b.lmax])
    vmax = (a.vmax * b.vmax >> RBITS) + Q + 1
    assert vmax < 1 << (RBITS - 1)
    return B(vmax, [MASK] * (NL - 1) + [vmax >> (W * (NL - 1))])


def b_mulN(pairs):
    for k in range(2 * NL - 1):
        s = 0
        for a, b in pairs:
            s += sum(a.lmax[i] * b.lmax[k - i] for i in range(NL) if 0 <= k - i < NL)
        s += NL * MASK * MASK + (1 << 36)
        assert s < 1 << 64, "possible column overflow in mulN"
    vmax = (sum(a.vmax * b.vmax for a, b in pairs) >> RBITS) + Q + 1
    assert vmax < 1 << (RBITS - 1)
    return B(vmax, [MASK] * (NL - 1) + [vmax >> (W * (NL - 1))])


def b_add(a, b):
    l = [x + y for x, y in zip(a.lmax, b.lmax)]
    assert all(v < 1 << 32 for v in l)
    assert a.vmax + b.vmax < 1 << RBITS
    return B(a.vmax + b.vmax, l)


ALLOWED_K = [4, 8, 12, 16, 24, 32, 40, 48, 64, 80, 96, 128]
SITE_K = {}   # site name -> chosen bias multiple (max over fixed-point iterations)


def pick_k(b, site):
    for k in ALLOWED_K:
        bias = bias_limbs(k)
        if b.vmax <= k * Q and all(bl <= z for bl, z in zip(b.lmax, bias)):
            k = max(k, SITE_K.get(site, 0))
            SITE_K[site] = k
            return k
    raise AssertionError("no bias large enough for %.1f p at %s" % (b.kp(), site))


def b_sub(a, b, k):
    if isinstance(k, str):
        k = pick_k(b, k)
    bias = bias_limbs(k)
    assert b.vmax <= k * Q, "bias %d p does not dominate subtrahend %.2f p" % (k, b.kp())
    assert all(bl <= z for bl, z in zip(b.lmax, bias)), "bias limb too small: %s vs %s" % (b.lmax, bias)
    l = [x + z for x, z in zip(a.lmax, bias)]
    assert all(v < 1 << 32 for v in l), "sub limb overflow"
    assert a.vmax + k * Q < 1 << RBITS
    return B(a.vmax + k * Q, l)


def b_wnorm(a):
    l = [MASK] + [MASK + (a.lmax[i - 1] >> W) for i in range(1, NL - 1)] + [min(a.lmax[NL - 1] + (a.lmax[NL - 2] >> W), (a.vmax >> (W * (NL - 1))) + 4)]
    return B(a.vmax, l)


def b_max(a, b):
    return B(max(a.vmax, b.vmax), [max(x, y) for x, y in zip(a.lmax, b.lmax)])


# ----------------------------------------------------------------------------------------------- formulas (generic over an "ops" object)
class ExactOps:
    def __init__(self):
        pass
    mul = staticmethod(mul_exact)
    mulN = staticmethod(mulN_exact)

    @staticmethod
    def reduce(a):
        return reduce_exact_p(a)

    add = staticmethod(add_exact)
    wnorm = staticmethod(wnorm_exact)

    @staticmethod
    def neg(a, k):
        if isinstance(k, str):
            k = SITE_K[k]
        return wnorm_exact(sub_exact(bias_limbs(k), a, [0] * NL))

    @staticmethod
    def sub(a, b, k):
        if isinstance(k, str):
            k = SITE_K[k]
        return sub_exact(a, b, bias_limbs(k))


class BoundOps:
    mul = staticmethod(b_mul)

    @staticmethod
    def reduce(a):  # u29p_reduce of a weakly normalised value: < 2.01 p, normalised limbs (exactness: reduce_exact_p)
        assert all(v + (1 << 11) < 1 << 32 for v in a.lmax)
        v = int(2.01 * Q)
        return B(v, [MASK] * (NL - 1) + [v >> (W * (NL - 1))])

    mulN = staticmethod(b_mulN)
    add = staticmethod(b_add)

    @staticmethod
    def neg(a, k):
        if isinstance(k, str):
            k = pick_k(a, k)
        bias = bias_limbs(k)
        assert a.vmax <= k * Q and all(al <= z for al, z in zip(a.lmax, bias))
        return b_wnorm(B(k * Q + 1, bias))

    sub = staticmethod(b_sub)
    wnorm = staticmethod(b_wnorm)


def madd_fp(O, X1, Y1, ZZ1, ZZZ1, X2, Y2):
    """XYZZ += affine (madd-2008-s), generic case.  Output (X3, Y3, ZZ3, ZZZ3) weakly normalised.  Site names index the
    bias multiple of each subtraction (SITE_K, filled by the bound propagation, hard-coded in ff29.hpp)."""
    U2 = O.mul(X2, ZZ1)
    S2 = O.mul(Y2, ZZZ1)
    P = O.wnorm(O.sub(U2, X1, "g1.P"))
    R = O.wnorm(O.sub(S2, Y1, "g1.R"))
    PP = O.mul(P, P)
    PPP = O.mul(P, PP)
    Qv = O.mul(X1, PP)
    t = O.mul(R, R)
    t = O.wnorm(O.sub(t, PPP, "g1.m"))
    t = O.sub(t, Qv, "g1.m")
    t = O.sub(t, Qv, "g1.m")
    X3 = O.wnorm(t)
    d = O.wnorm(O.sub(Qv, X3, "g1.QX"))
    Y3 = O.mulN([(R, d), (O.neg(Y1, "g1.nY"), PPP)])   # R d - Y1 PPP under ONE reduction: a direct product output
    ZZ3 = O.mul(ZZ1, PP)
    ZZZ3 = O.mul(ZZZ1, PPP)
    return X3, Y3, ZZ3, ZZZ3


def madd_fp_second(O, X1, Y1, X2, Y2):
    """The SECOND point of a task: the accumulator is still affine (ZZ1 = ZZZ1 = "one", X1 / Y1 the contracted first point), so U2 = X2, S2 = Y2,
    ZZ3 = PP and ZZZ3 = PPP -- four products less.  X2 / Y2 (fresh loads, < 32 p) are partially reduced instead (u29p_reduce, < 2.01 p), which keeps every
    value inside the envelope of the generic madd; the biases are those of the generic sites except P's (4 p: X1 < 1.2 p here).
    Measured on the GPU and NOT in the kernel (1.4 % fewer products, 3 registers more, no gain); kept here as the record of its bounds."""
    U2 = O.reduce(X2)
    S2 = O.reduce(Y2)
    P = O.wnorm(O.sub(U2, X1, 4))
    R = O.wnorm(O.sub(S2, Y1, "g1.R"))
    PP = O.mul(P, P)
    PPP = O.mul(P, PP)
    Qv = O.mul(X1, PP)
    t = O.mul(R, R)
    t = O.wnorm(O.sub(t, PPP, "g1.m"))
    t = O.sub(t, Qv, "g1.m")
    t = O.sub(t, Qv, "g1.m")
    X3 = O.wnorm(t)
    d = O.wnorm(O.sub(Qv, X3, "g1.QX"))
    Y3 = O.mulN([(R, d), (O.neg(Y1, "g1.nY"), PPP)])
    return X3, Y3, PP, PPP


def add_fp(O, A, Bp):
    """XYZZ + XYZZ (add-2008-s) on lazily reduced coordinates; both inputs anywhere in the class "every coordinate < 32 p"."""
    X1, Y1, ZZ1, ZZZ1 = A
    X2, Y2, ZZ2, ZZZ2 = Bp
    U1 = O.mul(X1, ZZ2)
    U2 = O.mul(X2, ZZ1)
    S1 = O.mul(Y1, ZZZ2)
    S2 = O.mul(Y2, ZZZ1)
    P = O.wnorm(O.sub(U2, U1, "g1a.8"))
    R = O.wnorm(O.sub(S2, S1, "g1a.8"))
    PP = O.mul(P, P)
    PPP = O.mul(P, PP)
    Qv = O.mul(U1, PP)
    t = O.mul(R, R)
    t = O.wnorm(O.sub(t, PPP, "g1a.4"))
    t = O.sub(t, Qv, "g1a.4")
    t = O.sub(t, Qv, "g1a.4")
    X3 = O.wnorm(t)
    d = O.wnorm(O.sub(Qv, X3, "g1a.16"))
    Y3 = O.mulN([(R, d), (O.neg(S1, "g1a.nS"), PPP)])
    ZZ3 = O.mul(O.mul(ZZ1, ZZ2), PP)
    ZZZ3 = O.mul(O.mul(ZZZ1, ZZZ2), PPP)
    return X3, Y3, ZZ3, ZZZ3


def dbl_fp(O, A):
    """2 * XYZZ (dbl-2008-s-1)"""
    X1, Y1, ZZ1, ZZZ1 = A
    U = O.add(Y1, Y1)
    V = O.mul(U, U)
    Wv = O.mul(U, V)
    S = O.mul(X1, V)
    X2 = O.mul(X1, X1)
    M = O.wnorm(O.add(O.add(X2, X2), X2))
    t = O.mul(M, M)
    t = O.sub(t, S, "g1d.8")
    X3 = O.wnorm(O.sub(t, S, "g1d.8"))
    d = O.wnorm(O.sub(S, X3, "g1d.24"))
    Y3 = O.mulN([(M, d), (O.neg(Wv, "g1d.nW"), Y1)])
    ZZ3 = O.mul(V, ZZ1)
    ZZZ3 = O.mul(Wv, ZZZ1)
    return X3, Y3, ZZ3, ZZZ3


def check_add_dbl_class():
    """the class "all four coordinates < 32 p, weakly normalised" is closed under load, madd, add and dbl"""
    cls = B(32 * Q, [MASK + 8] * (NL - 1) + [((32 * Q) >> (W * (NL - 1))) + 4])
    A = (cls, cls, cls, cls)
    for name, out in (("add", add_fp(BoundOps, A, A)), ("dbl", dbl_fp(BoundOps, A))):
        for c in out:
            assert c.vmax <= 32 * Q, (name, c.kp())
            assert all(l <= MASK + 8 for l in c.lmax[:-1]), name
        print("  %s: outputs (units of p): %s" % (name, ", ".join("%.1f" % c.kp() for c in out)))


def exact_check_add_dbl(n=40):
    random.seed(3)
    def on_curve_point():
        while True:
            x = rand_fe()
            rhs = (x * x * x + 3) % Q
            y = pow(rhs, (Q + 1) // 4, Q)
            if y * y % Q == rhs:
                return x, y
    def aff_add(P1, P2):
        if P1 == P2:
            lam = 3 * P1[0] * P1[0] * pow(2 * P1[1], -1, Q) % Q
        else:
            lam = (P2[1] - P1[1]) * pow(P2[0] - P1[0], -1, Q) % Q
        x3 = (lam * lam - P1[0] - P2[0]) % Q
        return x3, (lam * (P1[0] - x3) - P1[1]) % Q
    def lift(Pt):
        z = rand_fe()
        zz, zzz = z * z % Q, z * z * z % Q
        return tuple(to_u29(v) for v in (Pt[0] * zz % Q, Pt[1] * zzz % Q, zz, zzz))
    def aff(A):
        x, y, zz, zzz = (from_u29(v) for v in A)
        return x * pow(zz, -1, Q) % Q, y * pow(zzz, -1, Q) % Q
    P1, acc = on_curve_point(), None
    A = lift(P1)
    accp = P1
    for i in range(n):
        if i % 3 == 2:
            A = dbl_fp(ExactOps, A)
            accp = aff_add(accp, accp)
        else:
            P2 = on_curve_point()
            A = add_fp(ExactOps, A, lift(P2))
            accp = aff_add(accp, P2)
        assert aff(A) == accp
    print("  exact G1 add/dbl chain of %d operations: ok" % n)


# Fp2 helpers: values are pairs
def f2_mul(O, a, b):
    v0 = O.mul(a[0], b[0])
    v1 = O.mul(a[1], b[1])
    s = O.mul(O.add(a[0], a[1]), O.add(b[0], b[1]))
    c0 = O.wnorm(O.sub(v0, v1, "g2.m"))
    c1 = O.wnorm(O.sub(O.sub(s, v0, "g2.m"), v1, "g2.m"))
    return (c0, c1)


def f2_sqr(O, a, site):
    # (a0+a1)(a0-a1), 2 a0 a1
    d = O.wnorm(O.sub(a[0], a[1], site))
    s = O.add(a[0], a[1])
    c0 = O.mul(s, d)
    m = O.mul(a[0], a[1])
    return (c0, O.add(m, m))


def f2_sub(O, a, b, site):
    return (O.wnorm(O.sub(a[0], b[0], site)), O.wnorm(O.sub(a[1], b[1], site)))


def f2_contract(O, a, one):
    """multiply both components by the domain's one: same residues, values back below ~1.3 p"""
    return (O.mul(a[0], one), O.mul(a[1], one))


def madd_fp2(O, X1, Y1, ZZ1, ZZZ1, X2, Y2, one=None):
    """G2 madd: Karatsuba Fp2 products; X3 and Y3 are contracted (multiplied by one) so that the lazily reduced bounds close."""
    if one is None:
        one = B((1 << RBITS) % Q + 1, limbs((1 << RBITS) % Q)) if O is BoundOps else limbs((1 << RBITS) % Q)
    U2 = f2_mul(O, X2, ZZ1)
    S2 = f2_mul(O, Y2, ZZZ1)
    P = f2_sub(O, U2, X1, "g2.P")
    R = f2_sub(O, S2, Y1, "g2.R")
    PP = f2_sqr(O, P, "g2.sqP")
    PPP = f2_mul(O, P, PP)
    Qv = f2_mul(O, X1, PP)
    RR = f2_sqr(O, R, "g2.sqR")
    t = f2_sub(O, RR, PPP, "g2.x")
    t = f2_sub(O, t, Qv, "g2.x")
    X3 = f2_contract(O, f2_sub(O, t, Qv, "g2.x"), one)
    d = f2_sub(O, Qv, X3, "g2.QX")
    Y3 = f2_contract(O, f2_sub(O, f2_mul(O, R, d), f2_mul(O, Y1, PPP), "g2.x"), one)
    ZZ3 = f2_mul(O, ZZ1, PP)
    ZZZ3 = f2_mul(O, ZZZ1, PPP)
    return X3, Y3, ZZ3, ZZZ3


def f2_mulF(O, a, b, na1=None, site="g2f.n"):
    """Fp2 product with ONE Montgomery reduction per component: c0 = a0 b0 + (-a1) b1, c1 = a0 b1 + a1 b0."""
    if na1 is None:
        na1 = O.neg(a[1], site)
    return (O.mulN([(a[0], b[0]), (na1, b[1])]), O.mulN([(a[0], b[1]), (a[1], b[0])]))


def madd_fp2_fused(O, X1, Y1, ZZ1, ZZZ1, X2, Y2, nX2=None, nY2=None):
    """G2 madd with fused multi-product reductions: every stored coordinate is a direct product output (< ~3 p), so no
    contraction multiplications are needed.  X3 = R^2 - (P + 2 X1) PP,  Y3 = R (Q - X3) - Y1 PPP.
    nX2 / nY2: the negated second components of the point, where the caller has them already (window-table rows)."""
    U2 = f2_mulF(O, X2, ZZ1, nX2, site="g2f.nfresh")
    S2 = f2_mulF(O, Y2, ZZZ1, nY2, site="g2f.nfresh")
    P = f2_sub(O, U2, X1, "g2f.P")
    R = f2_sub(O, S2, Y1, "g2f.P")
    nP1 = O.neg(P[1], "g2f.n")
    nR1 = O.neg(R[1], "g2f.n")
    # PP = P^2 = ((P0 + P1)(P0 - P1), 2 P0 P1): complex squaring, two products
    PP = (O.mul(O.add(P[0], P[1]), O.wnorm(O.sub(P[0], P[1], "g2f.sq"))), O.mul(O.add(P[0], P[0]), P[1]))
    PPP = f2_mulF(O, P, PP, nP1)
    nX1 = O.neg(X1[1], "g2f.n")
    Qv = f2_mulF(O, X1, PP, nX1)
    # W = P + 2 X1 ; X3 = R^2 - W PP
    Wv = (O.wnorm(O.add(P[0], O.add(X1[0], X1[0]))), O.wnorm(O.add(P[1], O.add(X1[1], X1[1]))))
    nW0, nW1 = O.neg(Wv[0], "g2f.nW"), O.neg(Wv[1], "g2f.nW")
    X3 = (O.mulN([(O.add(R[0], R[1]), O.wnorm(O.sub(R[0], R[1], "g2f.sq"))), (nW0, PP[0]), (Wv[1], PP[1])]),
          O.mulN([(O.add(R[0], R[0]), R[1]), (nW0, PP[1]), (nW1, PP[0])]))
    d = f2_sub(O, Qv, X3, "g2f.P")
    nY0, nY1 = O.neg(Y1[0], "g2f.n"), O.neg(Y1[1], "g2f.n")
    Y3 = (O.mulN([(R[0], d[0]), (nR1, d[1]), (nY0, PPP[0]), (Y1[1], PPP[1])]),
          O.mulN([(R[0], d[1]), (R[1], d[0]), (nY0, PPP[1]), (nY1, PPP[0])]))
    nZ1 = O.neg(ZZ1[1], "g2f.n")
    ZZ3 = f2_mulF(O, ZZ1, PP, nZ1)
    nZZ1 = O.neg(ZZZ1[1], "g2f.n")
    ZZZ3 = f2_mulF(O, ZZZ1, PPP, nZZ1)
    return X3, Y3, ZZ3, ZZZ3


# ---- G2 bucket-reduction tail: XYZZ + XYZZ and doubling over Fp2 in fused form (every output coordinate a direct product output)
def add_fp2(O, A, Bp):
    X1, Y1, ZZ1, ZZZ1 = A
    X2, Y2, ZZ2, ZZZ2 = Bp
    U1 = f2_mulF(O, X1, ZZ2, site="g2a.nin")
    U2 = f2_mulF(O, X2, ZZ1, site="g2a.nin")
    S1 = f2_mulF(O, Y1, ZZZ2, site="g2a.nin")
    S2 = f2_mulF(O, Y2, ZZZ1, site="g2a.nin")
    P = f2_sub(O, U2, U1, "g2a.P")
    R = f2_sub(O, S2, S1, "g2a.P")
    nP1, nR1 = O.neg(P[1], "g2a.nP"), O.neg(R[1], "g2a.nP")
    PP = (O.mulN([(P[0], P[0]), (nP1, P[1])]), O.mul(O.add(P[0], P[0]), P[1]))
    PPP = f2_mulF(O, P, PP, nP1)
    Qv = f2_mulF(O, U1, PP, site="g2a.nU")
    Wv = (O.wnorm(O.add(P[0], O.add(U1[0], U1[0]))), O.wnorm(O.add(P[1], O.add(U1[1], U1[1]))))
    nW0, nW1 = O.neg(Wv[0], "g2a.nW"), O.neg(Wv[1], "g2a.nW")
    X3 = (O.mulN([(R[0], R[0]), (nR1, R[1]), (nW0, PP[0]), (Wv[1], PP[1])]),
          O.mulN([(O.add(R[0], R[0]), R[1]), (nW0, PP[1]), (nW1, PP[0])]))
    d = f2_sub(O, Qv, X3, "g2a.d")
    nS0, nS1 = O.neg(S1[0], "g2a.nU"), O.neg(S1[1], "g2a.nU")
    Y3 = (O.mulN([(R[0], d[0]), (nR1, d[1]), (nS0, PPP[0]), (S1[1], PPP[1])]),
          O.mulN([(R[0], d[1]), (R[1], d[0]), (nS0, PPP[1]), (nS1, PPP[0])]))
    ZZ = f2_mulF(O, ZZ1, ZZ2, site="g2a.nin")
    ZZ3 = f2_mulF(O, ZZ, PP, site="g2a.nU")
    ZZZ = f2_mulF(O, ZZZ1, ZZZ2, site="g2a.nin")
    ZZZ3 = f2_mulF(O, ZZZ, PPP, site="g2a.nU")
    return X3, Y3, ZZ3, ZZZ3, PP


def dbl_fp2(O, A, one=None):
    X1, Y1, ZZ1, ZZZ1 = A
    if one is None:
        one = B((1 << RBITS) % Q + 1, limbs((1 << RBITS) % Q)) if O is BoundOps else limbs((1 << RBITS) % Q)
    Yc = (O.mul(Y1[0], one), O.mul(Y1[1], one))          # contracted: keeps U = 2 Y small
    U = (O.wnorm(O.add(Yc[0], Yc[0])), O.wnorm(O.add(Yc[1], Yc[1])))
    nU1 = O.neg(U[1], "g2d.nU")
    V = (O.mulN([(U[0], U[0]), (nU1, U[1])]), O.mul(O.add(U[0], U[0]), U[1]))
    Wv = f2_mulF(O, U, V, nU1)
    S = f2_mulF(O, X1, V, site="g2d.nin")
    nX1 = O.neg(X1[1], "g2d.nin")
    X2 = (O.mulN([(X1[0], X1[0]), (nX1, X1[1])]), O.mul(O.add(X1[0], X1[0]), X1[1]))
    M = (O.wnorm(O.add(O.add(X2[0], X2[0]), X2[0])), O.wnorm(O.add(O.add(X2[1], X2[1]), X2[1])))
    nM1 = O.neg(M[1], "g2d.nM")
    tX0, tX1 = O.wnorm(O.add(X1[0], X1[0])), O.wnorm(O.add(X1[1], X1[1]))
    n2X0, n2X1 = O.neg(tX0, "g2d.n2X"), O.neg(tX1, "g2d.n2X")
    # X3 = M^2 - 2 X1 V, one reduction per component
    X3 = (O.mulN([(M[0], M[0]), (nM1, M[1]), (n2X0, V[0]), (tX1, V[1])]),
          O.mulN([(O.add(M[0], M[0]), M[1]), (n2X0, V[1]), (n2X1, V[0])]))
    d = f2_sub(O, S, X3, "g2d.d")
    nW0, nW1 = O.neg(Wv[0], "g2d.nW"), O.neg(Wv[1], "g2d.nW")
    # Y3 = M (S - X3) - W Y1
    Y3 = (O.mulN([(M[0], d[0]), (nM1, d[1]), (nW0, Y1[0]), (Wv[1], Y1[1])]),
          O.mulN([(M[0], d[1]), (M[1], d[0]), (nW0, Y1[1]), (nW1, Y1[0])]))
    ZZ3 = f2_mulF(O, V, ZZ1, site="g2d.nW")
    ZZZ3 = f2_mulF(O, Wv, ZZZ1, nW1)
    return X3, Y3, ZZ3, ZZZ3


def check_add_dbl_class_g2():
    """the class "both components of all four coordinates < 32 p, weakly normalised" is closed under load, add and dbl (G2)"""
    c1 = B(32 * Q, [MASK + 8] * (NL - 1) + [((32 * Q) >> (W * (NL - 1))) + 4])
    cls = (c1, c1)
    A = (cls, cls, cls, cls)
    for name, out in (("add", add_fp2(BoundOps, A, A)[:4]), ("dbl", dbl_fp2(BoundOps, A))):
        for c in out:
            for comp in c:
                assert comp.vmax <= 32 * Q, (name, comp.kp())
                assert all(l <= MASK + 8 for l in comp.lmax[:-1]), name
        print("  G2 %s: outputs (units of p): %s" % (name, ", ".join("%.1f/%.1f" % (c[0].kp(), c[1].kp()) for c in out)))


def exact_check_add_dbl_g2(n=30):
    random.seed(17)
    f2m = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
    f2s = lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
    def f2inv(a):
        dd = pow((a[0] * a[0] + a[1] * a[1]) % Q, -1, Q)
        return (a[0] * dd % Q, -a[1] * dd % Q)
    # the chord / tangent rules are algebraic identities: random pairs need not lie on the twist (tangent uses a = 0: lam = 3 x^2 / 2 y)
    def chord(P1, P2):
        lam = f2m(f2s(P2[1], P1[1]), f2inv(f2s(P2[0], P1[0])))
        x3 = f2s(f2s(f2m(lam, lam), P1[0]), P2[0])
        return x3, f2s(f2m(lam, f2s(P1[0], x3)), P1[1])
    def tangent(P1):
        x2 = f2m(P1[0], P1[0])
        lam = f2m(((3 * x2[0]) % Q, (3 * x2[1]) % Q), f2inv(((2 * P1[1][0]) % Q, (2 * P1[1][1]) % Q)))
        x3 = f2s(f2s(f2m(lam, lam), P1[0]), P1[0])
        return x3, f2s(f2m(lam, f2s(P1[0], x3)), P1[1])
    rp = lambda: ((rand_fe(), rand_fe()), (rand_fe(), rand_fe()))
    def lift(Pt):
        z = (rand_fe(), rand_fe())
        zz = f2m(z, z)
        zzz = f2m(zz, z)
        u = lambda v: (to_u29(v[0]), to_u29(v[1]))
        return (u(f2m(Pt[0], zz)), u(f2m(Pt[1], zzz)), u(zz), u(zzz))
    def aff(A):
        g = lambda v: (from_u29(v[0]), from_u29(v[1]))
        return f2m(g(A[0]), f2inv(g(A[2]))), f2m(g(A[1]), f2inv(g(A[3])))
    accp = rp()
    A = lift(accp)
    for i in range(n):
        if i % 3 == 2:
            A = dbl_fp2(ExactOps, A)
            accp = tangent(accp)
        else:
            P2 = rp()
            A = add_fp2(ExactOps, A, lift(P2))[:4]
            accp = chord(accp, P2)
        assert aff(A) == accp, i
    print("  exact G2 add/dbl chain of %d operations: ok" % n)


def fixed_point(madd, is_f2):
    fresh = B.fresh()
    one = B(2 * Q, [MASK] * (NL - 1) + [(2 * Q) >> (W * (NL - 1))])
    mk = (lambda b: (b, b)) if is_f2 else (lambda b: b)
    # the first point of a task becomes the accumulator after one contracting multiplication by "one" (2^261 mod p)
    X1, Y1, ZZ1, ZZZ1 = mk(one), mk(one), mk(one), mk(one)
    X2, Y2 = mk(fresh), mk(fresh)
    for it in range(12):
        X3, Y3, ZZ3, ZZZ3 = madd(BoundOps, X1, Y1, ZZ1, ZZZ1, X2, Y2)
        j = (lambda a, b: (b_max(a[0], b[0]), b_max(a[1], b[1]))) if is_f2 else b_max
        nX, nY, nZ, nZZ = j(X1, X3), j(Y1, Y3), j(ZZ1, ZZ3), j(ZZZ1, ZZZ3)
        X1, Y1, ZZ1, ZZZ1 = nX, nY, nZ, nZZ
    g = (lambda b: max(b[0].kp(), b[1].kp())) if is_f2 else (lambda b: b.kp())
    print("  fixed point bounds (units of p): X %.1f  Y %.1f  ZZ %.2f  ZZZ %.2f" % (g(X1), g(Y1), g(ZZ1), g(ZZZ1)))
    return X1, Y1, ZZ1, ZZZ1


def rand_fe():
    return random.randrange(Q)


def to_u29(x):  # canonical field element x -> Mont-256 image -> shifted by 5 -> limbs (what the kernel's load does)
    v = (x << 256) % Q
    return limbs(v << 5)


def from_u29(l):
    return val(l) * pow(1 << RBITS, -1, Q) % Q


def ec_madd_affine(P1, P2):
    x1, y1 = P1
    x2, y2 = P2
    lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return x3, (lam * (x1 - x3) - y1) % Q


def exact_check(n=300):
    random.seed(7)
    # G1: start from an affine point, add n random-ish points (not necessarily on the curve: madd formulas are generic
    # chord additions and the identity x/zz, y/zzz is checked against the affine chord rule on y^2 = x^3 + b for the
    # family of curves through the points -- so use real curve points instead)
    def on_curve_point():
        while True:
            x = rand_fe()
            rhs = (x * x * x + 3) % Q
            y = pow(rhs, (Q + 1) // 4, Q)
            if y * y % Q == rhs:
                return x, y
    P0 = on_curve_point()
    one = to_u29(1)
    one = mul_exact(one, limbs((1 << RBITS) % Q))  # canonical "one" of the radix-2^261 domain
    X, Y = mul_exact(to_u29(P0[0]), one), mul_exact(to_u29(P0[1]), one)
    ZZ, ZZZ = list(one), list(one)
    acc = P0
    for it in range(n):
        P2 = on_curve_point()
        if it == 0:   # the second point of the task: the shorter formula
            X, Y, ZZ, ZZZ = madd_fp_second(ExactOps, X, Y, to_u29(P2[0]), to_u29(P2[1]))
        else:
            X, Y, ZZ, ZZZ = madd_fp(ExactOps, X, Y, ZZ, ZZZ, to_u29(P2[0]), to_u29(P2[1]))
        acc = ec_madd_affine(acc, P2)
        x = from_u29(X) * pow(from_u29(ZZ), -1, Q) % Q
        y = from_u29(Y) * pow(from_u29(ZZZ), -1, Q) % Q
        assert (x, y) == acc
    print("  exact G1 simulation of %d chained madds: ok" % n)


def exact_check_g2(n=60, madd=None):
    madd = madd or madd_fp2
    random.seed(11)
    nonres = Q - 1  # u^2 = -1

    def f2m(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
    def f2inv(a):
        d = pow((a[0] * a[0] + a[1] * a[1]) % Q, -1, Q)
        return (a[0] * d % Q, -a[1] * d % Q)
    def f2s(a, b): return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
    # random affine "points" need not lie on the twist for the chord rule identity x3 = lam^2 - x1 - x2, y3 = lam (x1 - x3) - y1
    def chord(P1, P2):
        lam = f2m(f2s(P2[1], P1[1]), f2inv(f2s(P2[0], P1[0])))
        x3 = f2s(f2s(f2m(lam, lam), P1[0]), P2[0])
        return x3, f2s(f2m(lam, f2s(P1[0], x3)), P1[1])
    rp = lambda: ((rand_fe(), rand_fe()), (rand_fe(), rand_fe()))
    one = mul_exact(to_u29(1), limbs((1 << RBITS) % Q))
    zero = [0] * NL
    P0 = rp()
    X = (mul_exact(to_u29(P0[0][0]), one), mul_exact(to_u29(P0[0][1]), one))
    Y = (mul_exact(to_u29(P0[1][0]), one), mul_exact(to_u29(P0[1][1]), one))
    ZZ, ZZZ = (list(one), list(zero)), (list(one), list(zero))
    acc = P0
    for _ in range(n):
        P2 = rp()
        X, Y, ZZ, ZZZ = madd(ExactOps, X, Y, ZZ, ZZZ, (to_u29(P2[0][0]), to_u29(P2[0][1])), (to_u29(P2[1][0]), to_u29(P2[1][1])))
        acc = chord(acc, P2)
        g = lambda v: (from_u29(v[0]), from_u29(v[1]))
        x = f2m(g(X), f2inv(g(ZZ)))
        y = f2m(g(Y), f2inv(g(ZZZ)))
        assert (x, y) == acc
    print("  exact G2 simulation of %d chained madds: ok" % n)


# ----------------------------------------------------------------------------------------------- native window-table rows
# A window-table coordinate is kept in the accumulate kernel's own domain: x * 2^261 mod p, canonical (< p), packed into 8 words of 32 bits (a G1 entry: x
# then y, 16 words; a G2 entry: x.a0, x.a1, y.a0, y.a1, 32 words); the kernel unpacks it into 9 limbs below 2^29 (top limb below 2^22).  p < 2^254: bit 31 of
# the top word of y (G2: of y.a0) says "this entry is a point", so that a zeroed entry is the point at infinity.
# The kernel applies the digit's sign in limb form, y -> BIAS4 - y (no carries, NOT normalised: every product schedule takes limbs < 2^32), and the first
# point of a task is copied into the accumulator (negated: BIAS2 - y, weakly normalised: it is subtracted from, so it has to stay below the 4 p of site g1.R).
TAB_VALID = 1 << 31
TAB_SIGN_K, TAB_FIRST_K = 4, 2


def tab_limbs(x):
    return limbs((x << RBITS) % Q)


def tab_encode(coords):
    """coords: the canonical field elements of an entry (G1: x, y; G2: x0, x1, y0, y1); None: the point at infinity.  -> 8 words of 32 bits per coordinate"""
    if coords is None:
        return None
    out = [[(val(tab_limbs(c)) >> (32 * i)) & 0xffffffff for i in range(8)] for c in coords]
    out[len(coords) // 2][7] |= TAB_VALID
    return [w for c in out for w in c]


def tab_decode(words):
    """-> the limb vectors of the coordinates as the kernel unpacks them (u29_unpack; the flag masked off the top limb), or None for the point at infinity"""
    nc = len(words) // 8
    if not words[8 * (nc // 2) + 7] & TAB_VALID:
        return None
    out = []
    for k in range(nc):
        l = limbs(sum(w << (32 * i) for i, w in enumerate(words[8 * k:8 * k + 8])))
        l[NL - 1] &= (1 << 22) - 1
        out.append(l)
    return out


def tab_sign_exact(y, neg):
    return [b - v for b, v in zip(bias_limbs(TAB_SIGN_K), y)] if neg else list(y)


def tab_first_exact(y, neg):
    return wnorm_exact([b - v for b, v in zip(bias_limbs(TAB_FIRST_K), y)]) if neg else list(y)


def b_tab():
    return B(Q, [MASK] * (NL - 1) + [(Q - 1) >> (W * (NL - 1))])


def b_tab_signed():  # y or BIAS4 - y, as the kernel selects them
    return b_max(b_tab(), B(TAB_SIGN_K * Q + 1, bias_limbs(TAB_SIGN_K)))


def b_tab_first():   # y or wnorm(BIAS2 - y): the accumulator's Y after the first point
    return b_max(b_tab(), b_wnorm(B(TAB_FIRST_K * Q + 1, bias_limbs(TAB_FIRST_K))))


def fixed_point_table(is_f2):
    """The accumulate loop over window-table rows: first point copied, every later one through the generic madd with X2 < p normalised and Y2 sign-applied in
    limb form.  Must close with the biases the table-less loop already chose (the two variants share the formula's code)."""
    before = dict(SITE_K)
    one = B(2 * Q, [MASK] * (NL - 1) + [(2 * Q) >> (W * (NL - 1))])
    mk = (lambda b: (b, b)) if is_f2 else (lambda b: b)
    j = (lambda a, b: (b_max(a[0], b[0]), b_max(a[1], b[1]))) if is_f2 else b_max
    X1, Y1, ZZ1, ZZZ1 = mk(b_tab()), mk(b_tab_first()), mk(one), mk(one)
    X2, Y2 = mk(b_tab()), mk(b_tab_signed())
    for it in range(12):
        if is_f2:
            X3, Y3, ZZ3, ZZZ3 = madd_fp2_fused(BoundOps, X1, Y1, ZZ1, ZZZ1, X2, Y2, b_tab_signed(), b_tab_signed())
        else:
            X3, Y3, ZZ3, ZZZ3 = madd_fp(BoundOps, X1, Y1, ZZ1, ZZZ1, X2, Y2)
        X1, Y1, ZZ1, ZZZ1 = j(X1, X3), j(Y1, Y3), j(ZZ1, ZZ3), j(ZZZ1, ZZZ3)
    assert SITE_K == before, "window-table rows need larger biases: %s vs %s" % (SITE_K, before)
    g = (lambda b: max(b[0].kp(), b[1].kp())) if is_f2 else (lambda b: b.kp())
    lm = (lambda b: max(max(b[0].lmax), max(b[1].lmax))) if is_f2 else (lambda b: max(b.lmax))
    assert all(lm(v) < 1 << 32 for v in (X1, Y1, ZZ1, ZZZ1))
    print("  window-table rows, fixed point bounds (units of p): X %.1f  Y %.1f  ZZ %.2f  ZZZ %.2f, same biases" % (g(X1), g(Y1), g(ZZ1), g(ZZZ1)))
    return X1, Y1, ZZ1, ZZZ1


def exact_check_table(n=300):
    """chained madds from encoded window-table rows with random signs, against the affine chord rule (G1: curve points; G2: the generic identity)"""
    random.seed(29)
    def on_curve_point():
        while True:
            x = rand_fe()
            rhs = (x * x * x + 3) % Q
            y = pow(rhs, (Q + 1) // 4, Q)
            if y * y % Q == rhs:
                return x, y
    one = limbs((1 << RBITS) % Q)
    acc = None
    for it in range(n):
        P2 = on_curve_point()
        neg = random.random() < 0.5
        x2, y2 = tab_decode(tab_encode(P2))
        assert val(x2) == (P2[0] << RBITS) % Q and val(y2) == (P2[1] << RBITS) % Q
        S2 = (P2[0], (Q - P2[1]) % Q) if neg else P2
        if acc is None:
            X, Y, ZZ, ZZZ = x2, tab_first_exact(y2, neg), list(one), list(one)
            acc = S2
        else:
            X, Y, ZZ, ZZZ = madd_fp(ExactOps, X, Y, ZZ, ZZZ, x2, tab_sign_exact(y2, neg))
            acc = ec_madd_affine(acc, S2)
        assert (from_u29(X) * pow(from_u29(ZZ), -1, Q) % Q, from_u29(Y) * pow(from_u29(ZZZ), -1, Q) % Q) == acc
    print("  exact G1 simulation of %d chained madds from window-table rows: ok" % n)
    f2m = lambda a, b: ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
    f2s = lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)
    def f2inv(a):
        d = pow((a[0] * a[0] + a[1] * a[1]) % Q, -1, Q)
        return (a[0] * d % Q, -a[1] * d % Q)
    def chord(P1, P2):
        lam = f2m(f2s(P2[1], P1[1]), f2inv(f2s(P2[0], P1[0])))
        x3 = f2s(f2s(f2m(lam, lam), P1[0]), P2[0])
        return x3, f2s(f2m(lam, f2s(P1[0], x3)), P1[1])
    zero = [0] * NL
    acc = None
    for it in range(n // 5):
        P2 = ((rand_fe(), rand_fe()), (rand_fe(), rand_fe()))
        neg = random.random() < 0.5
        x0, x1, y0, y1 = tab_decode(tab_encode((P2[0][0], P2[0][1], P2[1][0], P2[1][1])))
        S2 = (P2[0], ((Q - P2[1][0]) % Q, (Q - P2[1][1]) % Q)) if neg else P2
        if acc is None:
            X, Y = (x0, x1), (tab_first_exact(y0, neg), tab_first_exact(y1, neg))
            ZZ, ZZZ = (list(one), list(zero)), (list(one), list(zero))
            acc = S2
        else:
            X, Y, ZZ, ZZZ = madd_fp2_fused(ExactOps, X, Y, ZZ, ZZZ, (x0, x1), (tab_sign_exact(y0, neg), tab_sign_exact(y1, neg)),
                                           tab_sign_exact(x1, True), tab_sign_exact(y1, not neg))
            acc = chord(acc, S2)
        g = lambda v: (from_u29(v[0]), from_u29(v[1]))
        assert (f2m(g(X), f2inv(g(ZZ))), f2m(g(Y), f2inv(g(ZZZ)))) == acc
    print("  exact G2 simulation of %d chained madds from window-table rows: ok" % (n // 5))


def check_table_rows():
    print("window-table rows (x * 2^261 mod p, packed), G1:")
    fixed_point_table(False)
    print("window-table rows (x * 2^261 mod p, packed), G2 fused:")
    fixed_point_table(True)
    exact_check_table()


RC_P = limbs((1 << RBITS) - Q)
QM_P = (1 << 53) // ((Q >> (W * (NL - 1))) + 1)


def reduce_exact_p(x):
    """x -= q p with q = mul_hi(top limb, QM_P) >> 21 (u29p_reduce): < 2.01 p, limbs 0..7 < 2^29"""
    q = ((x[NL - 1] * QM_P) >> 32) >> 21
    c, out = 0, [0] * NL
    for i in range(NL):
        assert x[i] + c < 1 << 32
        acc = q * RC_P[i] + x[i] + c
        assert acc < 1 << 64
        if i < NL - 1:
            out[i], c = acc & MASK, acc >> W
        else:
            out[i] = acc - (q << W)
            assert 0 <= out[i] < 1 << 32
    assert val(out) == val(x) - q * Q and val(out) < 2.01 * Q
    return out


def exact_check_interchange(n=5000):
    """G1 interchange format: pack(reduce(x)) made canonical == x mod p, and unpacking it gives limbs of a value < p"""
    random.seed(23)
    for _ in range(n):
        v = random.randrange(random.choice([1, 3, 14, 32, 200]) * Q)
        x = limbs(v)
        for i in range(NL - 1):
            if x[i + 1] > 0 and random.random() < 0.3:
                x[i] += 1 << W
                x[i + 1] -= 1
        y = val(reduce_exact_p(x))
        assert y < 1 << 256
        for _k in range(2):
            if y >= Q:
                y -= Q
        assert y == v % Q
    print("  G1 interchange format (partial reduction + pack): exact on %d samples" % n)


def main():
    print("p limbs (29-bit):", ", ".join("0x%08x" % v for v in PL))
    print("ninv29 = 0x%08x" % NINV)
    print("G1 (Fp) madd bound propagation:")
    # the second point of a task through the shorter formula: its outputs must lie inside the generic fixed point (they feed generic madds)
    fx, fy, fzz, fzzz = fixed_point(madd_fp, False)
    one = B(2 * Q, [MASK] * (NL - 1) + [(2 * Q) >> (W * (NL - 1))])
    sx, sy, szz, szzz = madd_fp_second(BoundOps, one, one, B.fresh(), B.fresh())
    # its outputs feed generic madds: propagate from them with the biases already chosen -- no subtraction site may need a larger multiple of p
    before = dict(SITE_K)
    gx, gy, gzz, gzzz = madd_fp(BoundOps, sx, sy, szz, szzz, B.fresh(), B.fresh())
    for _ in range(12):
        gx, gy, gzz, gzzz = madd_fp(BoundOps, b_max(gx, sx), b_max(gy, sy), b_max(gzz, szz), b_max(gzzz, szzz), B.fresh(), B.fresh())
    assert SITE_K == before, "the second-point formula needs larger biases: %s vs %s" % (SITE_K, before)
    print("  second-point formula: X %.2f  Y %.2f  ZZ %.2f  ZZZ %.2f p; generic madds after it: X %.2f  Y %.2f  ZZ %.2f  ZZZ %.2f p, same biases"
          % (sx.kp(), sy.kp(), szz.kp(), szzz.kp(), gx.kp(), gy.kp(), gzz.kp(), gzzz.kp()))
    print("G2 (Fp2) madd bound propagation:")
    fixed_point(madd_fp2, True)
    print("G2 (Fp2) FUSED madd bound propagation:")
    fixed_point(madd_fp2_fused, True)
    print("G1 add / dbl class check:")
    check_add_dbl_class()
    print("G2 add / dbl class check:")
    check_add_dbl_class_g2()
    check_table_rows()
    print("bias multiple per subtraction site:", SITE_K)
    print("bias   2 p:", ", ".join("0x%08xu" % v for v in bias_limbs(2)))
    for k in sorted(set(SITE_K.values())):
        print("bias %3d p:" % k, ", ".join("0x%08xu" % v for v in bias_limbs(k)))
    exact_check()
    exact_check_g2()
    exact_check_g2(60, madd_fp2_fused)
    exact_check_add_dbl()
    exact_check_interchange()
    exact_check_add_dbl_g2()
    # mul unit test
    random.seed(1)
    for _ in range(2000):
        a, b = rand_fe(), rand_fe()
        assert from_u29(mul_exact(to_u29(a), to_u29(b))) == a * b % Q
    print("  exact mul: ok")
    for _ in range(2000):
        a = [random.randrange(1 << 30) for _ in range(NL - 1)] + [random.randrange(1 << 24)]   # lazily reduced, un-normalised limbs
        assert sqr_exact(a) == mul_exact(a, a)
    print("  exact sqr (doubled-operand schedule) == mul(a, a): ok")


if __name__ == "__main__":
    main()
