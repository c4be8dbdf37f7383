"""The quotient of PLONK's round 3 (gnark v0.8.0 prove.go: the constraints on the coset of the big domain, iop.DivideByXMinusOne, the inverse coset transform)
in Python integers, and the inputs the row-batched device entry is tested on (tests/test_plonk_quotient_cpu.py, tests/test_gpu_plonk_quotient.py).  No device,
no library.

    t(x) = [ ql l + qr r + qm l r + qo o + qk + alpha (z(omega x) prod_j (w_j + beta s_j + gamma) - z prod_j (w_j + beta u^j x + gamma)) + alpha^2 (z - 1) L_1 ] / (x^n - 1)

on the N4 points x = g W^i, then the coset interpolation: N4 coefficients, of which those from 3 (n + 2) on vanish iff the witness satisfies the circuit.  The
arithmetic is Python integers throughout; with fast=True the transforms of 64 points and more go through the C oracle (oracle/bn254_oracle.c), as
oracle/plonk_ref.plonk_prove does it.  tests/test_plonk_quotient_cpu.py holds quotient() against that prover's own h, and the two transform providers against
each other.

Rows of ONE call share ONE key, so the pool needs several witnesses of one circuit: forward_circuit() builds gates whose output wire is a fresh variable with a
non-zero qo, which makes every assignment of the input variables extend to exactly one satisfying solution (solve())."""
import numpy as np

from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import plonk_ratio_ref as rr

R = ref.R
SENTINEL = rr.SENTINEL
M = pl.ints_to_mont_np
strided = rr.strided
POOL = 5


# ------------------------------------------------------------------------------------------------------------- the quotient
def key_tables(pk, fast=False):
    """the key's polynomials on the coset of the big domain, natural order (computed once per key): ql, qr, qm, qo, s1, s2, s3, l1, xs, xn_inv"""
    tag = "_quotient_tables_%d" % fast
    if tag not in pk:
        be, d0, d1, n = pl._Backend(fast), pk["d0"], pk["d1"], pk["n"]
        N4, rho = d1.n, d1.n // d0.n
        ev = lambda p: coset_eval(be, d1, p)
        t = {k: ev(pk[k]) for k in ("ql", "qr", "qm", "qo", "s1", "s2", "s3")}
        t["l1"] = ev([d0.card_inv] * n)                    # L_1 = (X^n - 1) / (n (X - 1)) = (1 / n) sum X^i
        xs, x = [0] * N4, d1.coset
        for i in range(N4):
            xs[i] = x
            x = x * d1.gen % R
        t["xs"] = xs
        t["xn_inv"] = [pow((pow(xs[i], n, R) - 1) % R, -1, R) for i in range(rho)]      # x^n takes rho values on the coset
        pk[tag] = t
    return pk[tag]


def coset_eval(be, d1, p):
    """canonical p -> its values at g W^i, i < N4, natural order"""
    return ref.bit_reverse(be.ntt(d1, list(p) + [0] * (d1.n - len(p)), False, ref.DIF, True))


def completed_qk(pk, public, fast=False):
    """LQk with the public inputs in front, canonical"""
    npub = pk["spr"].n_public
    assert len(public) == npub
    return pl._canonical(pl._Backend(fast), pk["d0"], [v % R for v in public] + list(pk["lqk"][npub:]))


def quotient(pk, bl, br, bo, bz, public, alpha, beta, gamma, fast=False):
    """-> (h[0 .. N4), status): the N4 coefficients of the coset interpolation of t, and 1 if any of h[3 (n + 2) ..) is non-zero, else 0.
    pk: oracle/plonk_ref.plonk_setup's key (its polynomials and domains); bl, br, bo: n + 2 blinded canonical coefficients, bz: n + 3."""
    be, d0, d1, n = pl._Backend(fast), pk["d0"], pk["d1"], pk["n"]
    N4, rho, u = d1.n, d1.n // d0.n, d0.coset
    assert len(bl) == len(br) == len(bo) == n + 2 and len(bz) == n + 3
    T = key_tables(pk, fast)
    e_l, e_r, e_o, e_z, e_qk = (coset_eval(be, d1, p) for p in (bl, br, bo, bz, completed_qk(pk, public, fast)))
    bu, buu = beta * u % R, beta * u % R * u % R
    ql, qr, qm, qo, s1, s2, s3, l1, xs, xn_inv = (T[k] for k in ("ql", "qr", "qm", "qo", "s1", "s2", "s3", "l1", "xs", "xn_inv"))
    t = [0] * N4
    for i in range(N4):
        lv, rv, ov, zv, zs, x = e_l[i], e_r[i], e_o[i], e_z[i], e_z[(i + rho) % N4], xs[i]          # z(omega x): rho steps of W
        gate = (ql[i] * lv + qr[i] * rv + qm[i] * lv % R * rv + qo[i] * ov + e_qk[i]) % R
        lg, rg, og = lv + gamma, rv + gamma, ov + gamma
        a = (lg + beta * x) * (rg + bu * x) % R * (og + buu * x) % R * zv % R
        b = (lg + beta * s1[i]) * (rg + beta * s2[i]) % R * (og + beta * s3[i]) % R * zs % R
        one = (zv - 1) * l1[i] % R
        t[i] = ((one * alpha + (b - a)) % R * alpha + gate) % R * xn_inv[i % rho] % R
    h = be.ntt(d1, ref.bit_reverse(t), True, ref.DIT, True)                    # bit-reversed in -> canonical, regular order out
    return h, int(any(h[3 * (n + 2):]))


def rounds_1_2(pk, sol, blinders, beta, gamma, fast=False):
    """what plonk_prove hands to round 3 for a solution and nine blinders: (bl, br, bo, bz) -- l, r, o in canonical form blinded with two scalars each, Z
    (tests/plonk_ratio_ref.ratio) in canonical form blinded with three"""
    be, d0, n = pl._Backend(fast), pk["d0"], pk["n"]
    l, r, o = pl.evaluate_lro(pk["spr"], n, sol)
    bl, br, bo = (pl._blind(pl._canonical(be, d0, w), n, blinders[2 * k:2 * k + 2]) for k, w in enumerate((l, r, o)))
    z = rr.ratio(l, r, o, pk["perm"], beta, gamma)
    return bl, br, bo, pl._blind(pl._canonical(be, d0, z), n, blinders[6:9])


def setup_polys(spr, fast=False):
    """oracle/plonk_ref.plonk_setup without the SRS: the key's polynomials, permutation and domains -- all that quotient() and rounds_1_2() read -- and none of the
    eight commitments of the verifying key (tests/test_plonk_quotient_cpu.py holds it against plonk_setup)"""
    be = pl._Backend(fast)
    npub, size = spr.n_public, len(spr.constraints) + spr.n_public
    d0 = ref.Domain(size)
    d1 = ref.Domain((8 if size < 6 else 4) * size)
    n = d0.n
    ql, qr_, qm, qo, qk = ([0] * n for _ in range(5))
    for i in range(npub):
        ql[i] = R - 1
    for i, (cl, cr, co, cm, cc, _, _, _) in enumerate(spr.constraints):
        ql[npub + i], qr_[npub + i], qm[npub + i], qo[npub + i], qk[npub + i] = cl % R, cr % R, cm % R, co % R, cc % R
    perm = pl.build_permutation(spr, n)
    sig = rr.sigma(perm, n)
    can = lambda v: pl._canonical(be, d0, v)
    return dict(spr=spr, d0=d0, d1=d1, n=n, perm=perm, ql=can(ql), qr=can(qr_), qm=can(qm), qo=can(qo), cqk=can(qk), lqk=list(qk),
                s1=can(sig[:n]), s2=can(sig[n:2 * n]), s3=can(sig[2 * n:]))


# ------------------------------------------------------------------------------------------- one circuit, many witnesses
def forward_circuit(n, npub, seed):
    """-> (SparseR1CS, number of input variables): n - npub gates with random selectors, qk included, on a domain of exactly n rows.  Gate i reads two
    variables that exist already (inputs or earlier outputs: copy cycles of every length) and writes the fresh variable n_in + i through a non-zero qo; every 7th
    gate has no qm, every 11th no ql, qr, as tests/plonk_shapes.circuit's random family.  Variables: npub public inputs, 3 secret inputs, then the outputs."""
    g = ref.SplitMix64(seed)
    nc, n_in = n - npub, npub + 3
    assert n >= 2 and n & (n - 1) == 0 and nc >= 1
    gates = []
    for i in range(nc):
        ql, qr, qm, qk = g.felt(), g.felt(), g.felt(), g.felt()
        qo = 1 + g.felt() % (R - 1)
        if i % 7 == 0: qm = 0
        if i % 11 == 0: ql = qr = 0
        gates.append((ql, qr, qo, qm, qk, int(g.next() % (n_in + i)), int(g.next() % (n_in + i)), n_in + i))
    return pl.SparseR1CS(npub, 3 + nc, gates), n_in


def solve(spr, inputs):
    """the one solution of a forward circuit with these input values"""
    sol = [v % R for v in inputs]
    for ql, qr, qo, qm, qk, xa, xb, xc in spr.constraints:
        assert xc == len(sol)
        sol.append(-(ql * sol[xa] + qr * sol[xb] + qm * sol[xa] * sol[xb] + qk) * pow(qo, -1, R) % R)
    return sol


def pool_row(pk, n_in, j, seed, fast=False):
    """row j of a pool of POOL rows against one key, each a different witness with different blinders and challenges:
         0  random inputs, alpha = 0            1  random inputs, beta = 0 (Z all ones)
         2  VIOLATED: a satisfied witness with one coefficient of bl incremented (status 1), alpha = beta = gamma = r - 1
         3  the `max` family's values -- public inputs alternate 0, r - 1, secret inputs r - 1 -- with blinders r - 1.  (Its challenges are random: with
            beta = gamma = r - 1 a public input 0 in row n / 2 makes the term l + beta omega^(n/2) + gamma of Z's numerator zero, and the witness no longer passes)
         4  random inputs, gamma = 0
    -> dict(bl, br, bo, bz, public, alpha, beta, gamma, sol, blinders, violated)"""
    spr, n = pk["spr"], pk["n"]
    g = ref.SplitMix64(seed * 1009 + j)
    npub = spr.n_public
    if j == 3:
        inputs = [(R - 1) * (i & 1) for i in range(npub)] + [R - 1] * (n_in - npub)
        blinders, ch = [R - 1] * 9, [g.felt() for _ in range(3)]
    else:
        inputs = [g.felt() for _ in range(n_in)]
        blinders, ch = [g.felt() for _ in range(9)], [g.felt() for _ in range(3)]
    if j == 2:
        ch = [R - 1] * 3
    if j in (0, 1, 4):
        ch[{0: 0, 1: 1, 4: 2}[j]] = 0
    alpha, beta, gamma = ch
    sol = solve(spr, inputs)
    assert spr.is_satisfied(sol)
    bl, br, bo, bz = rounds_1_2(pk, sol, blinders, beta, gamma, fast)
    if j == 2:
        k = int(g.next() % (n + 2))
        bl = list(bl)
        bl[k] = (bl[k] + 1) % R
    return dict(bl=bl, br=br, bo=bo, bz=bz, public=sol[:npub], alpha=alpha, beta=beta, gamma=gamma, sol=sol, blinders=blinders, violated=int(j == 2))


def rows_of(rows):
    """which pool rows a call of `rows` rows takes: from three rows on the violated row sits between satisfied ones"""
    return {1: [0], 2: [3, 4], 3: [1, 2, 3], 5: [0, 1, 2, 3, 4]}[rows]
