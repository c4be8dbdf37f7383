"""Rounds 4 and 5 of PLONK's prover (gnark v0.8.0 prove.go after the zeta challenge: the evaluations at zeta and omega zeta, kzg.Open of Z,
computeLinearizedPolynomial, the folded quotient, kzg.BatchOpenSinglePoint's fold and its division) in Python integers: what the three row entries
zk_bn254_fr_poly_open_rows_dev, zk_bn254_plonk_linearize_batch_dev and zk_bn254_plonk_open_batch_dev compute, and the rows they are tested on
(tests/test_plonk_open_cpu.py, tests/test_gpu_plonk_open.py).  No device, no library.

The one inverse is pow(x, R - 2, R), so zeta = 1 is defined (1 / 0 = 0, as fr.Element.Inverse has it; the oracle's inv raises there).  Rows are the pool of
tests/plonk_quotient_ref.py -- five witnesses of one circuit, the violated one included: its h is simply 3 (n + 2) coefficients, rounds 4 and 5 have no verdict --
and the zeta and kzg gamma of the rows cover 0, 1, omega (omega zeta wraps to omega^2, zeta^n - 1 = 0), R - 1 and random values."""
from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import plonk_quotient_ref as qr

R = ref.R
M = pl.ints_to_mont_np
POOL = qr.POOL
rows_of = qr.rows_of


def open_at(f, a):
    """-> (f(a), the len(f) - 1 coefficients of (f - f(a)) / (X - a)): the suffix recurrence S_i = f_i + a S_(i+1), q_i = S_(i+1)"""
    q, s = [0] * (len(f) - 1), 0
    for i in range(len(f) - 1, -1, -1):
        if i < len(q):
            q[i] = s
        s = (f[i] + a * s) % R
    return s, q


def linearize(pk, bl, br, bo, bz, h, alpha, beta, gamma, zeta):
    """-> dict(values: the proof's eight [foldedH, lin, l, r, o, s1, s2 at zeta; z at omega zeta], zquot (n + 2), lin (n + 3), fh (n + 2), lag)"""
    d0, n = pk["d0"], pk["n"]
    u = d0.coset
    assert len(bl) == len(br) == len(bo) == n + 2 and len(bz) == n + 3 and len(h) == 3 * (n + 2)
    lz, rz, oz, s1z, s2z = (open_at(p, zeta)[0] for p in (bl, br, bo, pk["s1"], pk["s2"]))
    zu, zquot = open_at(bz, zeta * d0.gen % R)
    c_s3 = (lz + beta * s1z + gamma) * (rz + beta * s2z + gamma) % R * zu % R * beta % R
    c_z = -(lz + beta * zeta + gamma) * (rz + beta * u * zeta + gamma) % R * (oz + beta * u * u * zeta + gamma) % R
    lag = (pow(zeta, n, R) - 1) * pow((zeta - 1) % R, R - 2, R) % R * alpha % R * alpha % R * d0.card_inv % R
    rl = lz * rz % R
    lin = []
    for i in range(n + 3):
        v = bz[i] * c_z % R
        if i < n:
            v = (v + pk["s3"][i] * c_s3) % R
        v = v * alpha % R
        if i < n:
            v = (v + pk["qm"][i] * rl + pk["ql"][i] * lz + pk["qr"][i] * rz + pk["qo"][i] * oz + pk["cqk"][i]) % R
        lin.append((v + bz[i] * lag) % R)
    zp = pow(zeta, n + 2, R)
    fh = [(h[i] + zp * h[n + 2 + i] + zp * zp % R * h[2 * (n + 2) + i]) % R for i in range(n + 2)]
    return dict(values=[open_at(fh, zeta)[0], open_at(lin, zeta)[0], lz, rz, oz, s1z, s2z, zu], zquot=zquot, lin=lin, fh=fh, lag=lag)


def fold7(pk, fh, lin, bl, br, bo, kg):
    """kzg.BatchOpenSinglePoint's fold: fh + g lin + g^2 l + g^3 r + g^4 o + g^5 s1 + g^6 s2, n + 3 coefficients"""
    n = pk["n"]
    folded, acc = [0] * (n + 3), 1
    for p in (fh, lin, bl, br, bo, pk["s1"], pk["s2"]):
        for j, c in enumerate(p):
            folded[j] = (folded[j] + c * acc) % R
        acc = acc * kg % R
    return folded


def open_batch(pk, fh, lin, bl, br, bo, zeta, kg):
    """-> (the n + 2 coefficients of (folded - folded(zeta)) / (X - zeta), folded(zeta))"""
    value, q = open_at(fold7(pk, fh, lin, bl, br, bo, kg), zeta)
    return q, value


def challenges(pk, j, seed):
    """(zeta, kzg gamma) of pool row j: between them the rows take 0, 1, omega, R - 1 and a random value for each"""
    g = ref.SplitMix64(seed * 2003 + j)
    rnd, omega = g.felt(), pk["d0"].gen
    return [omega, 1, 0, R - 1, rnd][j], [0, rnd, R - 1, 1, omega][j]


def pool_row(pk, n_in, j, seed, fast=False, h=None):
    """tests/plonk_quotient_ref.pool_row with what rounds 4 and 5 add: h (the 3 (n + 2) coefficients of round 3: quotient() unless given), zeta, kzg_gamma, and
    the expected outputs of both entries: values, zquot, lin, fh, q, value"""
    row = qr.pool_row(pk, n_in, j, seed, fast)
    n = pk["n"]
    if h is None:
        h = qr.quotient(pk, row["bl"], row["br"], row["bo"], row["bz"], row["public"], row["alpha"], row["beta"], row["gamma"], fast)[0][:3 * (n + 2)]
    row["h"] = list(h)
    row["zeta"], row["kzg_gamma"] = challenges(pk, j, seed)
    row.update(linearize(pk, row["bl"], row["br"], row["bo"], row["bz"], row["h"], row["alpha"], row["beta"], row["gamma"], row["zeta"]))
    row["q"], row["value"] = open_batch(pk, row["fh"], row["lin"], row["bl"], row["br"], row["bo"], row["zeta"], row["kzg_gamma"])
    return row
