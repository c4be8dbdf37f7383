"""The copy-constraint ratio Z of PLONK's round 2 (gnark-crypto iop.BuildRatioCopyConstraint, three entries, Lagrange regular) in Python integers, and the inputs
the row-batched device entries are tested on (tests/test_plonk_ratio_cpu.py, tests/test_gpu_plonk_ratio.py).  No device, no library.

    num_i  = prod_j (w_j(i) + beta * u^j * omega^i + gamma)          den_i  = prod_j (w_j(i) + beta * sigma_j(i) + gamma)
    z[0]   = 1,   z[i+1] = z[i] * num_i / den_i                      sigma_j(i) = id(perm[j n + i]),  id(p) = u^(p // n) * omega^(p mod n)

with fr.BatchInvert's rule: the inverse of 0 is 0, so a zero num_i or den_i makes every later z zero (what upstream's rolling products give).  One Montgomery-trick
inversion per row (one modular inverse), so 2^16 elements take a fraction of a second.  tests/test_plonk_ratio_cpu.py holds ratio() against
oracle/plonk_ref.plonk_prove's own Z."""
import numpy as np

from oracle import bn254_ref as ref
from oracle import plonk_ref as pl

R = ref.R
U = ref.FR_GEN                      # the shift between the three copies of the domain: fft.Domain.FrMultiplicativeGen
SENTINEL = np.array([0xDEADBEEFDEADBEEF, 0x0123456789ABCDEF, 0xFEEDFACECAFEF00D, 0x1BADB0021BADB002], dtype=np.uint64)   # tests/test_gpu_ntt_batch.py: not a canonical image
M = pl.ints_to_mont_np
POOL = 5                            # different rows per (size, permutation)

_omegas = {}


def omegas(n):
    """omega^i, i < n"""
    if n not in _omegas:
        w, g = [1] * n, ref.Domain(n).gen if n > 1 else 1
        for i in range(1, n):
            w[i] = w[i - 1] * g % R
        _omegas[n] = w
    return _omegas[n]


def identity_support(n):
    """getSupportIdentityPermutation: omega^i | u omega^i | u^2 omega^i"""
    w = omegas(n)
    return w + [U * x % R for x in w] + [U * U % R * x % R for x in w]


def sigma(perm, n):
    """S1 | S2 | S3 in Lagrange form: ident[perm]"""
    ident = identity_support(n)
    return [ident[p] for p in perm]


def batch_invert(a):
    """fr.BatchInvert: one inversion for the whole vector, zeros stay zeros and take no part"""
    pre, acc = [0] * len(a), 1
    for i, v in enumerate(a):
        pre[i] = acc
        if v:
            acc = acc * v % R
    inv = pow(acc, -1, R)
    out = [0] * len(a)
    for i in range(len(a) - 1, -1, -1):
        if a[i]:
            out[i] = inv * pre[i] % R
            inv = inv * a[i] % R
    return out


def term(l, r, o, sig, n, beta, gamma, i):
    """(num_i, den_i)"""
    w = omegas(n)[i]
    num = (l[i] + beta * w + gamma) * (r[i] + beta * U % R * w + gamma) % R * (o[i] + beta * U * U % R * w + gamma) % R
    den = (l[i] + beta * sig[i] + gamma) * (r[i] + beta * sig[n + i] + gamma) % R * (o[i] + beta * sig[2 * n + i] + gamma) % R
    return num, den


def terms(l, r, o, sig, beta, gamma):
    n = len(l)
    t = [term(l, r, o, sig, n, beta, gamma, i) for i in range(n)]
    return [x[0] for x in t], [x[1] for x in t]


def ratio_from_terms(num, den):
    dinv = batch_invert(den)
    z, acc = [1] * len(num), 1
    for i in range(len(num) - 1):
        acc = acc * num[i] % R * dinv[i] % R
        z[i + 1] = acc
    return z


def ratio(l, r, o, perm, beta, gamma):
    """Z of one witness: n integers"""
    n = len(l)
    return ratio_from_terms(*terms(l, r, o, sigma(perm, n), beta, gamma))


# ------------------------------------------------------------------------------------------------------------------- inputs
def edge_mix(n, seed):
    """n values from {0, 1, r - 1, random}, a quarter each on average"""
    g = ref.SplitMix64(seed)
    out = []
    for _ in range(n):
        k, v = g.next() & 3, g.felt()
        out.append((0, 1, R - 1, v)[k])
    return out


def random_circuit_perm(n, seed):
    """plonk_ref.build_permutation of a random circuit that fills a domain of n rows (n >= 2): long copy cycles through ~n / 3 variables"""
    from tests import plonk_shapes as ps
    spr, _ = ps.circuit("random", n, min(1, n - 1), "full", seed)
    assert ps.domain_size(spr) == n
    return pl.build_permutation(spr, n)


def uniform_perm(n, seed):
    return [int(x) for x in np.random.default_rng(seed).permutation(3 * n)]


PERMS = ("identity", "circuit", "uniform")


def permutation(kind, n, seed):
    if kind == "identity" or (kind == "circuit" and n < 2):
        return list(range(3 * n))
    return random_circuit_perm(n, seed) if kind == "circuit" else uniform_perm(n, seed)


def pool_row(n, j, seed):
    """row j of a pool of POOL rows, each a different vector with different challenges:
       0  l = r = o = r - 1 with beta = gamma = r - 1        1  beta = 0 (Z must be all ones)        POOL - 1  gamma = 0        else  edge mixes, random challenges"""
    g = ref.SplitMix64(seed * 977 + j)
    if j == 0:
        return dict(l=[R - 1] * n, r=[R - 1] * n, o=[R - 1] * n, beta=R - 1, gamma=R - 1)
    row = dict(l=edge_mix(n, seed * 31 + 3 * j), r=edge_mix(n, seed * 31 + 3 * j + 1), o=edge_mix(n, seed * 31 + 3 * j + 2), beta=g.felt(), gamma=g.felt())
    if j == 1:
        row["beta"] = 0
    if j == POOL - 1:
        row["gamma"] = 0
    return row


def rows_of(rows):
    """which pool rows a call of `rows` rows takes: the first is the r - 1 row, the last (from two rows on) the gamma = 0 row, from three on the beta = 0 row is among them"""
    return [0] if rows == 1 else [0] + list(range(1, rows - 1)) + [POOL - 1]


def zero_positions(n, K=8):
    """where a planted zero term meets a boundary of the scan: first element, either side of a lane boundary (K) and of a workgroup boundary (256 K), the last two"""
    return sorted({i for i in (0, K - 1, K, 256 * K - 1, 256 * K, n - 2, n - 1) if 0 <= i < n})


def plant_zero(row, sig, n, i, which):
    """the row with l[i] changed so that the first factor of den_i ("den") or num_i ("num") is zero"""
    s = sig[i] if which == "den" else omegas(n)[i]
    out = dict(row)
    out["l"] = list(row["l"])
    out["l"][i] = (-(row["beta"] * s + row["gamma"])) % R
    return out


def strided(vectors, stride):
    """(len(vectors) * stride + 1, 4): row i at i * stride, everything else -- the gaps and one element behind the last row -- the sentinel"""
    buf = np.tile(SENTINEL, (len(vectors) * stride + 1, 1))
    for i, v in enumerate(vectors):
        buf[i * stride:i * stride + v.shape[0]] = v
    return buf


# ------------------------------------------------------------------------------------- the recurrence on Montgomery images, for sizes too large for ratio()
def boundary_indices(n, plans):
    """every i < n - 1 that is a multiple of K or of 256 K, and the index before each, for each K of `plans`: the lane and workgroup boundaries of the scans"""
    parts = []
    for K in plans:
        m = np.arange(0, n, K, dtype=np.int64)
        parts += [m, m - 1]
    idx = np.unique(np.concatenate(parts))
    return idx[(idx >= 0) & (idx < n - 1)]


def _ints(a):
    raw = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]


def recurrence_failures(z, l, r, o, perm, beta, gamma, idx):
    """the indices i of idx at which z[i+1] * den_i != z[i] * num_i, and those at which num_i or den_i is zero -- in Python integers, on the (n, 4) Montgomery
    images as they are: with beta a plain integer and everything else an image x R, both sides of the identity carry the same power of R = 2^256.
    perm: 3 n positions (numpy); beta, gamma: plain integers."""
    n = l.shape[0]
    idx = np.asarray(idx, dtype=np.int64)
    low = min(n, 2048)                                 # omega^k = omega^(low h) * omega^l with k = low h + l: two small tables instead of n powers
    g = ref.Domain(n).gen if n > 1 else 1
    lo = [pow(g, k, R) for k in range(low)]
    step = pow(g, low, R)
    hi = [[], [], []]                                  # u^j omega^(low h) R: the image of the high part, per copy of the domain
    for j in range(3):
        v = pow(U, j, R) * ref.MONT_R % R
        for _ in range((n + low - 1) // low):
            hi[j].append(v)
            v = v * step % R
    bu, buu, gR = beta * U % R, beta * U * U % R, gamma * ref.MONT_R % R
    zi, zn, lv, rv, ov = _ints(z[idx]), _ints(z[idx + 1]), _ints(l[idx]), _ints(r[idx]), _ints(o[idx])
    sig = []
    for j in range(3):
        p = perm[j * n + idx].astype(np.int64)
        c, k = p // n, p % n
        sig.append([hi[cj][kh] * lo[kl] % R for cj, kh, kl in zip(c.tolist(), (k // low).tolist(), (k % low).tolist())])
    om = [hi[0][kh] * lo[kl] % R for kh, kl in zip((idx // low).tolist(), (idx % low).tolist())]
    bad, zero = [], []
    for i, a, b, x, y, t, wv, s1, s2, s3 in zip(idx.tolist(), zi, zn, lv, rv, ov, om, sig[0], sig[1], sig[2]):
        x += gR
        y += gR
        t += gR
        num = (x + beta * wv) * (y + bu * wv) % R * (t + buu * wv) % R
        den = (x + beta * s1) * (y + beta * s2) % R * (t + beta * s3) % R
        if num == 0 or den == 0:
            zero.append(i)
        if (b * den - a * num) % R:
            bad.append(i)
    return bad, zero
