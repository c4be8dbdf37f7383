"""Structured inputs for the device NTT / computeH sweeps (tests/test_gpu_ntt_shapes.py), their closed-form transforms in Python integers, and a
re-statement of csrc/ntt.hip's plan_passes() for the coverage check.  tests/test_ntt_shapes_cpu.py checks every builder and closed form against the
C oracle and the pure-Python fft.Domain, so a device mismatch points at the kernel, never at the expectation.

A vector is an (n, 4) uint64 array of Montgomery IMAGES in memory order.  The transforms are linear over Fr, so a closed form can be computed on the
images as field elements directly: T(image(x)) = image(T(x)).  The extreme values (r - 1, 0) are set on the image, because the
kernels' limb bounds concern the 256-bit word they unpack, not the residue behind it."""
import numpy as np

from oracle import bn254_ref as ref

R = ref.R
DIT, DIF = ref.DIT, ref.DIF
ONE_IMG = (1 << 256) % R                      # the image of 1

ALL_MODES = [(i, d, c) for i in (0, 1) for d in (DIT, DIF) for c in (0, 1)]            # (inverse, decimation, coset)
H_MODES = [(0, DIF, 0), (1, DIF, 0), (0, DIT, 1), (1, DIF, 1)]                          # the four combinations computeH uses

# ---------------------------------------------------------------------------------------------------- the pass plan, re-stated
TILE_LOG = 11    # csrc/ntt.hip TILE_LOG
K_STRIDED = 9    # csrc/ntt.hip K_STRIDED (its production value)


def plan_passes(log_n):
    """[(bit_lo, k, logL)] in increasing bit order: the contiguous pass first, then the strided ones -- csrc/ntt.hip plan_passes(), line by line"""
    kc = min(log_n, TILE_LOG)
    rest = log_n - kc
    np_ = (rest + K_STRIDED - 1) // K_STRIDED
    passes = [(0, kc, 0)]
    bit = kc
    for i in range(np_):
        k = (rest - (bit - kc) + (np_ - i) - 1) // (np_ - i)
        logL = min(TILE_LOG - k, bit)
        passes.append((bit, k, logL))
        bit += k
    assert bit == log_n
    return passes


def alt_bits(log_n):
    """the index bits the alt family takes at this size: all of them up to 2^12; above, bits 0, 1, 2, 10, 11, the top two and the first and last bit of
    every pass"""
    if log_n <= 12:
        return list(range(log_n))
    bits = {0, 1, 2, 10, 11, log_n - 2, log_n - 1}
    for bit_lo, k, _ in plan_passes(log_n):
        bits |= {bit_lo, bit_lo + k - 1}
    return sorted(bits)


# ---------------------------------------------------------------------------------------------------------------- limbs
def limbs_of(v):
    return np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)


def from_ints(vals):
    """python integers < 2^256 -> (n, 4) uint64"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def to_ints(a):
    b = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def bitrev_perm(log_n):
    """numpy index array i -> bitrev(i)"""
    idx = np.arange(1 << log_n, dtype=np.uint64)
    out = np.zeros_like(idx)
    for b in range(log_n):
        out |= ((idx >> np.uint64(b)) & np.uint64(1)) << np.uint64(log_n - 1 - b)
    return out.astype(np.int64)


def log2(n):
    log_n = n.bit_length() - 1
    assert n == 1 << log_n
    return log_n


# ------------------------------------------------------------------------------------------------------------- builders
def const(n, image):
    return np.tile(limbs_of(image), (n, 1))


def zeros(n):
    return np.zeros((n, 4), dtype=np.uint64)


def vmax(n):
    return const(n, R - 1)


def alt(n, j, complement=False):
    """r - 1 where bit j of the memory index is clear, 0 where it is set (complement: the other way round)"""
    idx = np.arange(n, dtype=np.uint64)
    hot = ((idx >> np.uint64(j)) & np.uint64(1)) == (1 if complement else 0)
    out = zeros(n)
    out[hot] = limbs_of(R - 1)
    return out


def impulse(n, p):
    out = zeros(n)
    out[p] = limbs_of(ONE_IMG)
    return out


def impulse_positions(n):
    return sorted({p for p in (0, 1, n // 2, n - 1, 2047, 2048) if 0 <= p < n})


def geometric_ratio(n, s, inverse, coset):
    """the ratio q of the logical input x_i = q^i whose transform in this mode is a single non-zero entry at logical index s"""
    dom = ref.Domain(n)
    if inverse:
        return pow(dom.gen, s, R)                                  # sum_i w^(s i) w^(-i k) = n [k == s]
    q = pow(dom.gen_inv, s, R)                                     # sum_i w^(-s i) w^(i k) = n [k == s]
    return q * dom.coset_inv % R if coset else q                   # the coset pre-scale g^i cancels


def geometric(n, s, inverse, decimation, coset):
    """images of x_i = q^i (logical order; stored bit-reversed for DIT, whose input order that is)"""
    q = geometric_ratio(n, s, inverse, coset)
    vals, v = [], ONE_IMG
    for _ in range(n):
        vals.append(v)
        v = v * q % R
    out = from_ints(vals)
    return out if decimation == DIF else out[bitrev_perm(log2(n))]


def geometric_shifts(n):
    return sorted({1 % n, (n - 1) % n, (n // 2 + 1) % n})


def rand_canonical(n, seed):
    """random canonical images (top limb below r's top limb: a value < r for any low limbs)"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    out[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
    return out


def edge_mix(n, seed):
    """random canonical images, about 15 % of them replaced by one of {0, 1, r - 1} (the mix of tools/u29_ntt_model.py's self-test)"""
    rng = np.random.default_rng(seed ^ 0x5EED)
    out = rand_canonical(n, seed)
    pick = rng.random(n) < 0.15
    which = rng.integers(0, 3, size=n)
    for w, image in enumerate((0, 1, R - 1)):
        out[pick & (which == w)] = limbs_of(image)
    return out


def is_canonical(a):
    """every image < r (the input contract of the NTT and computeH entries, include/zkmi.h)"""
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    rl = limbs_of(R)
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < rl[k])
        eq &= a[:, k] == rl[k]
    return bool(lt.all())


# --------------------------------------------------------------------------------------------------------- closed forms
def _geometric_column(n, c, rho):
    vals, v = [], c % R
    for _ in range(n):
        vals.append(v)
        v = v * rho % R
    return vals


def _batch_inverse(xs):
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def _store(vals, decimation, log_n):
    """logical (natural order) outputs -> memory order of the mode: DIF leaves them bit-reversed, DIT natural"""
    out = from_ints(vals)
    if decimation == DIF:
        out = out[bitrev_perm(log_n)]       # memory[i] = X[bitrev(i)]
    return np.ascontiguousarray(out)


def _sparse(n, decimation, k, v):
    out = zeros(n)
    out[ref.bitrev(k, log2(n)) if decimation == DIF else k] = limbs_of(v % R)
    return out


def closed_form(family, n, inverse, decimation, coset):
    """expected memory image of the transform of family (a tuple: name, parameters) in the mode, or None where the family has no closed form.
    FFT:        X_k = sum_i x_i g^i w^(i k)              (g = 1 without coset)
    FFTInverse: X_k = g^-k / n * sum_i x_i w^(-i k)
    x is the LOGICAL input: memory order for DIF, memory[bitrev(i)] for DIT."""
    log_n = log2(n)
    dom = ref.Domain(n)
    name = family[0]
    g = dom.coset if coset else 1
    if name == "zeros":
        return zeros(n)
    if name == "max":
        c = R - 1                                     # as a value: c * 2^-256; its transform's image is the transform of c
        if inverse:                                   # 1/n * n c at k = 0, times g^0
            return _sparse(n, decimation, 0, c)
        if not coset or n == 1:
            return _sparse(n, decimation, 0, c * n)
        # c sum_i (g w^k)^i = c (g^n - 1) / (g w^k - 1); g w^k != 1 because g = 5 is not in the subgroup
        den = _batch_inverse([(v - 1) % R for v in _geometric_column(n, g, dom.gen)])
        num = c * (pow(g, n, R) - 1) % R
        return _store([num * d % R for d in den], decimation, log_n)
    if name == "impulse":
        p = family[1]
        i = p if decimation == DIF else ref.bitrev(p, log_n)            # logical position
        if inverse:
            vals = _geometric_column(n, ONE_IMG * dom.card_inv, pow(dom.gen_inv, i, R) * (dom.coset_inv if coset else 1))
        else:
            vals = _geometric_column(n, ONE_IMG * pow(g, i, R), pow(dom.gen, i, R))
        return _store(vals, decimation, log_n)
    if name == "geometric":
        s = family[1]
        if inverse:
            return _sparse(n, decimation, s, ONE_IMG * (pow(dom.coset_inv, s, R) if coset else 1))
        return _sparse(n, decimation, s, ONE_IMG * n)
    return None


# -------------------------------------------------------------------------------------------------------------- families
STANDALONE_LOG_N = list(range(0, 26))     # the sizes of the stand-alone sweep
H_LOG_N = list(range(0, 23))              # the sizes of the computeH sweep (the entry accepts log_N = 0)
LARGE_FROM = 21                           # from here: computeH's four modes, and max / alt / edge-mix / random only
THIN_ALT_FROM = 23                        # from here every alt vector is taken in ONE mode, and only the first bit of each pass keeps both its vectors (the
                                          # others alternate plain / complement): the oracle needs seconds per transform at these sizes.  The size sweep
                                          # itself is never trimmed


def families(log_n, large=False):
    """the family descriptors of the stand-alone sweep at this size.  large (log_n >= 21): max, the alt subset, edge-mix and random only."""
    n = 1 << log_n
    fams = [("max",)]
    for j in alt_bits(log_n):
        fams += [("alt", j, False), ("alt", j, True)]
    fams += [("edge_mix", 0xE00 + log_n), ("random", 0xA00 + log_n)]
    if not large:
        fams += [("zeros",)]
        fams += [("impulse", p) for p in impulse_positions(n)]
        fams += [("geometric", s) for s in geometric_shifts(n)]
    return fams


def build(family, n, inverse, decimation, coset, rand_fr=None):
    """the input vector of a family in a mode (only geometric depends on the mode).  rand_fr: the oracle's generator, for the random family"""
    name = family[0]
    if name == "zeros":
        return zeros(n)
    if name == "max":
        return vmax(n)
    if name == "alt":
        return alt(n, family[1], family[2])
    if name == "impulse":
        return impulse(n, family[1])
    if name == "geometric":
        return geometric(n, family[1], inverse, decimation, coset)
    if name == "edge_mix":
        return edge_mix(n, family[1])
    if name == "random":
        return rand_fr(family[1], n)
    raise ValueError(family)


def standalone_cases(log_n):
    """[(family, (inverse, decimation, coset))] of the stand-alone sweep at this size"""
    if log_n < LARGE_FROM:
        return [(f, m) for f in families(log_n) for m in ALL_MODES]
    if log_n < THIN_ALT_FROM:
        return [(f, m) for f in families(log_n, large=True) for m in H_MODES]
    cases = [(f, m) for f in families(log_n, large=True) if f[0] != "alt" for m in H_MODES]
    # The complement on the lowest bits of a pass is the vector that shows an all-sums value left unreduced between the stage groups of a DIF pass (the
    # minuend is a sum of zeros, the subtrahend a sum of r - 1: see the module text of tests/test_gpu_ntt_shapes.py), so it goes to a DIF mode.
    first = {bit_lo for bit_lo, _, _ in plan_passes(log_n)}
    for i, j in enumerate(alt_bits(log_n)):
        if j in first:
            cases += [(("alt", j, True), H_MODES[i & 1]), (("alt", j, False), H_MODES[2])]
        else:
            cases.append((("alt", j, bool(i & 1)), H_MODES[i % len(H_MODES)]))
    return cases


def h_lengths(log_n):
    """computeH zero-pads: the full domain, one short of it, a single element, just over half"""
    N = 1 << log_n
    return sorted({n for n in (N, N - 1, 1, N // 2 + 1) if 1 <= n <= N}, reverse=True)


def h_cases(log_n):
    """[(triple, n)] of the computeH sweep: every triple (alt over the bits of alt_bits) at every length, at every size"""
    triples = [("zeros",), ("max",), ("quotient",), ("edge_mix",)] + [("alt", j) for j in alt_bits(log_n)]
    return [(t, n) for t in triples for n in h_lengths(log_n)]


QUOTIENT_PERIOD = 1 << 14


def h_triple(t, log_n, rand_fr, fe_mul):
    """full-length (a, b, c) of a computeH triple.  rand_fr / fe_mul: the oracle's generator and its single-element product (orc.fe_op("mul", 0, x, y)).
    quotient: c = a * b element-wise, so h is a true quotient.  One oracle call per element would take minutes at 2^22, so above 2^14 elements a and b
    repeat a block of 2^14 -- except for the second block, which is a stretch of its own: the vectors are not periodic and their spectra are dense."""
    N = 1 << log_n
    name = t[0]
    if name == "zeros":
        return zeros(N), zeros(N), zeros(N)
    if name == "max":
        return vmax(N), vmax(N), vmax(N)
    if name == "alt":
        return alt(N, t[1]), alt(N, t[1], True), vmax(N)
    if name == "edge_mix":
        return tuple(edge_mix(N, 0xC00 + 16 * log_n + i) for i in range(3))
    if name == "quotient":
        m = min(N, QUOTIENT_PERIOD)
        a, b = rand_fr(0x700 + log_n, m), rand_fr(0x800 + log_n, m)
        c = np.stack([fe_mul(a[i], b[i]) for i in range(m)])
        out = [np.ascontiguousarray(np.tile(v, (N // m, 1))) for v in (a, b, c)]
        if N >= 2 * m:
            a2, b2 = rand_fr(0x900 + log_n, m), rand_fr(0xA80 + log_n, m)
            c2 = np.stack([fe_mul(a2[i], b2[i]) for i in range(m)])
            for v, blk in zip(out, (a2, b2, c2)):
                v[m:2 * m] = blk
        return tuple(out)
    raise ValueError(t)
