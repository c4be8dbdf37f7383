"""Test vectors for the device key and point codecs (csrc/codec_dev.hpp through the probe library; tests/test_gpu_codec_edges.py), one element at a
time at the edges of each encoding, and what the reference decoders say about them.  Every vector and every expectation is built from
oracle/bn254_ref.py and oracle/plonk_ref.py (g1_decompress, g2_decompress(b, subgroup_check=False), f2_sqrt, g1_compress, g2_compress,
ec_mul(FP2, P, R)) and from plain integers -- never from the code under test.  tests/test_codec_edges_cpu.py checks that the tables hold what
they claim, so a device mismatch points at the kernel.

An encoding is handed to the device as it lies in a file: bytes, read as little-endian 32-bit words.  Field elements and points are Montgomery
images (arith_edges.img)."""
import functools
import random
import struct

from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import arith_edges as E

Q, R = ref.Q, ref.R
HALF_LO, HALF_HI = (Q - 1) // 2, (Q + 1) // 2          # the largest "smallest" y and the smallest "largest" y
Y_BOUNDARY = [1, HALF_LO, HALF_HI, Q - 1]
COFACTOR = 2 * Q - R                                    # the twist has (2 q - r) r points
SMALL_ORDERS = [10069, 5864401]
COFACTOR_PRIMES = SMALL_ORDERS + [1875725156269, COFACTOR // (10069 * 5864401 * 1875725156269)]
X0 = ref.X_BN
FLAGS = {"00": 0x00, "01": 0x40, "10": 0x80, "11": 0xC0}


def edge_elements(m):
    """the limb-edge values of arith_edges, (m + 1) / 2 and 2^(32 k) +- 1 below m"""
    out = E.canon_edges(m) + [(m + 1) // 2]
    for k in range(1, 8):
        out += [v for v in ((1 << (32 * k)) - 1, (1 << (32 * k)) + 1) if v < m]
    seen, uniq = set(), []
    for v in out:
        if v not in seen:
            seen.add(v)
            uniq.append(v)
    return uniq


def byte_words(b):
    assert len(b) % 4 == 0
    return list(struct.unpack("<%dI" % (len(b) // 4), bytes(b)))


def is_residue(a):
    return a % Q == 0 or pow(a, (Q - 1) // 2, Q) == 1


def g1_img(p):
    return [0] * 16 if p is None else E.img(p[0]) + E.img(p[1])


def g2_img(p):
    return [0] * 32 if p is None else E.img2(p[0]) + E.img2(p[1])


def enc1(x, flag):
    """32 bytes: x big-endian under the two flag bits (x may be anything below 2^254)"""
    assert 0 <= x < 1 << 254
    b = bytearray(x.to_bytes(32, "big"))
    b[0] |= FLAGS[flag]
    return bytes(b)


def enc2(x0, x1, flag):
    """64 bytes: X.A1 (under the flag bits) | X.A0"""
    assert 0 <= x0 < 1 << 256
    return enc1(x1, flag) + x0.to_bytes(32, "big")


def twist_rhs(x):
    return ref.f2_add(ref.f2_mul(ref.f2_sqr(x), x), ref.B_G2)


# ------------------------------------------------------------------------------------------------------------ Fp root
@functools.lru_cache(None)
def fp_root_vectors():
    """[(label, a)]; expected: a^((q-3)/4) and a^((q+1)/4) (fp_root_expect)"""
    rng = random.Random(101)
    out = [("edge %#x" % a, a) for a in edge_elements(Q)]
    res, non = [], []
    while len(res) < 64 or len(non) < 64:
        a = rng.randrange(1, Q)
        (res if is_residue(a) else non).append(a)
    out += [("residue %d" % i, a) for i, a in enumerate(res[:64])] + [("non-residue %d" % i, a) for i, a in enumerate(non[:64])]
    return out


def fp_root_expect(a):
    return E.img(pow(a, (Q - 3) // 4, Q)), E.img(pow(a, (Q + 1) // 4, Q))


# ------------------------------------------------------------------------------------------------------------ Fp2 root
def f2_class(a):
    """which branch of the complex method an element takes: zero, real+ (root (c, 0)), real- (root (0, c)), chi+ / chi- (the quadratic character of
    t = (a0 + s) / 2 with s = n^((q+1)/4) the root of the norm), nonsquare.  From the reference's own verdict and integer arithmetic."""
    if a == (0, 0):
        return "zero"
    if pl.f2_sqrt(a) is None:
        return "nonsquare"
    if a[1] == 0:
        return "real+" if is_residue(a[0]) else "real-"
    n = (a[0] * a[0] + a[1] * a[1]) % Q
    s = pow(n, (Q + 1) // 4, Q)
    assert s * s % Q == n
    t = (a[0] + s) * HALF_HI % Q
    assert t != 0
    return "chi+" if is_residue(t) else "chi-"


@functools.lru_cache(None)
def f2_root_vectors():
    """[(label, a, class)]; expected: ok == (class != nonsquare) and, when ok, root^2 == a (either root)"""
    rng = random.Random(102)
    edges = edge_elements(Q)
    vs = [("zero", (0, 0))]
    reals = [a for a in edges if a] + [rng.randrange(1, Q) for _ in range(24)]
    vs += [("real (%#x, 0)" % a, (a, 0)) for a in reals]
    vs += [("imaginary (0, %#x)" % a, (0, a)) for a in reals[:24]]
    for i, e in enumerate(edges):
        for sh in (0, 1, 7):
            z = (e, edges[(i + sh) % len(edges)])
            vs.append(("square of edges (%#x, %#x)" % z, ref.f2_sqr(z)))
    for i in range(96):
        vs.append(("random square %d" % i, ref.f2_sqr(E.rand_f2(rng))))
    n_non = 0
    while n_non < 48:
        a = E.rand_f2(rng)
        if pl.f2_sqrt(a) is None:
            vs.append(("random non-square %d" % n_non, a))
            n_non += 1
    return [(lab, a, f2_class(a)) for lab, a in vs]


# ------------------------------------------------------------------------------------------------------------ G1
def g1_ref_decode(b):
    """(point or None, bad) as the reference decoder has it"""
    try:
        return pl.g1_decompress(b), 0
    except ValueError:
        return None, 1


@functools.lru_cache(None)
def g1_valid_xs():
    rng = random.Random(103)
    xs, x = [], 0
    while len(xs) < 16:                      # small ones
        if is_residue(x ** 3 + 3):
            xs.append(x)
        x += 1
    while len(xs) < 64:                      # random ones
        x = rng.randrange(Q)
        if is_residue(x ** 3 + 3):
            xs.append(x)
    return xs


@functools.lru_cache(None)
def g1_invalid_xs():
    rng = random.Random(104)
    xs, x = [], 0
    while len(xs) < 8:
        if not is_residue(x ** 3 + 3):
            xs.append(x)
        x += 1
    while len(xs) < 20:
        x = rng.randrange(Q)
        if not is_residue(x ** 3 + 3):
            xs.append(x)
    return xs


@functools.lru_cache(None)
def g1_decompress_vectors():
    """[(label, 32 bytes, kind)]; expected: g1_ref_decode.  kind: valid / inf / invalid -- what the vector is meant to be (checked by the CPU test)"""
    vs = []
    for x in g1_valid_xs():
        for f in ("10", "11"):
            vs.append(("x %#x flag %s" % (x, f), enc1(x, f), "valid"))
    vs.append(("infinity", enc1(0, "01"), "inf"))
    vs += [("infinity flag, payload %#x" % x, enc1(x, "01"), "invalid") for x in (1, 1 << 248, 1 << 253, 1 << 32, Q - 1)]
    vs += [("flag 00, x %#x" % x, enc1(x, "00"), "invalid") for x in (0, 1, g1_valid_xs()[20])]
    for x in (Q, Q + 1, (1 << 254) - 1):
        vs += [("x %#x (>= q) flag %s" % (x, f), enc1(x, f), "invalid") for f in ("00", "01", "10", "11")]
    for x in g1_invalid_xs():
        vs += [("x %#x without a point, flag %s" % (x, f), enc1(x, f), "invalid") for f in ("10", "11")]
    return vs


@functools.lru_cache(None)
def g1_compress_vectors():
    """[(label, point or None -- raw coordinates, not always on the curve)]; expected: ref.g1_compress"""
    rng = random.Random(105)
    vs = [("infinity", None)]
    for x in g1_valid_xs()[:32]:
        p = pl.g1_decompress(enc1(x, "10"))
        vs += [("point x %#x smallest y" % x, p), ("point x %#x largest y" % x, (p[0], Q - p[1]))]
    for y in Y_BOUNDARY:
        for x in (0, 1, Q - 1, rng.randrange(Q)):
            if (x, y) != (0, 0):
                vs.append(("raw x %#x y %#x" % (x, y), (x, y)))
    return vs


# ------------------------------------------------------------------------------------------------------------ G2
def g2_ref_decode(b):
    try:
        return pl.g2_decompress(b, subgroup_check=False), 0
    except ValueError:
        return None, 1


def real_rhs_xs(want_residue, count):
    """x = (x0, x1) on the twist with x^3 + b' in Fp: x0^2 = (x1^3 - b'_1) / (3 x1), x1 = 1, 2, ...; the real right-hand side a residue (root (c, 0))
    or not (root (0, c)).  x0 and -x0 both make it real, with different real parts."""
    out, x1 = [], 1
    while len(out) < count:
        sq = (x1 ** 3 - ref.B_G2[1]) * pow(3 * x1, -1, Q) % Q
        if is_residue(sq):
            r = pow(sq, (Q + 1) // 4, Q)
            for x0 in (r, Q - r):
                rhs = twist_rhs((x0, x1))
                assert rhs[1] == 0
                if rhs[0] != 0 and is_residue(rhs[0]) == want_residue:
                    out.append((x0, x1))
        x1 += 1
    return out[:count]


@functools.lru_cache(None)
def g2_xs():
    """(valid x values: those with a twist point, invalid ones: those without), labelled"""
    rng = random.Random(106)
    valid, invalid = [], []
    cands = [("G2 point %d G" % k, ref.g2_mul(ref.G2_GEN, k)[0]) for k in (1, 2, 3, X0, 6 * X0 * X0)]
    cands += [("small (%d, %d)" % (a, b), (a, b)) for a in range(4) for b in range(4)]                   # x.a0 = 0, x.a1 = 0 and both among them
    cands += [("x.a0 = 0, x.a1 = %#x" % v, (0, v)) for v in (Q - 1, HALF_LO, rng.randrange(Q), rng.randrange(Q))]
    cands += [("x.a1 = 0, x.a0 = %#x" % v, (v, 0)) for v in (Q - 1, HALF_LO, rng.randrange(Q), rng.randrange(Q))]
    cands += [("edge (%#x, %#x)" % (a, b), (a, b)) for a, b in zip(edge_elements(Q)[3:], edge_elements(Q)[4:])]
    cands += [("random %d" % i, E.rand_f2(rng)) for i in range(48)]
    for lab, x in cands:
        (valid if pl.f2_sqrt(twist_rhs(x)) is not None else invalid).append((lab, x))
    valid += [("real residue right-hand side (%#x, %d)" % x, x) for x in real_rhs_xs(True, 4)]
    valid += [("real non-residue right-hand side (%#x, %d)" % x, x) for x in real_rhs_xs(False, 4)]
    return valid, invalid


@functools.lru_cache(None)
def g2_decompress_vectors():
    """[(label, 64 bytes, kind)]; expected: g2_ref_decode (no subgroup test)"""
    valid, invalid = g2_xs()
    vs = []
    for lab, x in valid:
        vs += [("%s flag %s" % (lab, f), enc2(x[0], x[1], f), "valid") for f in ("10", "11")]
    vs.append(("infinity", enc2(0, 0, "01"), "inf"))
    vs += [("infinity flag, payload a0 %#x a1 %#x" % x, enc2(x[0], x[1], "01"), "invalid") for x in ((1, 0), (0, 1), (1 << 255, 0), (0, 1 << 253), (1 << 32, 0))]
    vs += [("flag 00, x (%#x, %#x)" % x, enc2(x[0], x[1], "00"), "invalid") for x in ((0, 0), valid[0][1])]
    good = valid[0][1]
    for v in (Q, Q + 1, (1 << 254) - 1):
        for f in ("00", "01", "10", "11"):
            vs.append(("x.a1 %#x (>= q) alone, flag %s" % (v, f), enc2(good[0], v, f), "invalid"))
    for v in (Q, Q + 1, (1 << 254) - 1, (1 << 256) - 1):
        for f in ("00", "01", "10", "11"):
            vs.append(("x.a0 %#x (>= q) alone, flag %s" % (v, f), enc2(v, good[1], f), "invalid"))
    for lab, x in invalid:
        vs += [("%s without a point, flag %s" % (lab, f), enc2(x[0], x[1], f), "invalid") for f in ("10", "11")]
    return vs


@functools.lru_cache(None)
def g2_decompress_membership():
    """label -> True / False for every valid vector of g2_decompress_vectors: whether pl.g2_decompress(b, True) accepts it (one multiplication by r
    per x: the two flags give P and -P)"""
    out, by_x = {}, {}
    for lab, b, kind in g2_decompress_vectors():
        if kind != "valid":
            continue
        key = bytes([b[0] & 0x3F]) + b[1:]
        if key not in by_x:
            try:
                pl.g2_decompress(b, True)
                by_x[key] = True
            except ValueError:
                by_x[key] = False
        out[lab] = by_x[key]
    return out


@functools.lru_cache(None)
def g2_compress_vectors():
    """[(label, point or None -- raw coordinates)]; expected: ref.g2_compress"""
    rng = random.Random(107)
    vs = [("infinity", None)]
    for k in (1, 2, 3, X0, R - 1, rng.randrange(R), rng.randrange(R), rng.randrange(R)):
        p = ref.g2_mul(ref.G2_GEN, k)
        vs += [("%d G" % k, p), ("-%d G" % k, ref.g2_neg(p))]
    for x in real_rhs_xs(True, 2) + real_rhs_xs(False, 2):       # the only twist points with y.a1 = 0
        p = pl.g2_decompress(enc2(x[0], x[1], "10"), subgroup_check=False)
        vs += [("twist point with y.a1 = 0, x (%#x, %d)" % x, p), ("its negative, x (%#x, %d)" % x, ref.g2_neg(p))]
    for y in Y_BOUNDARY:
        x = E.rand_f2(rng)
        vs.append(("raw y.a1 %#x" % y, (x, (rng.randrange(Q), y))))
        vs.append(("raw y.a1 %#x, y.a0 = 0" % y, (x, (0, y))))
        vs.append(("raw y.a1 = 0, y.a0 %#x" % y, (x, (y, 0))))
        vs.append(("raw x = 0, y.a1 = 0, y.a0 %#x" % y, ((0, 0), (y, 0))))
    return vs


# ------------------------------------------------------------------------------------------------------------ subgroup
def twist_point(rng):
    while True:
        x = E.rand_f2(rng)
        if pl.f2_sqrt(twist_rhs(x)) is not None:
            return pl.g2_decompress(enc2(x[0], x[1], "10" if rng.random() < 0.5 else "11"), subgroup_check=False)


@functools.lru_cache(None)
def torsion_points():
    """{kind: [T, ...]}: points of the cofactor group, T = r P for a twist point P: of full order 2 q - r, of order 10069, of order 5864401"""
    rng = random.Random(108)
    full = []
    while len(full) < 2:
        t = ref.ec_mul(ref.FP2, twist_point(rng), R)
        if all(ref.ec_mul(ref.FP2, t, COFACTOR // p) is not None for p in COFACTOR_PRIMES):
            full.append(t)
    out = {"full": full}
    for o in SMALL_ORDERS:
        out[str(o)] = [ref.ec_mul(ref.FP2, t, COFACTOR // o) for t in full]
    return out


@functools.lru_cache(None)
def subgroup_vectors():
    """[(label, point, kind, member)]: member = ec_mul(FP2, P, R) is None -- the definition, for EVERY vector; kind names what the point was built as
    (g2 / twist / torsion / shifted)"""
    rng = random.Random(109)
    vs = []
    ks = [1, 2, 3, X0, X0 + 1, 6 * X0 * X0, R - 1]
    vs += [("%d G" % k, ref.ec_mul(ref.FP2, ref.G2_GEN, k), "g2") for k in ks]
    for i in range(24):
        k = rng.randrange(1, R)
        p = ref.ec_mul(ref.FP2, ref.G2_GEN, k)
        vs += [("random multiple %d of G" % i, p, "g2"), ("minus random multiple %d of G" % i, ref.g2_neg(p), "g2")]
    vs += [("random twist point %d" % i, twist_point(rng), "twist") for i in range(32)]
    tors = torsion_points()
    for kind, ts in tors.items():
        for j, t in enumerate(ts):
            vs.append(("torsion point %d of order %s" % (j, kind), t, "torsion"))
            vs.append(("minus torsion point %d of order %s" % (j, kind), ref.g2_neg(t), "torsion"))
            for k in (1, X0, rng.randrange(1, R)):
                vs.append(("%d G + torsion point %d of order %s" % (k, j, kind), ref.ec_add(ref.FP2, ref.ec_mul(ref.FP2, ref.G2_GEN, k), t), "shifted"))
    assert len(vs) <= 200
    return [(lab, p, kind, ref.ec_mul(ref.FP2, p, R) is None) for lab, p, kind in vs]


# ------------------------------------------------------------------------------------------------------------ Fr
@functools.lru_cache(None)
def fr_vectors():
    """[(label, value below 2^256)]; valid exactly when value < r"""
    rng = random.Random(110)
    vs = [("edge %#x" % v, v) for v in edge_elements(R)]
    vs += [("r", R), ("r + 1", R + 1), ("2 r", 2 * R), ("2^256 - 1", (1 << 256) - 1), ("2^255", 1 << 255)]
    vs += [("random %d" % i, rng.randrange(R)) for i in range(64)]
    return vs


def fr_be_words(v):
    return byte_words(v.to_bytes(32, "big"))


def fr_img(v):
    return E.words((v << 256) % R)


# ------------------------------------------------------------------------------------------------------------ hex
HEX_VALUE = {}                                  # the explicit table: 0-9 a-f A-F decode, every other byte value is an error
for _i, _c in enumerate("0123456789"):
    HEX_VALUE[ord(_c)] = _i
for _i, _c in enumerate("abcdef"):
    HEX_VALUE[ord(_c)] = 10 + _i
    HEX_VALUE[ord(_c.upper())] = 10 + _i
HEX_FILL = [b"7cE", b"A0f", b"b9D", b"F3a"]      # the three other characters of a word, mixed case, per position of the byte under test


@functools.lru_cache(None)
def hex_decode_vectors():
    """[(label, text word, decoded 16-bit value or None)]: every byte value at each of the four character positions.  Four characters c0 c1 c2 c3
    (c0 first in the text = the word's low byte) decode to the bytes (c0 c1), (c2 c3), the first in the low byte of the result."""
    vs = []
    for pos in range(4):
        for v in range(256):
            chars = bytearray(HEX_FILL[pos])
            chars.insert(pos, v)
            word = struct.unpack("<I", bytes(chars))[0]
            if v in HEX_VALUE:
                n = [HEX_VALUE[c] for c in chars]
                val = (n[0] << 4 | n[1]) | (n[2] << 4 | n[3]) << 8
            else:
                val = None
            vs.append(("byte %#04x at character %d" % (v, pos), word, val))
    return vs


def hex_encode_expect(b16):
    """the text word of a 16-bit value: its low byte is written first, each byte as two lowercase digits"""
    return struct.unpack("<I", ("%04x" % (((b16 & 0xff) << 8) | (b16 >> 8))).encode())[0]
