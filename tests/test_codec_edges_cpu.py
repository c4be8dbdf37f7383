"""The codec test vectors (tests/codec_edges.py) hold what they claim -- checked with the reference alone, no device.  This is what lets a
mismatch in tests/test_gpu_codec_edges.py point at the kernel: every minimum count is met by the reference's own classification, the special
points are what their labels say, and the reference encoders and decoders agree with each other on every valid vector."""
import collections

from oracle import bn254_ref as ref
from oracle import plonk_ref as pl
from tests import codec_edges as C

Q, R = C.Q, C.R


def test_edge_elements():
    for m in (Q, R):
        e = C.edge_elements(m)
        assert len(set(e)) == len(e) and all(0 <= v < m for v in e)
        for v in (0, 1, 2, m - 1, m - 2, (m - 1) // 2, (m + 1) // 2):
            assert v in e
        for k in range(1, 8):
            assert (1 << 32 * k) - 1 in e and (1 << 32 * k) + 1 in e
    assert C.HALF_LO == (Q - 1) // 2 and C.HALF_HI == (Q + 1) // 2 and C.HALF_LO + 1 == C.HALF_HI
    assert not ref._lex_largest_fp(C.HALF_LO) and ref._lex_largest_fp(C.HALF_HI)
    assert C.Y_BOUNDARY == [1, (Q - 1) // 2, (Q + 1) // 2, Q - 1]


def test_fp_root_table():
    vs = C.fp_root_vectors()
    assert len(set(a for _, a in vs)) == len(vs)
    assert sum(lab.startswith("residue") for lab, _ in vs) == 64 and sum(lab.startswith("non-residue") for lab, _ in vs) == 64
    for lab, a in vs:
        if lab.startswith("residue"):
            assert pow(a, (Q - 1) // 2, Q) == 1
        if lab.startswith("non-residue"):
            assert pow(a, (Q - 1) // 2, Q) == Q - 1
        e, c = (C.E.unimg(w) for w in C.fp_root_expect(a))
        assert c == e * a % Q                                     # a^((q+1)/4) = a^((q-3)/4) a
        assert c * c % Q == (a if C.is_residue(a) else Q - a)    # the candidate is a root of a or of -a
    assert C.fp_root_expect(0) == ([0] * 8, [0] * 8)             # an even exponent: 0 -> 0


def test_f2_root_table():
    vs = C.f2_root_vectors()
    n = collections.Counter(k for _, _, k in vs)
    assert n["chi+"] >= 32 and n["chi-"] >= 32 and n["real+"] >= 8 and n["real-"] >= 8 and n["nonsquare"] >= 32 and n["zero"] >= 1
    assert any(a[0] == 0 and a[1] != 0 for _, a, _ in vs)
    for lab, a, k in vs:
        r = pl.f2_sqrt(a)
        assert (r is None) == (k == "nonsquare"), lab
        if r is not None:
            assert ref.f2_sqr(r) == a, lab
        if k == "real+":                                          # the root is (c, 0)
            assert a[1] == 0 and pow(a[0], (Q + 1) // 4, Q) ** 2 % Q == a[0]
        if k == "real-":                                          # the root is (0, c), c^2 = -a0
            assert a[1] == 0 and pow(a[0], (Q + 1) // 4, Q) ** 2 % Q == Q - a[0]
    # the norm decides: a square in Fp2 exactly when a0^2 + a1^2 is one in Fp
    for lab, a, k in vs:
        assert C.is_residue(a[0] * a[0] + a[1] * a[1]) == (k != "nonsquare"), lab


def test_g1_tables():
    assert len(C.g1_valid_xs()) == 64 and len(set(C.g1_valid_xs())) == 64 and len(set(C.g1_invalid_xs())) >= 16
    vs = C.g1_decompress_vectors()
    assert len(set(b for _, b, _ in vs)) == len(vs)
    kinds = collections.Counter(k for _, _, k in vs)
    assert kinds["valid"] == 128 and kinds["inf"] == 1
    for lab, b, kind in vs:
        p, bad = C.g1_ref_decode(b)
        assert bad == (kind == "invalid"), lab
        assert (p is None) == (kind != "valid"), lab
        if kind == "valid":
            assert ref.g1_on_curve(p) and ref.g1_compress(p) == b, lab
    for x in C.g1_valid_xs():                                    # the two flags give y and q - y, the smaller one under 10
        p, n = pl.g1_decompress(C.enc1(x, "10")), pl.g1_decompress(C.enc1(x, "11"))
        assert p[0] == n[0] == x and p[1] + n[1] == Q and p[1] < n[1]
    labs = [lab for lab, _, _ in vs]
    for x in (Q, Q + 1, (1 << 254) - 1):
        for f in ("10", "11", "01", "00"):
            assert "x %#x (>= q) flag %s" % (x, f) in labs
    assert C.g1_ref_decode(C.enc1(0, "01")) == (None, 0)
    # no G1 point has y = (q -+ 1) / 2: only raw coordinates reach the boundary of "largest"
    for y in (C.HALF_LO, C.HALF_HI):
        c = (y * y - 3) % Q
        assert pow(c, (Q - 1) // 3, Q) != 1
    cv = C.g1_compress_vectors()
    ys = set(p[1] for _, p in cv if p is not None)
    assert set(C.Y_BOUNDARY) <= ys and any(p is None for _, p in cv)
    for lab, p in cv:
        if lab.startswith("point"):
            assert ref.g1_on_curve(p) and pl.g1_decompress(ref.g1_compress(p)) == p, lab
    assert sum(ref.g1_compress(p)[0] >> 6 == 3 for _, p in cv) >= 32 and sum(ref.g1_compress(p)[0] >> 6 == 2 for _, p in cv) >= 32


def test_g2_tables():
    valid, invalid = C.g2_xs()
    assert len(invalid) >= 16 and len(valid) >= 32
    assert any(x[0] == 0 and x[1] != 0 for _, x in valid + invalid) and any(x[1] == 0 and x[0] != 0 for _, x in valid + invalid)
    for want, root_is_real in ((True, True), (False, False)):
        xs = C.real_rhs_xs(want, 4)
        assert len(set(xs)) == 4
        for x in xs:
            rhs = C.twist_rhs(x)
            assert rhs[1] == 0 and rhs[0] != 0 and C.is_residue(rhs[0]) == want       # a zero imaginary part
            y = pl.f2_sqrt(rhs)
            assert ref.f2_sqr(y) == rhs and ((y[1] == 0) if root_is_real else (y[0] == 0))
            assert any(v == x for _, v in valid)
    vs = C.g2_decompress_vectors()
    assert len(set(b for _, b, _ in vs)) == len(vs) and len(set(lab for lab, _, _ in vs)) == len(vs)
    for lab, b, kind in vs:
        p, bad = C.g2_ref_decode(b)
        assert bad == (kind == "invalid"), lab
        assert (p is None) == (kind != "valid"), lab
        if kind == "valid":
            assert ref.g2_on_curve(p) and ref.g2_compress(p) == b, lab
    labs = " | ".join(lab for lab, _, _ in vs)
    assert "x.a0 %#x (>= q) alone" % Q in labs and "x.a1 %#x (>= q) alone" % Q in labs and "infinity flag, payload" in labs
    mem = C.g2_decompress_membership()
    assert sum(mem.values()) >= 8 and sum(not v for v in mem.values()) >= 32
    cv = C.g2_compress_vectors()
    assert set(C.Y_BOUNDARY) <= set(p[1][1] for _, p in cv if p) and set(C.Y_BOUNDARY) <= set(p[1][0] for _, p in cv if p and p[1][1] == 0)
    for lab, p in cv:
        if p is not None and not lab.startswith("raw"):
            assert ref.g2_on_curve(p) and pl.g2_decompress(ref.g2_compress(p), subgroup_check=False) == p, lab


def test_subgroup_table():
    assert C.COFACTOR % (10069 * 5864401 * 1875725156269) == 0
    prod = 1
    for p in C.COFACTOR_PRIMES:
        prod *= p
    assert prod == C.COFACTOR
    tors = C.torsion_points()
    for t in tors["full"]:
        assert ref.g2_on_curve(t) and ref.ec_mul(ref.FP2, t, C.COFACTOR) is None
        assert all(ref.ec_mul(ref.FP2, t, C.COFACTOR // p) is not None for p in C.COFACTOR_PRIMES)
    for o in C.SMALL_ORDERS:                                     # a prime order: o T = infinity and T is not
        for t in tors[str(o)]:
            assert t is not None and ref.g2_on_curve(t) and ref.ec_mul(ref.FP2, t, o) is None
    vs = C.subgroup_vectors()
    assert len(vs) <= 200 and len(set(p for _, p, _, _ in vs)) == len(vs)
    n = collections.Counter(m for _, _, _, m in vs)
    assert n[True] >= 32 and n[False] >= 32
    kinds = collections.Counter(k for _, _, k, _ in vs)
    assert kinds["twist"] == 32 and kinds["g2"] == 7 + 48
    for lab, p, kind, member in vs:
        assert p is not None and ref.g2_on_curve(p), lab
        assert member == (kind == "g2"), lab                      # r P != infinity for every expected reject
    for o in ("full",) + tuple(str(o) for o in C.SMALL_ORDERS):
        assert any("torsion point 0 of order %s" % o == lab for lab, _, _, _ in vs) and any(lab.endswith("G + torsion point 0 of order %s" % o) for lab, _, _, _ in vs)


def test_fr_and_hex_tables():
    vs = dict(C.fr_vectors())
    assert vs["r"] == R and vs["r + 1"] == R + 1 and vs["2^256 - 1"] == (1 << 256) - 1 and R - 1 in vs.values()
    assert sum(lab.startswith("random") for lab in vs) == 64
    for v in vs.values():
        assert int.from_bytes(b"".join(w.to_bytes(4, "little") for w in C.fr_be_words(v)), "big") == v
    hv = C.hex_decode_vectors()
    assert len(hv) == 1024 and sum(v is not None for _, _, v in hv) == 4 * 22 and len(C.HEX_VALUE) == 22
    for lab, word, val in hv:
        text = word.to_bytes(4, "little")
        ok = all(c in b"0123456789abcdefABCDEF" for c in text)
        assert ok == (val is not None), lab
        if ok:
            assert val.to_bytes(2, "little") == bytes.fromhex(text.decode()), lab     # (all four are digits here: no white space for fromhex to skip)
    assert any(text in (b" ", b"\n", b"\t") for text in (bytes([w >> 8 * k & 0xff]) for _, w, v in hv if v is None for k in range(4)))
    for b16 in (0, 0x1234, 0xabcd, 0xffff, 0x00ff):
        assert C.hex_encode_expect(b16).to_bytes(4, "little").decode() == b16.to_bytes(2, "little").hex()
