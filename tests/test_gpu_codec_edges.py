"""GPU suite: the device key and point codecs one element at a time (csrc/codec_dev.hpp through libzkmi_probe.so, tests/probe.py) against the
reference decoders and encoders on the vectors of tests/codec_edges.py: every flag, coordinate bound, square-root branch, "largest" boundary and
cofactor-torsion point the whole-key tests cannot reach.  Everything is compared as integers, exactly; a failure names the vector."""
import numpy as np
import pytest

from oracle import bn254_ref as ref
from tests import arith_edges as E
from tests import codec_edges as C
from tests import probe

pytestmark = pytest.mark.gpu

Q, R = C.Q, C.R


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    from noir_backend_using_gnark_amd import _lib
    _lib.require_device()


def rows(a):
    return [[int(v) for v in r] for r in a]


def check(name, labels, got, exp):
    assert len(got) == len(exp) == len(labels)
    for lab, g, e in zip(labels, got, exp):
        assert g == e, "%s [%s]: got %s, expected %s" % (name, lab, g, e)


def test_fp_root():
    vs = C.fp_root_vectors()
    labs, vin = [lab for lab, _ in vs], [E.img(a) for _, a in vs]
    exp = [C.fp_root_expect(a) for _, a in vs]
    check("FP_POW_QM3_4", labs, rows(probe.run("FP_POW_QM3_4", vin)), [e[0] for e in exp])
    check("FP_SQRT_CAND", labs, rows(probe.run("FP_SQRT_CAND", vin)), [e[1] for e in exp])


def test_f2_root():
    vs = C.f2_root_vectors()
    got = rows(probe.run("F2_SQRT", [E.img2(a) for _, a, _ in vs]))
    for (lab, a, k), g in zip(vs, got):
        lab = "%s, %s" % (lab, k)
        assert g[0] == (0 if k == "nonsquare" else 1), "F2_SQRT [%s]: ok = %d" % (lab, g[0])
        if g[0]:
            assert all(E.unwords(g[1 + 8 * j:9 + 8 * j]) < Q for j in range(2)), "F2_SQRT [%s]: root not canonical: %s" % (lab, g[1:])
            r = E.unimg2(g[1:])
            assert ref.f2_sqr(r) == a, "F2_SQRT [%s]: %s squared is not %s" % (lab, r, a)


def test_g1_decompress():
    vs = C.g1_decompress_vectors()
    got = rows(probe.run("G1_DECOMPRESS", [C.byte_words(b) for _, b, _ in vs]))
    exp = []
    for _, b, _ in vs:
        p, bad = C.g1_ref_decode(b)
        exp.append(C.g1_img(p) + [bad])                           # an invalid encoding: bad = 1 and the point at infinity
    check("G1_DECOMPRESS", [lab for lab, _, _ in vs], got, exp)


def test_g1_compress():
    vs = C.g1_compress_vectors()
    got = rows(probe.run("G1_COMPRESS", [C.g1_img(p) for _, p in vs]))
    check("G1_COMPRESS", [lab for lab, _ in vs], got, [C.byte_words(ref.g1_compress(p)) for _, p in vs])


def test_g2_decompress_and_membership():
    vs = C.g2_decompress_vectors()
    labs = [lab for lab, _, _ in vs]
    got = rows(probe.run("G2_DECOMPRESS", [C.byte_words(b) for _, b, _ in vs]))
    exp = []
    for _, b, _ in vs:
        p, bad = C.g2_ref_decode(b)
        exp.append(C.g2_img(p) + [bad])
    check("G2_DECOMPRESS", labs, got, exp)
    # the second half of the decoder on the device's own good outputs: accepted exactly when the reference decoder with its subgroup check accepts
    mem = C.g2_decompress_membership()
    good = [(lab, g[:32]) for lab, g in zip(labs, got) if g[32] == 0 and any(g[:32])]
    assert sorted(lab for lab, _ in good) == sorted(mem)
    verdict = rows(probe.run("G2_IN_SUBGROUP", np.array([g for _, g in good], dtype=np.uint32)))
    check("G2_IN_SUBGROUP after G2_DECOMPRESS", [lab for lab, _ in good], verdict, [[1 if mem[lab] else 0] for lab, _ in good])


def test_g2_compress():
    vs = C.g2_compress_vectors()
    got = rows(probe.run("G2_COMPRESS", [C.g2_img(p) for _, p in vs]))
    check("G2_COMPRESS", [lab for lab, _ in vs], got, [C.byte_words(ref.g2_compress(p)) for _, p in vs])


@pytest.mark.parametrize("op", ["G2_IN_SUBGROUP", "G2_IN_SUBGROUP_FULL"])
def test_g2_subgroup(op):
    """the psi test of the key readers and the definition r P = infinity (the A/B arm) on members, twist points, cofactor-torsion points and members
    shifted by them; the point at infinity is passed over as the kernels pass it over"""
    vs = C.subgroup_vectors()
    labs = [lab for lab, _, _, _ in vs] + ["infinity"]
    got = rows(probe.run(op, [C.g2_img(p) for _, p, _, _ in vs] + [C.g2_img(None)]))
    check(op, labs, got, [[1 if m else 0] for _, _, _, m in vs] + [[1]])


def test_fr_codec():
    vs = C.fr_vectors()
    labs = [lab for lab, _ in vs]
    got = rows(probe.run("FR_FROM_BE", [C.fr_be_words(v) for _, v in vs]))
    valid = [(lab, v) for lab, v in vs if v < R]
    for (lab, v), g in zip(vs, got):
        if v < R:
            assert g == C.fr_img(v) + [0], "FR_FROM_BE [%s]: got %s" % (lab, g)
        else:
            assert g[8] == 2, "FR_FROM_BE [%s]: status %d for a value >= r" % (lab, g[8])
    assert len(valid) < len(vs)
    # and back: the canonical big-endian bytes of the image just decoded (to_be(from_be(x)) == x) and of the reference's image
    back = rows(probe.run("FR_TO_BE", [g[:8] for (lab, v), g in zip(vs, got) if v < R]))
    check("FR_TO_BE(FR_FROM_BE)", [lab for lab, _ in valid], back, [C.fr_be_words(v) for _, v in valid])
    back = rows(probe.run("FR_TO_BE", [C.fr_img(v) for _, v in valid]))
    check("FR_TO_BE", [lab for lab, _ in valid], back, [C.fr_be_words(v) for _, v in valid])
    assert labs


def test_hex_codec():
    vs = C.hex_decode_vectors()
    got = rows(probe.run("HEX_DECODE4", [[w] for _, w, _ in vs]))
    for (lab, w, val), g in zip(vs, got):
        if val is None:
            assert g[1] == 1, "HEX_DECODE4 [%s, word %#010x]: accepted as %#06x" % (lab, w, g[0])
        else:
            assert g == [val, 0], "HEX_DECODE4 [%s, word %#010x]: got %s, expected %#06x" % (lab, w, g, val)
    got = probe.run("HEX_ENCODE2", np.arange(65536, dtype=np.uint32).reshape(-1, 1))
    exp = np.array([C.hex_encode_expect(v) for v in range(65536)], dtype=np.uint32)
    wrong = np.nonzero(got[:, 0] != exp)[0]
    assert wrong.size == 0, "HEX_ENCODE2 [value %#06x]: got %#010x, expected %#010x" % (wrong[0], got[wrong[0], 0], exp[wrong[0]])
