"""The bounds model of the 9 x 29-bit-limb arithmetic (tools/u29_model.py) with the window tables' native row format as an input class: table coordinates
(x * 2^261 mod p, packed) unpacked below p and normalised, the digit's sign applied in limb form, the first point of a task copied.  The propagation must reach its fixed point with the biases
the table-less loop already uses (the two variants share the formula's code), every limb below 2^32 and every column sum below 2^64; the limb-form negation
and the flag encoding must agree with big integers."""
import importlib.util
import os
import random

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def m():
    spec = importlib.util.spec_from_file_location("u29_model", os.path.join(HERE, "..", "tools", "u29_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    # the biases of the table-less loops (SITE_K is filled by their propagation; the table classes must not move it)
    mod.fixed_point(mod.madd_fp, False)
    mod.fixed_point(mod.madd_fp2_fused, True)
    return mod


def _edge_values(m):
    Q, W = m.Q, m.W
    vals = [0, 1, 2, Q - 1, Q - 2, (Q - 1) // 2]
    for i in range(1, m.NL):   # the limb boundaries
        for d in (-1, 0, 1):
            vals.append(((1 << (W * i)) + d) % Q)
    vals.append(sum(m.MASK << (W * i) for i in range(m.NL - 1)) % Q)   # every low limb full
    rng = random.Random(5)
    return vals + [rng.randrange(Q) for _ in range(300)]


def test_extended_bounds_model_passes(m, capsys):
    before = dict(m.SITE_K)
    for is_f2 in (False, True):
        X, Y, ZZ, ZZZ = m.fixed_point_table(is_f2)   # asserts: no column sum reaches 2^64, every bias dominates its subtrahend, SITE_K unchanged
        for v in (X, Y, ZZ, ZZZ):
            for b in (v if is_f2 else (v,)):
                assert max(b.lmax) < 1 << 32 and b.vmax < 1 << m.RBITS
    assert m.SITE_K == before
    # the classes themselves: a signed coordinate keeps every limb below 2^31, a copied first point is weakly normalised and below 2 p + 1
    assert max(m.b_tab_signed().lmax) < 1 << 31 and m.b_tab_signed().vmax == 4 * m.Q + 1
    assert m.b_tab_first().vmax == 2 * m.Q + 1 and max(m.b_tab_first().lmax[:-1]) <= m.MASK + 4
    m.exact_check_table(120)
    capsys.readouterr()


def test_limb_form_negation_agrees_with_big_integers(m):
    Q, R261 = m.Q, 1 << m.RBITS
    for x in _edge_values(m):
        t = m.tab_limbs(x)
        assert m.val(t) == x * R261 % Q and all(v <= m.MASK for v in t) and t[-1] < 1 << 22
        for neg in (False, True):
            s = m.tab_sign_exact(t, neg)
            assert all(0 <= v < 1 << 31 for v in s)
            assert m.val(s) == (4 * Q - m.val(t) if neg else m.val(t))
            assert m.from_u29(s) == (-x % Q if neg else x)
            f = m.tab_first_exact(t, neg)
            assert m.from_u29(f) == (-x % Q if neg else x) and m.val(f) <= 2 * Q
            assert all(v < (1 << m.W) + 8 for v in f[:-1])
            # what the first point is then subtracted under: the 4 p bias of site g1.R / g2f.P dominates it limb by limb
            assert all(a <= b for a, b in zip(f, m.bias_limbs(4)))
            # a product takes the un-normalised limbs as they are
            one = m.limbs(R261 % Q)
            assert m.from_u29(m.mul_exact(s, one)) == (-x % Q if neg else x)


def test_flag_encoding_agrees_with_big_integers(m):
    Q = m.Q
    assert m.tab_decode([0] * 16) is None and m.tab_decode([0] * 32) is None   # a zeroed entry: the point at infinity
    assert m.tab_encode(None) is None
    ev = _edge_values(m)
    rng = random.Random(9)
    for nc in (2, 4):
        for _ in range(400):
            coords = tuple(rng.choice(ev) for _ in range(nc))
            words = m.tab_encode(coords)
            assert len(words) == 8 * nc and all(0 <= w < 1 << 32 for w in words)
            # the flag sits in the top word of y (G2: of y.a0) and nowhere else: a value below p < 2^254 leaves the two top bits of its top word free
            flag_at = (nc // 2) * 8 + 7
            assert words[flag_at] & m.TAB_VALID and all(w < 1 << 30 for i, w in enumerate(words) if i % 8 == 7 and i != flag_at)
            assert (words[flag_at] & ~m.TAB_VALID) < 1 << 30
            back = m.tab_decode(words)
            assert back is not None and tuple(m.from_u29(c) for c in back) == coords
            assert all(m.val(c) < Q for c in back)
    # (0, 0) as coordinates is still a point to the decoder -- only the flag says infinity
    assert m.tab_decode(m.tab_encode((0, 0))) == [[0] * 9, [0] * 9]
