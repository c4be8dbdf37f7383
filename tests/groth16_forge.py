"""Groth16 proofs forged under a key whose discrete logarithms are known, for the device batch verifier (tests/test_gpu_verify_forged.py) and, as a
check of this file, the host verifier (tests/test_groth16_forge_cpu.py).  Plain integers, oracle/bn254_ref.py and the vectors of tests/codec_edges.py:
no device, no prover, no Setup, nothing of the library under test.

The key: alpha = a G, beta = b H, gamma = c H, delta = d H, K_j = k_j G (k_j = 0: the point at infinity), written as VerifyingKey.WriteTo bytes.
A proof Ar = x G, Bs = y H, Krs = z G with public inputs w is accepted exactly when
    x y = a b + ic c + z d  (mod r),   ic = k_0 + sum_j w_j k_j,
because e(G, H) has order r.  forge() solves that for z, so the expected verdict of every case below follows from the construction:
  accept      the equation holds and every slot is a valid encoding of a point of the group (the point at infinity included: gnark's decoder reads
              it, and e(O, Q) = e(P, O) = 1)
  reject      the equation is off by a known non-zero amount, or a slot holds bytes that the reference decoders of codec_edges refuse
A "flag-loss" case is a malformed slot in a proof that IS consistent once that slot is read as the point at infinity -- what the device decoder
leaves behind next to its per-point `bad` flag.  A verifier that drops the flag accepts it; every other tamper in the suite is rejected either way."""
import functools
from collections import namedtuple

import numpy as np

from oracle import bn254_ref as ref
from tests import codec_edges as ce

R = ref.R
SLOTS = {"Ar": (0, 32), "Bs": (32, 96), "Krs": (96, 128)}
G1_INF, G2_INF = ref.g1_compress(None), ref.g2_compress(None)

# label, the key, 128 proof bytes, public inputs ((n_public, 4) uint64 Montgomery limbs), expected verdict (0 / 1)
Case = namedtuple("Case", "label key proof pub expect")


def g1(k):
    return ref.g1_mul(ref.G1_GEN, k) if k % R else None


def g2(k):
    return ref.g2_mul(ref.G2_GEN, k) if k % R else None


def limbs(values, plus_r=False):
    """integers mod r -> (n, 4) uint64 Montgomery images; plus_r: each image increased by r (the same value, limbs >= r)"""
    out = np.zeros((len(values), 4), np.uint64)
    for i, v in enumerate(values):
        m = ref.to_mont(v % R, R) + (R if plus_r else 0)
        assert m < 1 << 256
        out[i] = np.frombuffer(m.to_bytes(32, "little"), dtype=np.uint64)
    return out


class ToyKey:
    def __init__(self, a, b, c, d, ks):
        assert a % R and b % R and c % R and d % R and len(ks) >= 1
        self.a, self.b, self.c, self.d, self.ks = a, b, c, d, list(ks)
        self.n_public = len(ks) - 1
        # [alpha]1 [beta]1 [beta]2 [gamma]2 [delta]1 [delta]2 u32 len(K) K
        self.bytes = (ref.g1_compress(g1(a)) + ref.g1_compress(g1(b)) + ref.g2_compress(g2(b)) + ref.g2_compress(g2(c)) + ref.g1_compress(g1(d))
                      + ref.g2_compress(g2(d)) + len(ks).to_bytes(4, "big") + b"".join(ref.g1_compress(g1(k)) for k in ks))

    def ic(self, w):
        assert len(w) == self.n_public
        return (self.ks[0] + sum(wj * kj for wj, kj in zip(w, self.ks[1:]))) % R

    def krs(self, x, y, w):
        return (x * y - self.a * self.b - self.ic(w) * self.c) * pow(self.d, -1, R) % R

    def y_for_krs_at_infinity(self, x, w):
        return (self.a * self.b + self.ic(w) * self.c) * pow(x, -1, R) % R

    def points(self):
        """the oracle's view of the key (ref.groth16_verify)"""
        return dict(g1_alpha=g1(self.a), g2_beta=g2(self.b), g2_gamma=g2(self.c), g2_delta=g2(self.d), g1_ic=[g1(k) for k in self.ks])

    def forge(self, x, y, w, dz=0, ar=None, bs=None, krs=None):
        """the proof (x G, y H, (z + dz) G) with z solving the equation for the public inputs w; ar / bs / krs: raw bytes put in that slot instead"""
        p = [ref.g1_compress(g1(x)), ref.g2_compress(g2(y)), ref.g1_compress(g1(self.krs(x, y, w) + dz))]
        for i, over in enumerate((ar, bs, krs)):
            if over is not None:
                assert len(over) == len(p[i])
                p[i] = bytes(over)
        return b"".join(p)


def _rng(seed):
    g = ref.SplitMix64(seed)
    return lambda: g.felt() % (R - 1) + 1          # never zero


@functools.lru_cache(None)
def key(n_public, k_inf=None):
    """the toy key with n_public public inputs; k_inf: the index j of a K_j at infinity"""
    f = _rng(0x70F0 + n_public)
    ks = [f() for _ in range(n_public + 1)]
    if k_inf is not None:
        ks[k_inf] = 0
    return ToyKey(f(), f(), f(), f(), ks)


KEY = key(2)


def good_cases(k, count, seed=1):
    """count distinct accepted proofs under the key k, each with its own public inputs"""
    f = _rng(0x600D + 131 * k.n_public + seed)
    out = []
    for i in range(count):
        w = [f() for _ in range(k.n_public)]
        out.append(Case("good %d" % i, k, k.forge(f(), f(), w), limbs(w), 1))
    return out


def reject_case(k, seed=7):
    """a well-formed proof whose equation is off by d D: every point decodes, the pairing check refuses it"""
    f = _rng(0xBAD + seed)
    w = [f() for _ in range(k.n_public)]
    return Case("Krs + D", k, k.forge(f(), f(), w, dz=f()), limbs(w), 0)


# ---------------------------------------------------------------------------------------------------------------- flag loss
def vector_class(label, kind):
    """the class of a codec_edges vector: flags 00 / infinity flag with payload / x >= q / x without a point / off-subgroup"""
    if kind == "off-subgroup":
        return kind
    if ">= q" in label:
        return "x >= q"
    if label.startswith("flag 00"):
        return "flags 00"
    if label.startswith("infinity flag"):
        return "infinity flag with payload"
    assert "without a point" in label, label
    return "x without a point"


@functools.lru_cache(None)
def slot_vectors(slot):
    """[(label, bytes, class)]: every encoding that the reference decoders refuse in that slot"""
    if slot in ("Ar", "Krs"):
        vs = [(lab, b, "invalid") for lab, b, kind in ce.g1_decompress_vectors() if kind == "invalid"]
    else:
        vs = [(lab, b, "invalid") for lab, b, kind in ce.g2_decompress_vectors() if kind == "invalid"]
        member = ce.g2_decompress_membership()
        vs += [(lab + " (off the subgroup)", b, "off-subgroup") for lab, b, kind in ce.g2_decompress_vectors() if kind == "valid" and not member[lab]]
        vs += [(lab + " (off the subgroup)", ref.g2_compress(p), "off-subgroup") for lab, p, _, is_member in ce.subgroup_vectors() if not is_member]
    return [(lab, b, vector_class(lab, kind)) for lab, b, kind in vs]


@functools.lru_cache(None)
def _flag_loss_bases(slot):
    """four proofs per slot, each consistent with that slot at infinity: (kwargs of forge without the override, public inputs)"""
    f = _rng(0xF1A6 + len(slot))
    out = []
    for _ in range(4):
        w = [f() for _ in range(KEY.n_public)]
        if slot == "Ar":
            x, y = 0, f()
        elif slot == "Bs":
            x, y = f(), 0
        else:
            x = f()
            y = KEY.y_for_krs_at_infinity(x, w)
            assert KEY.krs(x, y, w) == 0
        out.append((KEY.forge(x, y, w), limbs(w)))
        assert out[-1][0][slice(*SLOTS[slot])] == (G2_INF if slot == "Bs" else G1_INF)
    return out


@functools.lru_cache(None)
def flag_loss_cases(slot):
    """every refused encoding in that slot of a proof consistent with the slot at infinity; all expected 0"""
    lo, hi = SLOTS[slot]
    out = []
    for i, (lab, b, _) in enumerate(slot_vectors(slot)):
        base, pub = _flag_loss_bases(slot)[i % 4]
        out.append(Case("%s <- %s" % (slot, lab), KEY, base[:lo] + b + base[hi:], pub, 0))
    return out


@functools.lru_cache(None)
def flag_loss_representatives():
    """one case per (slot, class)"""
    out = []
    for slot in SLOTS:
        seen = set()
        for case, (_, _, cls) in zip(flag_loss_cases(slot), slot_vectors(slot)):
            if cls not in seen and (cls != "x >= q" or "flag 10" in case.label):       # x >= q under flag bits that are fine
                seen.add(cls)
                out.append(case._replace(label="%s [%s]" % (case.label, cls)))
    return out


# ---------------------------------------------------------------------------------------------------------------- coefficients
# a group of proofs, each rejected alone, whose equations multiply to one: equal (or linearly related) batch coefficients accept them all.
# members: the cases; pairs: per member the exponent pairs [(g1 scalar, g2 scalar), ..] of its equation prod e(P, Q) == 1
Group = namedtuple("Group", "label members pairs")


def _equation(k, x, y, z, w):
    """-e(x G, y H) e(a G, b H) e(ic G, c H) e(z G, d H)"""
    return [(-x % R, y), (k.a, k.b), (k.ic(w), k.c), (z % R, k.d)]


@functools.lru_cache(None)
def coefficient_groups():
    f = _rng(0xC0EF)
    k, out = KEY, []
    D = f()
    # Krs + D and Krs - D on two copies of one proof
    x, y, w = f(), f(), [f(), f()]
    z = k.krs(x, y, w)
    out.append(Group("Krs +- D", [Case("Krs %s D" % s, k, k.forge(x, y, w, dz=dz), limbs(w), 0) for s, dz in (("+", D), ("-", -D))],
                     [_equation(k, x, y, z + dz, w) for dz in (D, -D)]))
    # Ar + D and Ar - D under one Bs (Krs made for Ar)
    x, y, w = f(), f(), [f(), f()]
    z = k.krs(x, y, w)
    out.append(Group("Ar +- D", [Case("Ar %s D" % s, k, k.forge(x, y, w, ar=ref.g1_compress(g1(x + dx))), limbs(w), 0) for s, dx in (("+", D), ("-", -D))],
                     [_equation(k, x + dx, y, z, w) for dx in (D, -D)]))
    # one proof, its public input w_1 + e and w_1 - e
    x, y, w, e = f(), f(), [f(), f()], f()
    z = k.krs(x, y, w)
    ws = [[w[0], (w[1] + de) % R] for de in (e, -e)]
    out.append(Group("w +- e", [Case("w_1 %s e" % s, k, k.forge(x, y, w), limbs(wv), 0) for s, wv in zip("+-", ws)],
                     [_equation(k, x, y, z, wv) for wv in ws]))
    # Krs + 2 D, Krs - D, Krs - D: coefficients r, r, r and r_0 = (r_1 + r_2) / 2 both accept
    x, y, w = f(), f(), [f(), f()]
    z = k.krs(x, y, w)
    dzs = (2 * D, -D, -D)
    out.append(Group("Krs + 2 D, - D, - D", [Case("Krs %s D (member %d)" % ("- 1" if i else "+ 2", i), k, k.forge(x, y, w, dz=dz), limbs(w), 0) for i, dz in enumerate(dzs)],
                     [_equation(k, x, y, z + dz, w) for dz in dzs]))
    return out


# ---------------------------------------------------------------------------------------------------------------- accepts
@functools.lru_cache(None)
def accept_cases():
    """{key name: [Case, ..]}, all expected 1: a point at infinity in each slot, IC at infinity, a key with K_1 at infinity, a key without public inputs,
    the public inputs 0, 1 and r - 1, and public inputs as Montgomery images increased by r"""
    f = _rng(0xACCE)
    out = {}
    for name, k in (("two public inputs", KEY), ("K_1 at infinity", key(2, 1)), ("K_0 at infinity", key(2, 0)), ("no public input", key(0))):
        cs = []

        def add(label, x, y, w, plus_r=False):
            cs.append(Case("%s: %s" % (name, label), k, k.forge(x, y, w), limbs(w, plus_r), 1))

        def ws():
            return [f() for _ in range(k.n_public)]

        add("plain", f(), f(), ws())
        add("Ar at infinity", 0, f(), ws())
        add("Bs at infinity", f(), 0, ws())
        add("Ar and Bs at infinity", 0, 0, ws())
        w, x = ws(), f()
        add("Krs at infinity", x, k.y_for_krs_at_infinity(x, w), w)
        assert cs[-1].proof[96:] == G1_INF
        if k.n_public:
            for v in (0, 1, R - 1):
                add("public inputs %s and random" % ("r - 1" if v == R - 1 else v), f(), f(), [v, f()])
                add("public inputs random and %s" % ("r - 1" if v == R - 1 else v), f(), f(), [f(), v])
            add("public inputs 0, 0", f(), f(), [0, 0])
            add("public inputs r - 1, r - 1", f(), f(), [R - 1, R - 1])
            add("public inputs + r", f(), f(), ws(), plus_r=True)
            add("public inputs 0, r - 1, + r", f(), f(), [0, R - 1], plus_r=True)
            add("public inputs 1, 0, + r, Ar at infinity", 0, f(), [1, 0], plus_r=True)
            if k.ks[2]:
                w0 = f()
                w = [w0, -(k.ks[0] + w0 * k.ks[1]) * pow(k.ks[2], -1, R) % R]
                assert k.ic(w) == 0
                add("IC at infinity", f(), f(), w)
        out[name] = cs
    return out
