"""Material for the many-key Groth16 batch verifier (zk_bn254_groth16_verify_batch_keys): rows of (case, the key the row is verified against) built on
tests/groth16_forge.py's ToyKey, whose discrete logarithms are known, so every expected verdict follows from the construction: a case's own verdict under its
own key, 0 under another.  tests/test_groth16_verify_keys_cpu.py holds all of it against the host verifier.  Nothing here asks the device."""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np

from noir_backend_using_gnark_amd import _lib
from oracle import bn254_ref as ref
from tests import groth16_forge as gf

R = gf.R
Case = gf.Case
# members: cases under different keys, each rejected alone, whose errors (exponents of e(G, H)) sum to zero; errors: those exponents
Group = namedtuple("Group", "label members errors")


def fresh_key(n_public, seed):
    """a ToyKey of this file's own: every scalar random and non-zero"""
    f = gf._rng(0x6B16_0000 + seed)
    ks = [f() for _ in range(n_public + 1)]
    return gf.ToyKey(f(), f(), f(), f(), ks)


def plus_r(pub):
    """(n, 4) uint64 Montgomery images -> the same values as images in [r, 2 r)"""
    out = np.zeros_like(pub)
    for i, row in enumerate(pub):
        m = int.from_bytes(row.tobytes(), "little") % R + R
        out[i] = np.frombuffer(m.to_bytes(32, "little"), dtype=np.uint64)
    return out


def _made_accepts(k, seed):
    """the forge's accept variants under any key: plain, a point at infinity in each slot, public inputs + r, IC at infinity"""
    f = gf._rng(0xACC0_0000 + seed)
    cs = []

    def ws():
        return [f() for _ in range(k.n_public)]

    def add(label, x, y, w, wide=False):
        cs.append(Case(label, k, k.forge(x, y, w), gf.limbs(w, wide), 1))

    add("plain", f(), f(), ws())
    add("Ar at infinity", 0, f(), ws())
    add("Bs at infinity", f(), 0, ws())
    w, x = ws(), f()
    add("Krs at infinity", x, k.y_for_krs_at_infinity(x, w), w)
    assert cs[-1].proof[96:] == gf.G1_INF
    if k.n_public:
        add("public inputs + r", f(), f(), ws(), wide=True)
        if k.ks[-1]:
            w = ws()
            w[-1] = -(k.ic(w) - w[-1] * k.ks[-1]) * pow(k.ks[-1], -1, R) % R
            assert k.ic(w) == 0
            add("IC at infinity", f(), f(), w)
    add("plain 2", f(), f(), ws())
    return cs


_FORGE_NAMES = {id(gf.KEY): "two public inputs", id(gf.key(2, 1)): "K_1 at infinity", id(gf.key(2, 0)): "K_0 at infinity", id(gf.key(0)): "no public input"}


@functools.lru_cache(None)
def accepts_of(k):
    """accepted proofs of the key: the forge's table for the forge's keys, the same variants made here for the others"""
    if id(k) in _FORGE_NAMES:
        cs = list(gf.accept_cases()[_FORGE_NAMES[id(k)]])
    else:
        cs = _made_accepts(k, sum(k.bytes[:8]) + 977 * k.n_public)
    assert all(c.key is k and c.expect == 1 for c in cs)
    return cs


@functools.lru_cache(None)
def np2_keys():
    """16 distinct keys with two public inputs: the forge's (plain, K_0 at infinity, K_1 at infinity) and 13 made here"""
    ks = [gf.KEY, gf.key(2, 0), gf.key(2, 1)] + [fresh_key(2, 0x200 + j) for j in range(13)]
    assert len(ks) == 16 and all(k.n_public == 2 for k in ks) and len({k.bytes for k in ks}) == 16
    return ks


N_PUBLIC = (0, 1, 2, 33, 64)


@functools.lru_cache(None)
def npub_keys():
    ks = [fresh_key(n, 0x400 + n) for n in N_PUBLIC]
    assert [k.n_public for k in ks] == list(N_PUBLIC)
    return ks


def tiled_accepts(keys, key_of):
    """rows: lane i an accept of keys[key_of[i]], another one each time the key comes up"""
    seen, rows = {}, []
    for j in key_of:
        k = keys[j]
        cs = accepts_of(k)
        rows.append((cs[seen.get(j, 0) % len(cs)], k))
        seen[j] = seen.get(j, 0) + 1
    return rows


@functools.lru_cache(None)
def wrong_key_rows():
    """an accept of key j of np2_keys() pointed at key j + 1 (rows 0..15), then at key j - 1 (rows 16..31): the same n_public, another key"""
    ks = np2_keys()
    return [(accepts_of(k)[0], ks[(j + d) % len(ks)]) for d in (1, -1) for j, k in enumerate(ks)]


@functools.lru_cache(None)
def cross_key_groups():
    """pairs under two different keys whose errors cancel when the two lanes share a coefficient.  A lane's equation is
    -x y + a b + ic c + z d = 0 in the exponent of e(G, H) whatever its key is, and the combined check adds the lanes' equations times their coefficients"""
    ks = np2_keys()
    f = gf._rng(0xC7055)
    out = []
    # Krs + dz_1 under key A and Krs + dz_2 under key B, dz_2 = -dz_1 d_A / d_B
    A, B = ks[0], ks[3]
    dz1 = f()
    dz2 = -dz1 * A.d % R * pow(B.d, -1, R) % R
    errs = [dz1 * A.d % R, dz2 * B.d % R]
    assert sum(errs) % R == 0 and dz2
    ms = []
    for k, dz, s in ((A, dz1, "1"), (B, dz2, "2")):
        w = [f(), f()]
        ms.append(Case("cross-key Krs + dz_%s" % s, k, k.forge(f(), f(), w, dz=dz), gf.limbs(w), 0))
    out.append(Group("Krs across keys", ms, errs))
    # Ar + dx_1 under A (against Bs = y_1 H) and Ar + dx_2 under B (against y_2 H), dx_2 y_2 = -dx_1 y_1; Krs is made for the undisturbed Ar
    A, B = ks[4], ks[1]
    dx1, y1, y2 = f(), f(), f()
    dx2 = -dx1 * y1 % R * pow(y2, -1, R) % R
    errs = [-dx1 * y1 % R, -dx2 * y2 % R]
    assert sum(errs) % R == 0 and dx2
    ms = []
    for k, dx, y, s in ((A, dx1, y1, "1"), (B, dx2, y2, "2")):
        x, w = f(), [f(), f()]
        ms.append(Case("cross-key Ar + dx_%s" % s, k, k.forge(x, y, w, ar=ref.g1_compress(gf.g1(x + dx))), gf.limbs(w), 0))
    out.append(Group("Ar across keys", ms, errs))
    # w_1 + e_1 under A and w_1 + e_2 under B, e_2 k_B1 c_B = -e_1 k_A1 c_A
    A, B = ks[5], ks[1]
    assert A.ks[1] and B.ks[1]
    e1 = f()
    e2 = -e1 * A.ks[1] % R * A.c % R * pow(B.ks[1] * B.c % R, -1, R) % R
    errs = [e1 * A.ks[1] % R * A.c % R, e2 * B.ks[1] % R * B.c % R]
    assert sum(errs) % R == 0 and e2
    ms = []
    for k, e, s in ((A, e1, "1"), (B, e2, "2")):
        w = [f(), f()]
        ms.append(Case("cross-key w_1 + e_%s" % s, k, k.forge(f(), f(), w), gf.limbs([(w[0] + e) % R, w[1]]), 0))
    out.append(Group("w_1 across keys", ms, errs))
    assert all(g.members[0].key is not g.members[1].key for g in out)
    return out


MANY = 300


@functools.lru_cache(None)
def many_keys():
    """([(key, an accept of it)] for MANY freshly made keys with one public input, a "Krs + D" reject of the last key)"""
    out = []
    f = gf._rng(0x3A00_0000)
    x, y, sx, sy = f(), f(), f(), f()
    X, Y, dX, dY = gf.g1(x), gf.g2(y), gf.g1(sx), gf.g2(sy)      # Ar and Bs step like the keys' points; Krs is solved per key
    for j, k in enumerate(_stepped_keys(MANY, 0x3000)):
        w = [f()]
        proof = ref.g1_compress(X) + ref.g2_compress(Y) + ref.g1_compress(gf.g1(k.krs(x, y, w)))
        if j % 100 == 0:
            assert proof == k.forge(x, y, w)             # as the forge itself would write it
        out.append((k, Case("many %d: accept" % j, k, proof, gf.limbs(w), 1)))
        x, y, X, Y = (x + sx) % R, (y + sy) % R, ref.g1_add(X, dX), ref.g2_add(Y, dY)
    assert len({k.bytes for k, _ in out}) == MANY and len({c.proof for _, c in out}) == MANY
    return out, gf.reject_case(out[-1][0])


def _stepped_keys(count, seed):
    """count ToyKeys with one public input whose scalars step from random starts by random strides: key j's points are key j - 1's plus fixed points, so a
    key costs seven point additions instead of eight scalar multiplications (300 keys in a second).  Every point of every key differs from every other key's"""
    f = gf._rng(0x57E9_0000 + seed)
    names = ("a", "b", "c", "d", "k0", "k1")
    at = {n: f() for n in names}
    step = {n: f() for n in names}
    g1s, g2s = ("a", "b", "d", "k0", "k1"), ("b", "c", "d")
    p1 = {n: gf.g1(at[n]) for n in g1s}
    p2 = {n: gf.g2(at[n]) for n in g2s}
    d1 = {n: gf.g1(step[n]) for n in g1s}
    d2 = {n: gf.g2(step[n]) for n in g2s}
    out = []
    for _ in range(count):
        k = gf.ToyKey.__new__(gf.ToyKey)
        k.a, k.b, k.c, k.d, k.ks = at["a"], at["b"], at["c"], at["d"], [at["k0"], at["k1"]]
        assert all(v % R for v in (k.a, k.b, k.c, k.d, *k.ks))
        k.n_public = 1
        k.bytes = (ref.g1_compress(p1["a"]) + ref.g1_compress(p1["b"]) + ref.g2_compress(p2["b"]) + ref.g2_compress(p2["c"]) + ref.g1_compress(p1["d"])
                   + ref.g2_compress(p2["d"]) + (2).to_bytes(4, "big") + ref.g1_compress(p1["k0"]) + ref.g1_compress(p1["k1"]))
        out.append(k)
        for n in names:
            at[n] = (at[n] + step[n]) % R
        for n in g1s:
            p1[n] = ref.g1_add(p1[n], d1[n])
        for n in g2s:
            p2[n] = ref.g2_add(p2[n], d2[n])
    # the first and the last key as the forge itself would write them
    for k in (out[0], out[-1]):
        assert k.bytes == gf.ToyKey(k.a, k.b, k.c, k.d, k.ks).bytes
    return out


# ---------------------------------------------------------------------------------------------------------------- a batch as the C entry takes it
class Batch:
    """rows [(case, key or None for the case's own)] -> the distinct keys in order of first use (extra: keys given but not referred to, in front), key_of, the
    proofs, the public inputs at `stride` elements per row with `fill` (a uint64, or an rng for garbage that differs per call) behind each row's own, the
    expected verdicts"""

    def __init__(self, rows, stride=None, extra=()):
        self.rows = [(c, c.key if k is None else k) for c, k in rows]
        self.keys = list(extra)
        for _, k in self.rows:
            if not any(k is q for q in self.keys):
                self.keys.append(k)
        self.key_of = np.array([next(j for j, q in enumerate(self.keys) if q is k) for _, k in self.rows], np.uint32)
        self.n = len(self.rows)
        self.blob = b"".join(c.proof for c, _ in self.rows)
        self.stride = max([k.n_public for k in self.keys] + [0]) if stride is None else stride
        self.expect = np.array([c.expect if c.key is k else 0 for c, k in self.rows], np.uint8)
        assert all(c.key.n_public == k.n_public for c, k in self.rows)

    def pubs(self, fill=0xBADC0FFEE0DDF00D, wide=False):
        out = np.full((self.n, self.stride, 4), fill, np.uint64) if not hasattr(fill, "integers") else \
            fill.integers(1, 1 << 63, (self.n, self.stride, 4), dtype=np.uint64)
        for i, (c, k) in enumerate(self.rows):
            if k.n_public:
                out[i, :k.n_public] = plus_r(c.pub) if wide else c.pub
        return out

    def key_args(self):
        """(char*[K], size_t[K]) of the keys' bytes"""
        raw = [k.bytes for k in self.keys]
        return (C.c_char_p * max(len(raw), 1))(*raw), (C.c_size_t * max(len(raw), 1))(*[len(b) for b in raw])


def call_host_form(b, pubs, key_of=None):
    """zk_bn254_groth16_verify_batch_keys itself, its output buffers poisoned -> (rc, accepted bytes, *n_accepted)"""
    acc, n_acc = np.full(max(b.n, 1), 0xEE, np.uint8), C.c_size_t(1 << 40)
    ptrs, lens = b.key_args()
    ko = np.ascontiguousarray(b.key_of if key_of is None else key_of, dtype=np.uint32)
    pubs = np.ascontiguousarray(pubs, dtype=np.uint64)
    rc = _lib.lib().zk_bn254_groth16_verify_batch_keys(b.blob, b.n, ptrs, lens, len(b.keys), 0, _lib.vp(ko), _lib.vp(pubs) if pubs.size else None,
                                                       pubs.shape[1], _lib.vp(acc), C.addressof(n_acc))
    return rc, acc[:b.n], n_acc.value
