"""PLONK proofs and KZG openings forged under an SRS whose secret tau is known, for the device batch verifiers (tests/test_gpu_plonk_verify_forged.py,
tests/test_gpu_kzg.py) and, as a check of this file, the host verifiers (tests/test_plonk_forge_cpu.py).  Plain integers, oracle/bn254_ref.py, the transcript
and the writers of oracle/plonk_ref.py, the vectors of tests/codec_edges.py and the C oracle's multiples of the generator: no device, no prover, no Setup,
nothing of the library under test.

Every point is k G with k known.  The key: S1 S2 S3 Ql Qr Qm Qo Qk = k_X G (k_X = 0: the point at infinity), a domain of n = 2^log_n rows (size_inv, generator
omega and coset shift u from ref.Domain), n_public, srs_g2 = [H, tau H]; written as the 368 bytes of plonk_vk_bytes.  A proof for the public inputs w:
  commitments  L R O Z H0 H1 H2 = a_X G; gamma, beta, alpha, zeta from the transcript as plonk_verify derives them (they bind the commitments only)
  values       quot, lin_z, l, r, o, s1z, s2z at zeta and zu at omega zeta: free, but for ONE that the quotient identity dictates,
                   lin_z + PI(zeta) + f1 f2 (o + gamma) alpha zu - alpha^2 L1(zeta) == quot (zeta^n - 1),  f1 = l + beta s1z + gamma, f2 = r + beta s2z + gamma
  digests      d_fh = a_H0 + zp a_H1 + zp^2 a_H2 (zp = zeta^(n+2));  d_lin = l k_Ql + r k_Qr + l r k_Qm + o k_Qo + k_Qk + c_s3 k_S3 + c_z a_Z
  openings     kg = kzg_derive_gamma(zeta, [d_fh G, d_lin G, L, R, O, S1, S2], the seven values);
               W = sum_k kg^k (d_k - v_k) / (tau - zeta) G,  d = (d_fh, d_lin, a_L, a_R, a_O, k_S1, k_S2);   W' = (a_Z - zu) / (tau - omega zeta) G
because e(C - v G + z X, H) == e(X, tau H) for C = c G, X = x G says c - v + z x = tau x: e(G, H) has order r.

A proof is accepted exactly when  the identity holds,  W and W' are these two points,  the count word is 7  and every point slot decodes (the point at
infinity included: gnark's decoder reads it); the eight values are read mod r, as fr.SetBytes does.  Draft.finish() derives each case's verdict from the
first three conditions and flag_loss_cases() from the reference decoder, so nothing below asks a verifier.  What each kind of case is for:
  identity     the identity is off by a known non-zero amount while BOTH openings are made for the values as written: only the identity check rejects
  flag loss    a refused encoding in a slot of a proof that IS accepted once the slot is read as the point at infinity -- what the device decoder leaves next
               to its `bad` flag.  A verifier that drops the flag accepts it
  header       an accepted proof with another count word
  opening      W or W' off by a known multiple of G.  rho == rho': W + d G and W' - d' G with d' = d (zeta - tau) / (omega zeta - tau): the two errors cancel
               in  rho (.. + zeta W - tau W) + rho' (.. + omega zeta W' - tau W')  exactly when rho == rho'.  A pair: W_1 + d_1 G, W_2 + d_2 G with
               d_2 = -d_1 (zeta_1 - tau) / (zeta_2 - tau): they cancel when the two lanes share their coefficient

W at infinity: every term of its sum is made zero, a_L = l, a_R = r, a_O = o, s1z = k_S1, s2z = k_S2, quot = d_fh, which leaves d_lin == lin_z.  Both sides
are linear in zu: d_lin = A + B zu with B = f1 f2 beta alpha k_S3 (c_s3 = f1 f2 beta alpha zu), and the identity gives lin_z = C - D zu with
C = quot (zeta^n - 1) - PI + alpha^2 L1 and D = f1 f2 (o + gamma) alpha; so zu = (C - A) / (B + D).  d_lin G at infinity: zu = -A / B.  d_fh G at infinity:
H0 = H1 = H2 = infinity (zp is a hash of the three, so nothing else can be solved for).

KZG lanes (C = c G, X = x G, v, z): accepted exactly when c - v + z x == tau x.  For z != tau that is x = (c - v) / (tau - z); for z == tau it is c == v with
ANY x: the check reads e(c G - v G + tau X, H) == e(X, tau H), and the two sides agree whatever X is.  T = C - v G + z X = tau X, so an accepted lane has T at
infinity exactly when X is."""
import functools
from collections import namedtuple

import numpy as np

from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import codec_edges as ce

R = ref.R
TAU = 0x1d3f6a8b0c4e2f9071a5b3c6d8e0f2143a5c7e9092b4d6f81a3c5e7092b4d6f3 % R
POINT_SLOTS = {"L": 0, "R": 32, "O": 64, "Z": 96, "H0": 128, "H1": 160, "H2": 192, "W": 224, "W'": 484}
VALUE_SLOTS = {"quot": 260, "lin_z": 292, "l": 324, "r": 356, "o": 388, "s1z": 420, "s2z": 452, "zu": 516}
COMMITS = ("L", "R", "O", "Z", "H0", "H1", "H2")
KEY_POINTS = ("S1", "S2", "S3", "Ql", "Qr", "Qm", "Qo", "Qk")
G1_INF = ref.g1_compress(None)
_G_IMG = pl.g1_to_np(ref.G1_GEN)
MAX_LOG_N = 28          # plonk_vk_parse (csrc/verify.hip) refuses a size above 2^28, which is also the two-adicity of r - 1

# label, the key, 548 proof bytes, public inputs ((n_public, 4) uint64 Montgomery limbs), expected verdict (0 / 1), kind: accept / identity / flag / header / opening
Case = namedtuple("Case", "label key proof pub expect kind")
# proofs, each rejected alone, whose opening errors cancel when the lanes share their coefficient
Pair = namedtuple("Pair", "label members")


def gmul(ks):
    """[k G for k in ks] as affine integer points, None for k = 0 mod r"""
    sc = np.frombuffer(b"".join((k % R).to_bytes(32, "little") for k in ks), np.uint64).reshape(-1, 4)
    if len(ks) >= 64:                                 # (the many-scalar entry builds its table of the generator per call)
        out = orc.g1_mul_gen_many(sc, scalars_mont=False, nthreads=1)
    else:
        out = [orc.g1_mul(_G_IMG, k, k_mont=False) for k in sc]
    return [pl.g1_from_np(p) for p in out]


def limbs(values):
    """integers mod r -> (n, 4) uint64 Montgomery images"""
    out = np.zeros((len(values), 4), np.uint64)
    for i, v in enumerate(values):
        out[i] = np.frombuffer(ref.to_mont(v % R, R).to_bytes(32, "little"), dtype=np.uint64)
    return out


def plus_r(pub):
    """the same values as Montgomery images increased by r (limbs >= r)"""
    out = np.zeros_like(pub)
    for i, row in enumerate(pub):
        m = int.from_bytes(np.asarray(row, dtype=np.uint64).tobytes(), "little") + R
        assert m < 1 << 256
        out[i] = np.frombuffer(m.to_bytes(32, "little"), dtype=np.uint64)
    return out


def inv(a):
    assert a % R, "a zero denominator: pick another seed"
    return pow(a % R, -1, R)


@functools.lru_cache(None)
def srs_g2():
    pts = [ref.G2_GEN, ref.g2_mul(ref.G2_GEN, TAU)]
    return pts, np.stack([np.frombuffer(ref.g2_affine_mont_bytes(p), dtype=np.uint64) for p in pts])


class ToyKey:
    def __init__(self, name, log_n, n_public, ks):
        assert set(ks) == set(KEY_POINTS) and 0 <= log_n <= MAX_LOG_N
        self.name, self.log_n, self.n, self.n_public, self.ks = name, log_n, 1 << log_n, n_public, dict(ks)
        dom = ref.Domain(self.n)
        assert dom.n == self.n
        self.omega, self.size_inv, self.u = dom.gen, dom.card_inv, dom.coset
        pts = gmul([ks[k] for k in KEY_POINTS])
        g2_pts, self.g2 = srs_g2()
        self.vk = dict(size=self.n, size_inv=self.size_inv, generator=self.omega, n_public=n_public, coset_shift=self.u, srs_g2=g2_pts,
                       s=pts[:3], ql=pts[3], qr=pts[4], qm=pts[5], qo=pts[6], qk=pts[7])
        self.bytes = pl.plonk_vk_bytes(self.vk)
        assert len(self.bytes) == 368


class Draft:
    """the commitments of one proof and what follows from them alone: the challenges, zeta^n - 1, PI(zeta), L1(zeta), zp, d_fh"""

    def __init__(self, key, w, a):
        assert len(w) == key.n_public and set(a) == set(COMMITS)
        self.key, self.w, self.a = key, [x % R for x in w], {k: v % R for k, v in a.items()}
        self.pts = dict(zip(COMMITS, gmul([self.a[k] for k in COMMITS])))
        fs = pl.Transcript("gamma", "beta", "alpha", "zeta")
        pl._bind_public_data(fs, key.vk, self.w)
        self.gamma = fs.challenge_fr("gamma", self.pts["L"], self.pts["R"], self.pts["O"])
        self.beta = fs.challenge_fr("beta")
        self.alpha = fs.challenge_fr("alpha", self.pts["Z"])
        self.zeta = zeta = fs.challenge_fr("zeta", self.pts["H0"], self.pts["H1"], self.pts["H2"])
        assert (TAU - zeta) % R and (TAU - key.omega * zeta) % R
        self.zz = (pow(zeta, key.n, R) - 1) % R
        assert self.zz
        self.pi, wi = 0, 1
        for x in self.w:
            self.pi = (self.pi + wi * key.size_inv % R * self.zz % R * inv(zeta - wi) % R * x) % R
            wi = wi * key.omega % R
        self.l1 = self.zz * key.size_inv % R * inv(zeta - 1) % R
        self.zp = pow(zeta, key.n + 2, R)
        self.d_fh = (self.a["H0"] + self.zp * self.a["H1"] + self.zp * self.zp % R * self.a["H2"]) % R

    def f1f2(self, v):
        return (v["l"] + self.beta * v["s1z"] + self.gamma) * (v["r"] + self.beta * v["s2z"] + self.gamma) % R

    def identity_gap(self, v):
        """left side minus right side of the quotient identity"""
        t = self.f1f2(v) * (v["o"] + self.gamma) % R * self.alpha % R * v["zu"] % R
        return (v["lin_z"] + self.pi + t - self.alpha * self.alpha % R * self.l1 - v["quot"] * self.zz) % R

    def with_lin_z(self, v):
        """v with the lin_z that the identity dictates"""
        v = dict(v, lin_z=0)
        v["lin_z"] = -self.identity_gap(v) % R
        return v

    def with_quot(self, v):
        """v with the quot that the identity dictates (lin_z given)"""
        v = dict(v, quot=0)
        v["quot"] = self.identity_gap(v) * inv(self.zz) % R
        return v

    def d_lin_parts(self, v):
        """d_lin = A + B zu"""
        k, a, b, g, z, u = self.key.ks, self.alpha, self.beta, self.gamma, self.zeta, self.key.u
        c_z = (-(v["l"] + b * z + g) * (v["r"] + b * u % R * z + g) % R * (v["o"] + b * u * u % R * z + g) % R * a + a * a % R * self.l1) % R
        A = (v["l"] * k["Ql"] + v["r"] * k["Qr"] + v["l"] * v["r"] % R * k["Qm"] + v["o"] * k["Qo"] + k["Qk"] + c_z * self.a["Z"]) % R
        B = self.f1f2(v) * b % R * a % R * k["S3"] % R
        return A, B

    def d_lin(self, v):
        A, B = self.d_lin_parts(v)
        return (A + B * v["zu"]) % R

    def opening_scalars(self, v):
        """(kg, w, w'): W = w G and W' = w' G open the digests at the values v"""
        k, a = self.key, self.a
        d = [self.d_fh, self.d_lin(v), a["L"], a["R"], a["O"], k.ks["S1"], k.ks["S2"]]
        claimed = [v[s] for s in ("quot", "lin_z", "l", "r", "o", "s1z", "s2z")]
        fh, lin = gmul(d[:2])
        kg = pl.kzg_derive_gamma(self.zeta, [fh, lin, self.pts["L"], self.pts["R"], self.pts["O"], k.vk["s"][0], k.vk["s"][1]], claimed)
        num, acc = 0, 1
        for dk, vk in zip(d, claimed):
            num = (num + acc * (dk - vk)) % R
            acc = acc * kg % R
        return kg, num * inv(TAU - self.zeta) % R, (a["Z"] - v["zu"]) * inv(TAU - k.omega * self.zeta) % R

    def finish(self, label, v, kind="accept", dw=0, dws=0, count=7, raw=None):
        """the case: the proof with the values v, W + dw G and W' + dws G, the count word `count`; raw: {value slot: the integer < 2^256 written there
        (equal to the value mod r)}.  The verdict follows from the conditions of the module's docstring (every slot decodes: the writer made them)"""
        assert set(v) == set(VALUE_SLOTS) and all(0 <= x < R for x in v.values())
        _, w, ws = self.opening_scalars(v)
        W, Ws = gmul([w + dw, ws + dws])
        p = self.pts
        b = bytearray(pl.plonk_proof_bytes(dict(lro=[p["L"], p["R"], p["O"]], z=p["Z"], h=[p["H0"], p["H1"], p["H2"]], batch_h=W, z_open_h=Ws,
                                                claimed=[v[s] for s in ("quot", "lin_z", "l", "r", "o", "s1z", "s2z")], zu=v["zu"])))
        assert len(b) == 548 and b[256:260] == b"\0\0\0\7"
        b[256:260] = count.to_bytes(4, "big")
        for s, x in (raw or {}).items():
            assert x % R == v[s] and x < 1 << 256
            b[VALUE_SLOTS[s]:VALUE_SLOTS[s] + 32] = x.to_bytes(32, "big")
        expect = int(self.identity_gap(v) == 0 and dw % R == 0 and dws % R == 0 and count == 7)
        assert expect == (kind == "accept") and kind in ("accept", "identity", "header", "opening"), (label, kind, expect)
        return Case("%s: %s" % (self.key.name, label), self.key, bytes(b), limbs(self.w), expect, kind)


# ---------------------------------------------------------------------------------------------------------------- keys
def _rng(seed):
    g = ref.SplitMix64(seed)
    return lambda: g.felt() % (R - 1) + 1          # never zero


@functools.lru_cache(None)
def key(name, log_n, n_public, zero=(), same=()):
    """zero: the key points at infinity; same: (X, Y): k_Y = k_X"""
    f = _rng(0x9E7 + 1009 * log_n + 31 * n_public + sum(KEY_POINTS.index(z) + 1 for z in zero))
    ks = {p: (0 if p in zero else f()) for p in KEY_POINTS}
    if same:
        ks[same[1]] = ks[same[0]]
    return ToyKey(name, log_n, n_public, ks)


def base_key():
    return key("base", 3, 2)


def pi_key():
    return key("three public inputs", 4, 3)


def double_key():
    return key("Ql = Qr", 3, 1, (), ("Ql", "Qr"))


def infinity_keys():
    return [key("%s at infinity" % p, 3, 1, (p,)) for p in KEY_POINTS] + [key("Ql Qr Qm Qo Qk at infinity", 3, 1, ("Ql", "Qr", "Qm", "Qo", "Qk"))]


N_PUBLIC = (0, 1, 2, 31, 32, 33, 64)
LOG_N = (1, 2, 16, 24, MAX_LOG_N)


def n_public_key(n_public):
    return key("n_public %d" % n_public, 7, n_public)


def log_n_key(log_n):
    return key("log_n %d" % log_n, log_n, 1)


# ---------------------------------------------------------------------------------------------------------------- builders
class Forge:
    """seeded drafts and values for one key"""

    def __init__(self, k, seed):
        self.key, self.f = k, _rng(seed)

    def publics(self, pattern="random"):
        f, np_ = self.f, self.key.n_public
        if pattern == "random":
            return [f() for _ in range(np_)]
        if pattern == "edges":                       # 0, r - 1, random, 0, r - 1, ..
            return [(0, R - 1, f())[j % 3] for j in range(np_)]
        if pattern == "edges shifted":               # r - 1, random, 0, ..
            return [(R - 1, f(), 0)[j % 3] for j in range(np_)]
        assert pattern in ("zeros", "r - 1")
        return [0 if pattern == "zeros" else R - 1] * np_

    def draft(self, zero=(), w=None, pattern="random"):
        a = {c: (0 if c in zero else self.f()) for c in COMMITS}
        return Draft(self.key, self.publics(pattern) if w is None else w, a)

    def free(self, **fixed):
        """random values in the seven free slots, but for those given"""
        v = {s: self.f() for s in VALUE_SLOTS if s != "lin_z"}
        v.update(fixed)
        return v

    def good(self, label, zero=(), pattern="random", **fixed):
        d = self.draft(zero, pattern=pattern)
        return d.finish(label, d.with_lin_z(self.free(**fixed)))

    def w_at_infinity(self):
        """(draft, values): every term of W's sum zero (the module's docstring)"""
        d = self.draft()
        k, a = self.key.ks, d.a
        v = dict(l=a["L"], r=a["R"], o=a["O"], s1z=k["S1"], s2z=k["S2"], quot=d.d_fh, zu=0, lin_z=0)
        A, B = d.d_lin_parts(v)
        C = (v["quot"] * d.zz - d.pi + d.alpha * d.alpha % R * d.l1) % R
        D = d.f1f2(v) * (v["o"] + d.gamma) % R * d.alpha % R
        v["zu"] = (C - A) * inv(B + D) % R
        v = d.with_lin_z(v)
        assert v["lin_z"] == d.d_lin(v) and d.opening_scalars(v)[1] == 0
        return d, v

    def ws_at_infinity(self):
        d = self.draft()
        v = d.with_lin_z(self.free(zu=d.a["Z"]))
        assert d.opening_scalars(v)[2] == 0
        return d, v

    def lin_at_infinity(self):
        d = self.draft()
        v = self.free()
        A, B = d.d_lin_parts(dict(v, lin_z=0))
        v["zu"] = -A * inv(B) % R
        v = d.with_lin_z(v)
        assert d.d_lin(v) == 0
        return d, v

    def slot_at_infinity(self, slot):
        """(draft, values) of an accepted proof with the point at infinity in that slot"""
        if slot == "W":
            return self.w_at_infinity()
        if slot == "W'":
            return self.ws_at_infinity()
        d = self.draft((slot,))
        return d, d.with_lin_z(self.free())


def opening_reject(k, seed=5):
    """a well-formed proof whose W is off by a multiple of G: every point decodes, the identity holds, the pairings refuse it"""
    g = Forge(k, 0x0BAD + seed)
    d = g.draft()
    return d.finish("W + d G", d.with_lin_z(g.free()), "opening", dw=g.f())


def good_cases(k, count, seed=1, pattern="random"):
    g = Forge(k, 0x600D + seed)
    return [g.good("good %d" % i, pattern=pattern) for i in range(count)]


# ---------------------------------------------------------------------------------------------------------------- accepts
@functools.lru_cache(None)
def base_accepts():
    k = base_key()
    g = Forge(k, 0xACCE)
    cs = [g.good("baseline")]
    for c in COMMITS:
        cs.append(g.good("%s at infinity" % c, (c,)))
    cs.append(g.good("L R O Z H0 H1 H2 at infinity", COMMITS))
    for slot, what in (("W", "W at infinity"), ("W'", "W' at infinity")):
        d, v = g.slot_at_infinity(slot)
        cs.append(d.finish(what, v))
        assert cs[-1].proof[POINT_SLOTS[slot]:POINT_SLOTS[slot] + 32] == G1_INF
    cs.append(g.good("d_fh G at infinity (H0 H1 H2 at infinity)", ("H0", "H1", "H2")))
    d, v = g.lin_at_infinity()
    cs.append(d.finish("d_lin G at infinity", v))
    # 0 and r - 1 in every value slot: a free slot takes the edge and lin_z absorbs it; for lin_z itself quot is solved for
    for s in VALUE_SLOTS:
        for edge, name in ((0, "0"), (R - 1, "r - 1")):
            d = g.draft()
            v = d.with_quot(dict(g.free(), lin_z=edge)) if s == "lin_z" else d.with_lin_z(g.free(**{s: edge}))
            assert v[s] == edge
            cs.append(d.finish("%s = %s" % (s, name), v))
    # the same value written as v + r and as the largest v + k r below 2^256
    # (2^256 = 5.29 r: the value is chosen below 2^256 - 5 r, so that the largest writing is v + 5 r and takes every subtraction a reduction has)
    for s in VALUE_SLOTS:
        d = g.draft()
        small = g.f() % ((1 << 256) - 5 * R)
        v = d.with_quot(dict(g.free(), lin_z=small)) if s == "lin_z" else d.with_lin_z(g.free(**{s: small}))
        top = v[s] + 5 * R
        assert v[s] == small and top < 1 << 256 <= top + R
        cs.append(d.finish("%s written as v + r" % s, v, raw={s: v[s] + R}))
        cs.append(d.finish("%s written as the largest v + k r" % s, v, raw={s: top}))
    d = g.draft()
    v = d.with_lin_z(g.free())
    cs.append(d.finish("every value written as v + r", v, raw={s: v[s] + R for s in VALUE_SLOTS}))
    return cs


@functools.lru_cache(None)
def key_accepts():
    """{key name: cases}: every key with a point at infinity, Ql = Qr with a doubling and a cancellation in the digest's sum, the key with three public inputs"""
    out = {}
    for k in infinity_keys():
        g = Forge(k, 0x1AF + sum(map(ord, k.name)))
        d, v = g.w_at_infinity() if "S3" not in k.name else g.ws_at_infinity()
        out[k.name] = [g.good("baseline"), g.good("public input 0", pattern="zeros"), d.finish("W or W' at infinity", v)]
    k = double_key()
    g = Forge(k, 0xD0B1)
    l = g.f()
    out[k.name] = [g.good("baseline"), g.good("l = r: l Ql + r Qr doubles", l=l, r=l), g.good("r = -l: l Ql + r Qr cancels", l=l, r=R - l),
                   g.good("l = r = 0, o = 0", l=0, r=0, o=0)]
    k = pi_key()
    g = Forge(k, 0x3141)
    out[k.name] = [g.good("baseline"), g.good("public inputs 0, r - 1, random", pattern="edges"), g.good("public inputs r - 1", pattern="r - 1")]
    return out


@functools.lru_cache(None)
def n_public_cases(n_public):
    k = n_public_key(n_public)
    g = Forge(k, 0x9B + n_public)
    return [g.good("random"), g.good("0, r - 1, random", pattern="edges"), g.good("r - 1, random, 0", pattern="edges shifted"), g.good("zeros", pattern="zeros")]


@functools.lru_cache(None)
def log_n_cases(log_n):
    k = log_n_key(log_n)
    g = Forge(k, 0x106 + log_n)
    return [g.good("random"), g.good("public input r - 1", pattern="r - 1"), g.good("Z at infinity", ("Z",))]


# ---------------------------------------------------------------------------------------------------------------- rejects
@functools.lru_cache(None)
def identity_rejects():
    """only the quotient identity refuses these: W and W' open the digests at the values as written"""
    g = Forge(base_key(), 0x1DE7)
    out = []
    for s in ("quot", "lin_z"):
        d = g.draft()
        v = d.with_lin_z(g.free())
        v[s] = (v[s] + 1) % R
        out.append(d.finish("%s + 1" % s, v, "identity"))
    d = g.draft()
    v = d.with_lin_z(g.free(zu=0))                    # zu = 0: the permutation term vanishes, the identity is lin_z + PI - alpha^2 L1 == quot (zeta^n - 1)
    v["lin_z"] = (v["lin_z"] + 1) % R
    out.append(d.finish("lin_z + 1 with zu = 0", v, "identity"))
    g = Forge(pi_key(), 0x1DE8)
    d = g.draft()
    assert d.pi
    v = d.with_lin_z(g.free())
    v["lin_z"] = (v["lin_z"] + d.pi) % R              # the lin_z of an identity without PI(zeta)
    out.append(d.finish("lin_z made without PI", v, "identity"))
    d = g.draft(w=[0, 0, g.f()])                      # only the last public input counts
    assert d.pi
    v = d.with_lin_z(g.free())
    v["lin_z"] = (v["lin_z"] + d.pi) % R
    out.append(d.finish("lin_z made without PI, public inputs 0, 0, w", v, "identity"))
    return out


@functools.lru_cache(None)
def refused_encodings():
    """[(label, 32 bytes)]: every G1 encoding of the codec tables that the reference decoder refuses"""
    return [(lab, b) for lab, b, kind in ce.g1_decompress_vectors() if kind == "invalid"]


def encoding_class(label):
    if ">= q" in label:
        return "x >= q"
    if label.startswith("flag 00"):
        return "flags 00"
    if label.startswith("infinity flag"):
        return "infinity flag with payload"
    assert "without a point" in label, label
    return "x without a point"


@functools.lru_cache(None)
def flag_loss_bases(slot):
    """two accepted proofs with the point at infinity in that slot: (draft, values, the accepted case)"""
    g = Forge(base_key(), 0xF1A6 + POINT_SLOTS[slot])
    out = []
    for i in range(2):
        d, v = g.slot_at_infinity(slot)
        out.append((d, v, d.finish("%s at infinity (flag-loss base %d)" % (slot, i), v)))
    return out


@functools.lru_cache(None)
def flag_loss_cases(slot):
    """every refused encoding in that slot of a proof that is accepted with the slot at infinity; all expected 0"""
    out, off = [], POINT_SLOTS[slot]
    for i, (lab, b) in enumerate(refused_encodings()):
        base = flag_loss_bases(slot)[i % 2][2]
        assert base.expect == 1 and base.proof[off:off + 32] == G1_INF and len(b) == 32
        try:
            pl.g1_decompress(b)
            raise AssertionError("the reference decoder reads %s" % lab)
        except ValueError:
            pass
        out.append(base._replace(label="%s: %s <- %s" % (base.key.name, slot, lab), proof=base.proof[:off] + b + base.proof[off + 32:], expect=0, kind="flag"))
    return out


@functools.lru_cache(None)
def flag_loss_representatives():
    """one case per (slot, class of encoding)"""
    out = []
    for slot in POINT_SLOTS:
        seen = set()
        for c, (lab, _) in zip(flag_loss_cases(slot), refused_encodings()):
            cls = encoding_class(lab)
            if cls not in seen and (cls != "x >= q" or "flag 10" in lab):
                seen.add(cls)
                out.append(c)
    return out


@functools.lru_cache(None)
def header_rejects():
    g = Forge(base_key(), 0x4EAD)
    out = []
    for count in (6, 8):
        d = g.draft()
        out.append(d.finish("count word %d" % count, d.with_lin_z(g.free()), "header", count=count))
    return out


@functools.lru_cache(None)
def opening_rejects():
    """W + d G, W' + d G, and both in one proof so that they cancel when rho == rho'"""
    g = Forge(base_key(), 0x09E4)
    out = []
    for what, sel in (("W + d G", (1, 0)), ("W' + d G", (0, 1))):
        d = g.draft()
        dl = g.f()
        out.append(d.finish(what, d.with_lin_z(g.free()), "opening", dw=dl * sel[0], dws=dl * sel[1]))
    for i in range(2):
        d = g.draft()
        dl = g.f()
        dl2 = dl * (d.zeta - TAU) % R * inv(d.key.omega * d.zeta - TAU) % R
        # rho (zeta - tau) dl - rho' (omega zeta - tau) dl2 == 0 exactly when rho == rho'
        assert (dl * (d.zeta - TAU) - dl2 * (d.key.omega * d.zeta - TAU)) % R == 0 and dl2
        out.append(d.finish("W + d G and W' - d' G (cancel when rho == rho') %d" % i, d.with_lin_z(g.free()), "opening", dw=dl, dws=-dl2))
    return out


def rho_cases():
    return [c for c in opening_rejects() if "rho == rho'" in c.label]


@functools.lru_cache(None)
def cancelling_pairs():
    """two proofs with different zeta, W_1 + d_1 G and W_2 + d_2 G: the errors cancel when both lanes use one coefficient"""
    g = Forge(base_key(), 0xCA9C)
    out = []
    for i in range(3):
        d1, d2 = g.draft(), g.draft()
        assert d1.zeta != d2.zeta
        dl1 = g.f()
        dl2 = -dl1 * (d1.zeta - TAU) % R * inv(d2.zeta - TAU) % R
        assert (dl1 * (d1.zeta - TAU) + dl2 * (d2.zeta - TAU)) % R == 0 and dl2
        out.append(Pair("pair %d" % i, [d1.finish("pair %d: W_1 + d_1 G" % i, d1.with_lin_z(g.free()), "opening", dw=dl1),
                                        d2.finish("pair %d: W_2 + d_2 G" % i, d2.with_lin_z(g.free()), "opening", dw=dl2)]))
    return out


# ---------------------------------------------------------------------------------------------------------------- the table
@functools.lru_cache(None)
def table():
    """{key name: [Case, ..]}: every case of this file, by key"""
    out = {}

    def add(cases):
        for c in cases:
            out.setdefault(c.key.name, []).append(c)

    add(base_accepts())
    add(good_cases(base_key(), 8))
    for cs in key_accepts().values():
        add(cs)
    for n_public in N_PUBLIC:
        add(n_public_cases(n_public))
    for log_n in LOG_N:
        add(log_n_cases(log_n))
    add(identity_rejects())
    for slot in POINT_SLOTS:
        add(c for _, _, c in flag_loss_bases(slot))
        add(flag_loss_cases(slot))
    add(header_rejects())
    add(opening_rejects())
    for p in cancelling_pairs():
        add(p.members)
    for k in infinity_keys() + [double_key(), pi_key()] + [n_public_key(n) for n in N_PUBLIC] + [log_n_key(n) for n in LOG_N]:
        add([opening_reject(k)])
    return out


# the table's keys (a constant, so that a test can be parametrised over them without forging anything)
KEY_NAMES = (["base"] + ["%s at infinity" % p for p in KEY_POINTS] + ["Ql Qr Qm Qo Qk at infinity", "Ql = Qr", "three public inputs"]
             + ["n_public %d" % n for n in N_PUBLIC] + ["log_n %d" % n for n in LOG_N])


# ---------------------------------------------------------------------------------------------------------------- KZG lanes
# C = c G, X = x G (the opening proof; the module's docstring), claimed value v, point z, expected verdict
Lane = namedtuple("Lane", "label c x v z expect")


def _lane(label, c, v, z, dx=0, x=None):
    if x is None:
        x = (c - v) * inv(TAU - z) % R
    x = (x + dx) % R
    return Lane(label, c % R, x, v % R, z % R, int((c - v + z * x - TAU * x) % R == 0))


@functools.lru_cache(None)
def kzg_accepts():
    f = _rng(0x4296)
    out = []
    for vn, v in (("0", 0), ("1", 1), ("2^192 - 1", (1 << 192) - 1), ("2^224", 1 << 224), ("r - 1", R - 1), ("random", f())):
        for zn, z in (("0", 0), ("1", 1), ("r - 1", R - 1), ("random", f())):
            out.append(_lane("v = %s, z = %s" % (vn, zn), f(), v, z))
    out.append(_lane("C at infinity", 0, f(), f()))
    out.append(_lane("C at infinity, v = 0: X at infinity too", 0, 0, f()))
    v = f()
    out.append(_lane("c = v: X and C - v G + z X at infinity", v, v, f()))
    out.append(_lane("c = v, z = 0", v, v, 0))
    out.append(_lane("z = tau, c = v, X arbitrary", v, v, TAU, x=f()))
    out.append(_lane("z = tau, c = v = 0, X arbitrary", 0, 0, TAU, x=f()))
    out.append(_lane("z = tau, c = v, X at infinity", v, v, TAU, x=0))
    assert all(l.expect == 1 for l in out)
    assert out[-5].x == 0 and out[-6].x == 0
    return out


@functools.lru_cache(None)
def kzg_rejects():
    f = _rng(0x4297)
    out = [_lane("X + d G", f(), f(), f(), dx=f()), _lane("X + d G, v = 1", f(), 1, f(), dx=f()), _lane("X + d G, z = 0", f(), f(), 0, dx=f()),
           _lane("X at infinity where it is not", f(), f(), f(), x=0), _lane("z = tau, c != v", f(), f(), TAU, x=f())]
    assert all(l.expect == 0 for l in out)
    return out


@functools.lru_cache(None)
def kzg_cancelling_pairs():
    """[(lane, lane)]: lambda_1 d_1 (z_1 - tau) + lambda_2 d_2 (z_2 - tau) == 0 when lambda_1 == lambda_2"""
    f = _rng(0x4298)
    out = []
    for i in range(3):
        z1, z2, d1 = f(), f(), f()
        d2 = -d1 * (z1 - TAU) % R * inv(z2 - TAU) % R
        assert (d1 * (z1 - TAU) + d2 * (z2 - TAU)) % R == 0
        pair = (_lane("pair %d: X_1 + d_1 G" % i, f(), f(), z1, dx=d1), _lane("pair %d: X_2 + d_2 G" % i, f(), f(), z2, dx=d2))
        assert pair[0].expect == 0 and pair[1].expect == 0
        out.append(pair)
    return out


def kzg_arrays(lanes):
    """(digests (n, 8), proofs (n, 8), claimed values (n, 4), points (n, 4), expected (n,) uint8, srs_g2 (2, 16)): affine and Montgomery images"""
    pts = gmul([l.c for l in lanes] + [l.x for l in lanes])
    img = np.stack([np.frombuffer(ref.g1_affine_mont_bytes(p), dtype=np.uint64) for p in pts])
    n = len(lanes)
    return (np.ascontiguousarray(img[:n]), np.ascontiguousarray(img[n:]), limbs([l.v for l in lanes]), limbs([l.z for l in lanes]),
            np.array([l.expect for l in lanes], np.uint8), srs_g2()[1])
