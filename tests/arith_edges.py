"""Adversarial test vectors for the device field and curve arithmetic (tests/test_gpu_arith_edges.py), and the big-integer expectations they are
checked against.  Bounds, bias multiples and exact limb algorithms come from the limb models (tools/u29_model.py for Fp, tools/u29_ntt_model.py
for Fr) so the vectors follow the models when they change.  Every generator has a precondition check (`*_pre`); tests/test_arith_probe_cpu.py
runs them all, so a device mismatch always points at the kernel, never at the generator."""
import contextlib
import hashlib
import io
import os
import random
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import u29_model as M  # noqa: E402
import u29_ntt_model as MR  # noqa: E402
from oracle import bn254_ref as ref  # noqa: E402

P, R = ref.Q, ref.R
MASK, NL = M.MASK, M.NL
WMAX = MASK + 8           # largest limb 0..7 of a weakly normalised value (u29_wnorm: "below 2^29 + 8")
RINV = pow(1 << 256, -1, P)
R29INV = pow(1 << M.RBITS, -1, P)

# the proven bounds, read off the models (bound propagation only prints)
with contextlib.redirect_stdout(io.StringIO()):
    _FP_G1 = M.fixed_point(M.madd_fp, False)
    _FP_G2 = M.fixed_point(M.madd_fp2_fused, True)
G1_MADD_BOUNDS = [b.vmax for b in _FP_G1]                          # X < 13.2 p, Y, ZZ, ZZZ < 2 p
G2_MADD_BOUNDS = [max(b[0].vmax, b[1].vmax) for b in _FP_G2]
TAIL_BOUND = 32 * P                                                # the add / dbl class of check_add_dbl_class(_g2)
STORE_MAX = (1 << 260) - 1                                         # u29_store: any lazily reduced value < 2^260
FP_KS = [4, 8, 12, 16, 24, 32, 40, 64, 80]                         # every u29_sub / u29_neg multiple the kernels instantiate
FR_KS = [4, 16, 24, 40]


# ------------------------------------------------------------------------------------------------------------ words and limbs
def words(x, n=8):
    assert 0 <= x < 1 << (32 * n)
    return [(x >> (32 * i)) & 0xffffffff for i in range(n)]


def unwords(w):
    return sum(int(v) << (32 * i) for i, v in enumerate(w))


def limbs(x):
    return M.limbs(x)


def val(l):
    return M.val([int(v) for v in l])


def weak_max(bound):
    """limbs 0..7 all at WMAX, the top limb as large as keeps the value below `bound`"""
    low = val([WMAX] * (NL - 1) + [0])
    top = (bound - 1 - low) >> (29 * (NL - 1))
    l = [WMAX] * (NL - 1) + [top]
    assert val(l) < bound
    return l


def weak_rand(rng, bound):
    while True:
        l = [rng.randrange(WMAX + 1) for _ in range(NL - 1)]
        top_max = (bound - 1 - val(l + [0])) >> (29 * (NL - 1))
        if top_max >= 0:
            return l + [rng.randrange(top_max + 1)]


def is_weak(l, bound):
    return all(0 <= v <= WMAX for v in l[:-1]) and 0 <= l[-1] < 1 << 32 and val(l) < bound


def canon_edges(m):
    top = m >> 224
    return [0, 1, 2, m - 1, m - 2, (m - 1) // 2, (1 << 256) % m, (1 << 512) % m, (1 << 224) - 1, ((top - 1) << 224) | ((1 << 224) - 1)]


def canon_vals(rng, m, n):
    v = canon_edges(m)
    return v + [rng.randrange(m) for _ in range(n - len(v))]


def lazy_vals(bound):
    """values a lazily reduced operand can take at the top of its range: multiples of p, their neighbours, bound - 1"""
    out = [0, 1, P - 1, P, P + 1, 2 * P - 1, bound - 1]
    out += [k * P for k in range(1, 32) if k * P < bound] + [k * P - 1 for k in range(1, 33) if k * P - 1 < bound]
    return sorted(set(v for v in out if 0 <= v < bound))


def u29_operands(rng, bound, n):
    """weakly normalised operands < bound: normalised edge values, all-limbs-at-maximum forms, random limbs"""
    ops = [limbs(v) for v in lazy_vals(bound)] + [weak_max(bound)]
    while len(ops) < n:
        ops.append(weak_rand(rng, bound) if rng.random() < 0.6 else limbs(rng.randrange(bound)))
    return ops[:n]


# ------------------------------------------------------------------------------------------------------------ 29-bit op vectors
# Each generator returns (input word lists, expected raw output word lists, precondition check).  Expectations are the model's exact limb
# algorithms, so a mismatch that is still right mod p means the asm and the proof diverged.
def ripple(l):
    out, c = [], 0
    for i in range(NL - 1):
        t = l[i] + c
        assert t < 1 << 32
        out.append(t & MASK)
        c = t >> 29
    out.append(l[-1] + c)
    assert out[-1] < 1 << 32
    return out


def mul_pre(*ops):
    """column sums < 2^64 and a top limb < 2^32: the model's exact algorithm asserts both"""
    pairs = list(zip(ops[0::2], ops[1::2]))
    M.mulN_exact(pairs)
    return True


def u29_mul_vectors(rng, n):
    a = u29_operands(rng, TAIL_BOUND, n)
    b = u29_operands(rng, TAIL_BOUND, n)
    rng.shuffle(b)
    return [x + y for x, y in zip(a, b)], [M.mul_exact(x, y) for x, y in zip(a, b)], [(x, y) for x, y in zip(a, b)]


def mulN_vectors(rng, n, N, bound):
    ops = [u29_operands(rng, bound, n) for _ in range(2 * N)]
    for o in ops[1:]:
        rng.shuffle(o)
    vin, vout, pre = [], [], []
    for k in range(n):
        pairs = [(ops[2 * t][k], ops[2 * t + 1][k]) for t in range(N)]
        vin.append(sum((x + y for x, y in pairs), []))
        vout.append(M.mulN_exact(pairs))
        pre.append(sum(pairs, ()))
    return vin, vout, pre


def dominated(rng, bias, n):
    """weakly normalised subtrahends whose limbs the bias dominates limb by limb (the model's b_sub / neg precondition): the all-maximum form
    (just under K p), normalised values just under it, random limbs"""
    top = bias[-1]
    out = [[WMAX] * (NL - 1) + [top], limbs((top << 232) | ((1 << 232) - 1)), limbs(top << 232), [0] * NL]
    while len(out) < n:
        out.append([rng.randrange(WMAX + 1) for _ in range(NL - 1)] + [rng.randrange(top + 1)])
    return out


def sub_vectors(rng, n, K):
    """a - b + K p: b up to the largest subtrahend K p dominates; a any weakly normalised tail-class value"""
    bs = dominated(rng, M.bias_limbs(K), n)
    as_ = u29_operands(rng, TAIL_BOUND, n)
    return [x + y for x, y in zip(as_, bs)], [M.sub_exact(x, y, M.bias_limbs(K)) for x, y in zip(as_, bs)], list(zip(as_, bs))


def sub_pre(a, b, K, model=M):
    mod = model.Q if model is M else model.P
    bias = model.bias_limbs(K)
    return (all(v <= WMAX for v in b[:-1]) and val(b) < K * mod and all(x <= z for x, z in zip(b, bias))
            and all(x + z < 1 << 32 for x, z in zip(a, bias)))


def store_inputs(rng, n):
    """u29_store's domain, any lazily reduced value < 2^260: multiples of p and their neighbours up to the top, the all-maximum form, random limbs"""
    xs = [limbs(v) for v in lazy_vals(STORE_MAX + 1)] + [limbs(k * P) for k in range(32, STORE_MAX // P + 1)]
    xs += [limbs(STORE_MAX), limbs(STORE_MAX - P), weak_max(STORE_MAX + 1)] + [limbs(v) for v in range(P, 4 * P, P // 7)]
    while len(xs) < n:
        xs.append(weak_rand(rng, STORE_MAX + 1))
    return xs


def neg_expect(a, K):
    return M.wnorm_exact(M.sub_exact(M.bias_limbs(K), a, [0] * NL))


# ------------------------------------------------------------------------------------------------------------ Fp2 / F6 / F12 (gnark's tower)
XI = (9, 1)
f2m, f2a, f2s, f2i = ref.f2_mul, ref.f2_add, ref.f2_sub, ref.f2_inv
F2_0, F2_1 = (0, 0), (1, 0)


def f6_mul(a, b):  # schoolbook, v^3 = xi
    c = [F2_0] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = f2a(c[i + j], f2m(a[i], b[j]))
    return (f2a(c[0], f2m(XI, c[3])), f2a(c[1], f2m(XI, c[4])), c[2])


def f6_add(a, b): return tuple(f2a(x, y) for x, y in zip(a, b))
def f6_sub(a, b): return tuple(f2s(x, y) for x, y in zip(a, b))
def f6_mulv(a): return (f2m(XI, a[2]), a[0], a[1])


def f6_inv(a):
    b0, b1, b2 = a
    t0 = f2s(f2m(b0, b0), f2m(XI, f2m(b1, b2)))
    t1 = f2s(f2m(XI, f2m(b2, b2)), f2m(b0, b1))
    t2 = f2s(f2m(b1, b1), f2m(b0, b2))
    d = f2i(f2a(f2m(b0, t0), f2m(XI, f2a(f2m(b2, t1), f2m(b1, t2)))))
    r = (f2m(t0, d), f2m(t1, d), f2m(t2, d))
    assert f6_mul(a, r) == (F2_1, F2_0, F2_0)
    return r


F6_1 = (F2_1, F2_0, F2_0)
F6_0 = (F2_0, F2_0, F2_0)
F12_1 = (F6_1, F6_0)


def f12_mul(a, b):  # w^2 = v
    return (f6_add(f6_mul(a[0], b[0]), f6_mulv(f6_mul(a[1], b[1]))), f6_add(f6_mul(a[0], b[1]), f6_mul(a[1], b[0])))


def f12_conj(a): return (a[0], tuple(ref.f2_neg(x) for x in a[1]))


def f12_inv(a):
    d = f6_inv(f6_sub(f6_mul(a[0], a[0]), f6_mulv(f6_mul(a[1], a[1]))))
    r = (f6_mul(a[0], d), tuple(ref.f2_neg(x) for x in f6_mul(a[1], d)))
    assert f12_mul(a, r) == F12_1
    return r


def f12_pow(a, e):
    out = F12_1
    while e:
        if e & 1:
            out = f12_mul(out, a)
        a = f12_mul(a, a)
        e >>= 1
    return out


def f2_pow(a, e):
    out = F2_1
    while e:
        if e & 1:
            out = f2m(out, a)
        a = f2m(a, a)
        e >>= 1
    return out


FROB_G1 = [f2_pow(XI, i * (P - 1) // 6) for i in range(6)]
FROB_G2 = [f2_pow(XI, i * (P * P - 1) // 6) for i in range(6)]
assert all(g[1] == 0 for g in FROB_G2)


def rand_f2(rng): return (rng.randrange(P), rng.randrange(P))
def rand_f6(rng): return tuple(rand_f2(rng) for _ in range(3))
def rand_f12(rng): return (rand_f6(rng), rand_f6(rng))


def cyclotomic(f):
    """f^((p^6 - 1)(p^2 + 1)): the image of the easy part, where cyc_sqr applies"""
    g = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_pow(g, P * P), g)


# memory images (Montgomery 2^256, canonical)
def img(x): return words((x << 256) % P)
def unimg(w): return unwords(w) * RINV % P
def img2(a): return img(a[0]) + img(a[1])
def img6(a): return sum((img2(x) for x in a), [])
def img12(a): return img6(a[0]) + img6(a[1])


def unimg2(w): return (unimg(w[0:8]), unimg(w[8:16]))
def unimg6(w): return tuple(unimg2(w[16 * i:16 * i + 16]) for i in range(3))
def unimg12(w): return (unimg6(w[0:48]), unimg6(w[48:96]))


# ------------------------------------------------------------------------------------------------------------ points
def g1_point(rng):
    while True:
        x = rng.randrange(P)
        rhs = (x * x * x + 3) % P
        y = pow(rhs, (P + 1) // 4, P)
        if y * y % P == rhs:
            return (x, y)


def g2_points(n, seed):
    """n distinct points of the G2 subgroup: k G, (k + 1) G, ..."""
    pt = ref.g2_mul(ref.G2_GEN, seed)
    out = []
    for _ in range(n):
        out.append(pt)
        pt = ref.g2_add(pt, ref.G2_GEN)
    return out


def xyzz_of(F, pt, z):
    """(x z^2, y z^3, z^2, z^3) for an affine point, infinity as all zero"""
    if pt is None:
        return (F.zero,) * 4
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    return (F.mul(pt[0], zz), F.mul(pt[1], zzz), zz, zzz)


def affine_of(F, c):
    x, y, zz, zzz = c
    if F.is_zero(zz):
        return None
    return (F.mul(x, F.inv(zz)), F.mul(y, F.inv(zzz)))


# lazily reduced accumulator coordinates: value x * 2^261 mod p, plus k p for the largest k the bound allows
def lazy29(x, bound, rng=None):
    v = (x << M.RBITS) % P
    k = (bound - 1 - v) // P
    if rng is not None:
        k = rng.randrange(k + 1) if rng.random() < 0.3 else k
    l = limbs(v + k * P)
    assert val(l) < bound
    return l


def from29(l): return val(l) * R29INV % P


# ------------------------------------------------------------------------------------------------------------ SHA-256
_K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3,
      0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13,
      0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
      0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
SHA_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def sha256_midstate(data):
    """the chaining value after len(data) bytes (a multiple of 64), FIPS 180-4 -- only to build resume() vectors; digests come from hashlib"""
    assert len(data) % 64 == 0
    rot = lambda x, n: ((x >> n) | (x << (32 - n))) & 0xffffffff
    h = list(SHA_IV)
    for off in range(0, len(data), 64):
        w = list(struct.unpack(">16I", data[off:off + 64]))
        for i in range(16, 64):
            s0 = rot(w[i - 15], 7) ^ rot(w[i - 15], 18) ^ (w[i - 15] >> 3)
            s1 = rot(w[i - 2], 17) ^ rot(w[i - 2], 19) ^ (w[i - 2] >> 10)
            w.append((w[i - 16] + s0 + w[i - 7] + s1) & 0xffffffff)
        a, b, c, d, e, f, g, hh = h
        for i in range(64):
            t1 = (hh + (rot(e, 6) ^ rot(e, 11) ^ rot(e, 25)) + ((e & f) ^ (~e & g)) + _K[i] + w[i]) & 0xffffffff
            t2 = ((rot(a, 2) ^ rot(a, 13) ^ rot(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & 0xffffffff
            hh, g, f, e, d, c, b, a = g, f, e, (d + t1) & 0xffffffff, c, b, a, (t1 + t2) & 0xffffffff
        h = [(x + y) & 0xffffffff for x, y in zip(h, [a, b, c, d, e, f, g, hh])]
    assert len(data) != 0 or h == SHA_IV
    return h


SHA_MAX = 320


def sha_record(mode, msg, piece=1, offset=0, mid=(0,) * 8, count=None):
    buf = bytes(msg) + bytes(SHA_MAX - len(msg))
    return [mode, len(msg) if count is None else count, piece, offset] + list(mid) + list(struct.unpack("<%dI" % (SHA_MAX // 4), buf))


def sha_words(digest):
    return list(struct.unpack(">8I", digest))


def sha_vectors(seed=5):
    """(records, expected digest words, label): every length 0..300 in odd pieces, resumption at 64 and 128, put256 of 0..9 integers"""
    rng = random.Random(seed)
    recs, exp, lab = [], [], []
    pieces = [1, 3, 7, 13, 31, 55, 64, 65, 300]
    for L in range(0, 301):
        msg = bytes(rng.randrange(256) for _ in range(L))
        pc = pieces[L % len(pieces)]
        recs.append(sha_record(0, msg, piece=pc))
        exp.append(sha_words(hashlib.sha256(msg).digest()))
        lab.append("len %d piece %d" % (L, pc))
        for cut in (64, 128):
            if L >= cut:
                recs.append(sha_record(1, msg[cut:], offset=cut, mid=sha256_midstate(msg[:cut])))
                exp.append(sha_words(hashlib.sha256(msg).digest()))
                lab.append("len %d resumed at %d" % (L, cut))
    for j in range(10):
        ints = [rng.randrange(1 << 256) for _ in range(j)]
        if j:
            ints[0] = (1 << 256) - 1
        recs.append([2, 32 * j, 1, 0] + [0] * 8 + sum((words(v) for v in ints), []) + [0] * (SHA_MAX // 4 - 8 * j))
        exp.append(sha_words(hashlib.sha256(b"".join(v.to_bytes(32, "big") for v in ints)).digest()))
        lab.append("put256 x %d" % j)
    return recs, exp, lab
