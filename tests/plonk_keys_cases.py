"""Material for the many-key PLONK batch verifier (zk_bn254_plonk_verify_batch_keys): rows of (case, the key the row is verified against) built from
tests/plonk_forge.py, whose toy keys all sit under one tau and so share srs_g2.  A row's expected verdict is the case's own when it meets its own key and 0
under any other key; tests/test_plonk_verify_keys_cpu.py holds both against the host verifier.  Nothing here asks the device."""
import ctypes as C
import functools

import numpy as np

from noir_backend_using_gnark_amd import _lib
from tests import plonk_forge as pf

R, TAU = pf.R, pf.TAU


@functools.lru_cache(None)
def np1_keys():
    """every key of pf.KEY_NAMES with one public input: the nine with points at infinity (S1 and S2 among them), Ql = Qr, n_public 1, log_n 1 2 16 24 28"""
    ks = pf.infinity_keys() + [pf.double_key(), pf.n_public_key(1)] + [pf.log_n_key(n) for n in pf.LOG_N]
    assert len(ks) == 16 and all(k.n_public == 1 and k.name in pf.KEY_NAMES for k in ks) and len({k.bytes for k in ks}) == 16
    return ks


@functools.lru_cache(None)
def accepts_of(key):
    if key.name in pf.key_accepts():
        cs = pf.key_accepts()[key.name]
    elif key.name.startswith("log_n "):
        cs = pf.log_n_cases(key.log_n)
    elif key.name.startswith("n_public "):
        cs = pf.n_public_cases(key.n_public)
    else:
        assert key is pf.base_key()
        cs = pf.good_cases(key, 8)
    assert all(c.key is key and c.expect == 1 for c in cs)
    return list(cs)


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
    """an accept of key j of np1_keys() pointed at key j + 1 (rows 0..15), then at key j - 1 (rows 16..31): the same n_public, another key"""
    ks = np1_keys()
    return [(accepts_of(k)[0], ks[(j + d) % len(ks)]) for d in (1, -1) for j, k in enumerate(ks)]


@functools.lru_cache(None)
def cross_key_pairs():
    """pf.cancelling_pairs() across keys: W_1 + d_1 G under key A, W_2 + d_2 G under key B, d_2 = -d_1 (zeta_1 - tau) / (zeta_2 - tau).  The error of a lane
    is rho d (zeta - tau) G whatever its key is, so the two cancel when the lanes share their coefficient"""
    by = {k.name: k for k in np1_keys()}
    out = []
    for i, (na, nb) in enumerate((("S1 at infinity", "Ql = Qr"), ("Ql = Qr", "log_n 16"), ("log_n 16", "S2 at infinity"))):
        ga, gb = pf.Forge(by[na], 0xC4A0 + i), pf.Forge(by[nb], 0xC4B0 + i)
        d1, d2 = ga.draft(), gb.draft()
        assert d1.zeta != d2.zeta
        dl1 = ga.f()
        dl2 = -dl1 * (d1.zeta - TAU) % R * pf.inv(d2.zeta - TAU) % R
        assert (dl1 * (d1.zeta - TAU) + dl2 * (d2.zeta - TAU)) % R == 0 and dl2
        out.append(pf.Pair("cross-key pair %d" % i, [d1.finish("cross-key pair %d: W_1 + d_1 G" % i, d1.with_lin_z(ga.free()), "opening", dw=dl1),
                                                      d2.finish("cross-key pair %d: W_2 + d_2 G" % i, d2.with_lin_z(gb.free()), "opening", dw=dl2)]))
    return out


MANY = 300


@functools.lru_cache(None)
def many_keys():
    """[(key, an accept of it)]: MANY freshly made keys of 8 rows and one public input, and an opening reject of the last"""
    f = pf._rng(0x300C)
    out = []
    for j in range(MANY):
        k = pf.ToyKey("many %d" % j, 3, 1, {p: f() for p in pf.KEY_POINTS})
        out.append((k, pf.Forge(k, 0x3000 + j).good("accept")))
    assert len({k.bytes for k, _ in out}) == MANY
    return out, pf.opening_reject(out[-1][0])


# ---------------------------------------------------------------------------------------------------------------- a batch as the C entry takes it
class Batch:
    """rows [(case, key)] -> the distinct keys in order of first use (extra: keys given but not referred to, in front), key_of, the proofs, the public inputs
    at `stride` elements per row with `fill` (a uint64, or an rng for garbage that differs per call) behind each row's own, the expected verdicts"""

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
                out[i, :k.n_public] = pf.plus_r(c.pub) if wide else c.pub
        return out

    def key_args(self):
        """(char*[K], size_t[K]) of the keys' bytes"""
        raw = [k.bytes for k in self.keys]
        return (C.c_char_p * len(raw))(*raw), (C.c_size_t * len(raw))(*[len(b) for b in raw])


def call_host_form(b, pubs, key_of=None):
    """zk_bn254_plonk_verify_batch_keys itself, its output buffers poisoned -> (rc, accepted bytes, *n_accepted)"""
    acc, n_acc = np.full(max(b.n, 1), 0xEE, np.uint8), C.c_size_t(1 << 40)
    ptrs, lens = b.key_args()
    g2 = np.ascontiguousarray(pf.srs_g2()[1], dtype=np.uint64)
    ko = np.ascontiguousarray(b.key_of if key_of is None else key_of, dtype=np.uint32)
    pubs = np.ascontiguousarray(pubs, dtype=np.uint64)
    rc = _lib.lib().zk_bn254_plonk_verify_batch_keys(b.blob, b.n, ptrs, lens, len(b.keys), 0, _lib.vp(g2), _lib.vp(ko), _lib.vp(pubs) if pubs.size else None,
                                                     pubs.shape[1], _lib.vp(acc), C.addressof(n_acc))
    return rc, acc[:b.n], n_acc.value
