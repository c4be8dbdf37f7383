"""The row-batched openings of PLONK's rounds 4 and 5 (csrc/plonk.hip poly_open_rows_dev, linearize_rows_dev, open_rows_dev over scan.hpp's pass bodies) through
zk_bn254_fr_poly_open_rows_dev, zk_bn254_plonk_linearize_batch_dev, zk_bn254_plonk_open_batch_dev and their Python doors  (-m gpu).  Everything is bit-exact.

The ingredient: lengths 1, 2, 8 (one lane), 9 (a lane boundary), 2047, 2048 (256 lanes exactly), 2049 (257 lanes: the second workgroup holds one), 2050 and
2^16 + 3 (33 workgroups), and 2^21 + 3, the first length whose plan has K = 9 (911 workgroups); 1, 2, 3 and 5 rows with gaps in every stride; evaluate-only,
disjoint and in-place; points 0, 1, R - 1 and random.  Its expectation is Python Horner on the Montgomery images themselves: with the coefficients' images and
the point's value, the recurrence yields the images of the results.
The two key entries at 2^2, 2^3, 2^6, 2^9, 2^10, 2^11 (s1 and s2 fill one workgroup exactly while l, r, o and z need a second), 2^12 and one row at 2^16: rows are
the pool of tests/plonk_open_ref.py; the h of a row is the device's own quotient (zk_bn254_plonk_quotient_batch_dev, held against Python by
tests/test_gpu_plonk_quotient.py), the expectation tests/plonk_open_ref.py (held against the oracle prover by tests/test_plonk_open_cpu.py)."""
import ctypes as C
import random

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import kzg as zkzg
from noir_backend_using_gnark_amd import plonk as zp
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_open_ref as po
from tests import plonk_quotient_ref as qr

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
SENTINEL = qr.SENTINEL
LOG_N = (2, 3, 6, 9, 10, 11, 12)
ROW_COUNTS = (1, 2, 3, 5)
LENGTHS = (1, 2, 8, 9, 2047, 2048, 2049, 2050, (1 << 16) + 3)
BIG_LEN = (1 << 21) + 3
BIG = 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback
    yield
    for k in list(_keys):
        key = _keys.pop(k)
        key["pk"].free()
        key["rb"].free()


class _Dev:
    """device buffers that are freed together"""

    def __init__(self):
        self.bufs = []

    def up(self, a):
        self.bufs.append(_lib.DeviceBuffer.from_numpy(a))
        return self.bufs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _strided(rows, stride):
    """rows of (k, 4) images at `stride` elements, sentinels in the gaps and one behind the end"""
    out = np.tile(SENTINEL, (len(rows) * stride + 1, 1))
    for v, r in enumerate(rows):
        out[v * stride:v * stride + len(r)] = r
    return out


def _check_rows(got, want_rows, stride, what, base=None):
    """`got` holds want_rows[v] at v * stride and, everywhere else, what `base` held there (sentinels when None)"""
    free = np.ones(got.shape[0], dtype=bool)
    for v, w in enumerate(want_rows):
        assert (got[v * stride:v * stride + len(w)] == w).all(), what + ("row", v)
        free[v * stride:v * stride + len(w)] = False
    assert (got[free] == (SENTINEL if base is None else base[free])).all(), what + ("untouched",)


# ---------------------------------------------------------------------------------------------------- the ingredient
def _raw(a):
    """(k, 4) uint64 -> the k 256-bit integers the limbs spell (the Montgomery images as they are)"""
    b = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(len(a))]


def _raw_np(ints):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _random_images(rng, count):
    """canonical images: four random limbs with the top one below the modulus's"""
    a = rng.integers(0, 1 << 63, size=(count, 4), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(count, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=count, dtype=np.uint64)
    return a


def _horner(f, a):
    """po.open_at on images: f the images' integers, a the point's value"""
    return po.open_at(f, a)


_poly = {}


def _ingredient_rows(length):
    """five rows of `length` random coefficients with the points random, 0, 1, R - 1, random: (images, points, expected value image, expected quotient images)"""
    if length not in _poly:
        rng = np.random.default_rng(0x0A11 + length)
        g = random.Random(0x0B22 + length)
        rows = []
        for a in (g.randrange(R), 0, 1, R - 1, g.randrange(R)):
            img = _random_images(rng, length)
            value, q = _horner(_raw(img), a)
            img.setflags(write=False)
            rows.append((img, a, _raw_np([value]), _raw_np(q) if q else np.zeros((0, 4), np.uint64)))
        _poly[length] = rows
    return _poly[length]


def _open_dev(f, in_stride, length, rows, pts, q, q_stride, values):
    return _lib.lib().zk_bn254_fr_poly_open_rows_dev(C.c_void_p(f), C.c_size_t(in_stride), C.c_size_t(length), C.c_size_t(rows), C.c_void_p(pts), C.c_void_p(q),
                                                     C.c_size_t(q_stride), C.c_void_p(values), None)


@pytest.mark.parametrize("length", LENGTHS)
def test_ingredient_every_row_count_stride_and_form(length):
    """1, 2, 3, 5 rows (the one-row call at every point) at strides at their minimum and above; evaluate-only, disjoint and in place: values and quotients
    equal Python Horner, the gaps, the ends, element length - 1 of an in-place row and the inputs are as they were"""
    pool = _ingredient_rows(length)
    for idx in [[j] for j in range(5)] + [qr.rows_of(k) for k in ROW_COUNTS[1:]]:
        rows = len(idx)
        sel = [pool[j] for j in idx]
        pts = np.concatenate([M([a]) for _, a, _, _ in sel] + [SENTINEL[None]])
        for in_stride, q_stride in ((length, max(length - 1, 0)), (length + 3, length + 1)):
            if rows == 1 and in_stride != length and length > 9:
                continue
            f = _strided([r[0] for r in sel], in_stride)
            want_v = [r[2] for r in sel]
            for form in ("evaluate", "disjoint", "in place"):
                what = (length, rows, in_stride, form)
                with _Dev() as d:
                    df, dp = d.up(f), d.up(pts)
                    dv = d.up(np.tile(SENTINEL, (rows + 1, 1)))
                    dq = d.up(np.tile(SENTINEL, (rows * q_stride + 1, 1))) if form == "disjoint" else None
                    q_ptr, qs = {"evaluate": (0, 0), "disjoint": (dq.ptr if dq else 0, q_stride), "in place": (df.ptr, in_stride)}[form]
                    _lib.check(_open_dev(df.ptr, in_stride, length, rows, dp.ptr, q_ptr, qs, dv.ptr))
                    _check_rows(dv.to_numpy(np.uint64, (rows + 1, 4)), want_v, 1, what + ("values",))
                    assert (dp.to_numpy(np.uint64, pts.shape) == pts).all(), what
                    after = df.to_numpy(np.uint64, f.shape)
                    if form == "in place":
                        _check_rows(after, [r[3] for r in sel], in_stride, what + ("q",), base=f)
                    else:
                        assert (after == f).all(), what + ("input",)
                    if form == "disjoint":
                        _check_rows(dq.to_numpy(np.uint64, (rows * q_stride + 1, 4)), [r[3] for r in sel], q_stride, what + ("q",))


def test_ingredient_at_the_first_length_with_nine_coefficients_a_lane():
    """2^21 + 3 coefficients: K = 9, 911 workgroups.  The value against Python Horner; q by the recurrence q[i - 1] = f[i] + a q[i] at every lane and workgroup
    boundary and at 300 random indices, and q[len - 2] = f[len - 1]"""
    length = BIG_LEN
    K = max(8, -(-length // (1 << 18)))
    assert K == 9 and -(-(-(-length // K)) // 256) == 911
    rng = np.random.default_rng(0xB16)
    img = _random_images(rng, length)
    a = random.Random(0xB17).randrange(R)
    f = _raw(img)
    value = 0
    for c in reversed(f):
        value = (c + a * value) % R
    with _Dev() as d:
        df, dp = d.up(img), d.up(M([a]))
        dv, dq = d.up(np.tile(SENTINEL, (2, 1))), d.up(np.tile(SENTINEL, (length, 1)))
        _lib.check(_open_dev(df.ptr, length, length, 1, dp.ptr, dq.ptr, length - 1, dv.ptr))
        got_v, q = dv.to_numpy(np.uint64, (2, 4)), dq.to_numpy(np.uint64, (length, 4))
        assert (df.to_numpy(np.uint64, img.shape) == img).all()
    assert _raw(got_v) == [value, _raw(SENTINEL[None])[0]] and (q[length - 1] == SENTINEL).all()
    assert (q[length - 2] == img[length - 1]).all()
    at = {i for i in range(K, length - 1, K)} | {1, 2, length - 2}
    at |= {random.Random(0xB18 + k).randrange(1, length - 1) for k in range(300)}
    idx = np.array(sorted(at))
    qi, qm, fi = _raw(q[idx]), _raw(q[idx - 1]), _raw(img[idx])
    wrong = [int(i) for i, x, y, c in zip(idx, qi, qm, fi) if y != (c + a * x) % R]
    assert wrong == []


def test_ingredient_python_door_host_and_device_forms():
    rows = _ingredient_rows(2049)
    f, pts = np.ascontiguousarray(np.stack([r[0] for r in rows])), np.ascontiguousarray(np.concatenate([M([r[1]]) for r in rows]))
    values, q = zk.poly_open_rows(f, pts)
    assert values.shape == (5, 4) and q.shape == (5, 2048, 4)
    for v, r in enumerate(rows):
        assert (values[v] == r[2][0]).all() and (q[v] == r[3]).all()
    v2, none = zk.poly_open_rows(f, pts, divide=False, rows=5, length=2049)
    assert none is None and (v2 == values).all()
    with _Dev() as d:
        df, dp = d.up(f), d.up(pts)
        dv, dq = zp.poly_open_rows(df, dp, rows=5, length=2049)
        try:
            assert (dv.to_numpy(np.uint64, (5, 4)) == values).all() and (dq.to_numpy(np.uint64, (5, 2048, 4)) == q).all()
        finally:
            dv.free()
            dq.free()
        mine = d.up(np.tile(SENTINEL, (5, 1)))
        got = zp.poly_open_rows(df, dp, rows=5, length=2049, out=df, values=mine)
        assert got == (mine, df) and (mine.to_numpy(np.uint64, (5, 4)) == values).all()
        after = df.to_numpy(np.uint64, f.shape)
        assert (after[:, :2048] == q).all() and (after[:, 2048] == f[:, 2048]).all()


# ---------------------------------------------------------------------------------------------------- keys, rows and expectations, computed once
_keys, _rows = {}, {}
IN_KEYS = ("bl", "br", "bo", "bz", "h", "alpha", "beta", "gamma", "zeta")
OUT_KEYS = ("values", "zquot", "lin", "fh")


def _circuit(spr) -> zp.Circuit:
    g = spr.constraints
    col = lambda k: M([c[k] for c in g])
    return zp.Circuit(spr.n_public, spr.n_vars, col(0), col(1), col(2), col(3), col(4), [c[5] for c in g], [c[6] for c in g], [c[7] for c in g])


def _device_key(spr, n):
    rb = zb.ResidentBases(orc.g1_gen_points(0x9F0 + n, n + 3))
    return zp.setup(_circuit(spr), rb), rb


def _key(log_n):
    if log_n not in _keys:
        n = 1 << log_n
        spr, n_in = qr.forward_circuit(n, 1, 0x7C0 + 64 + log_n)
        pk, rb = _device_key(spr, n)
        assert pk.domain_size == n
        _keys[log_n] = dict(spr=spr, n_in=n_in, n=n, keep=3 * (n + 2), opk=qr.setup_polys(spr, fast=True), pk=pk, rb=rb)
    return _keys[log_n]


def _device_h(key, row):
    one = lambda v: np.ascontiguousarray(M(v)[None])
    h, status = key["pk"].quotient_batch(one(row["bl"]), one(row["br"]), one(row["bo"]), one(row["bz"]), one(row["public"]), M([row["alpha"]]), M([row["beta"]]),
                                         M([row["gamma"]]))
    assert status.tolist() == [row["violated"]]
    return pl.mont_np_to_ints(h[0])


def _row(log_n, j):
    """pool row j of the key: (integers with the expected outputs, Montgomery images of inputs and outputs)"""
    if (log_n, j) not in _rows:
        key = _key(log_n)
        seed = 0xD00 + 16 + log_n
        base = qr.pool_row(key["opk"], key["n_in"], j, seed, fast=True)
        row = po.pool_row(key["opk"], key["n_in"], j, seed, fast=True, h=_device_h(key, base))
        img = {k: M(row[k]) for k in ("bl", "br", "bo", "bz", "h", "values", "zquot", "lin", "fh", "q")}
        img.update({k: M([row[k]]) for k in ("alpha", "beta", "gamma", "zeta", "kzg_gamma", "value")})
        for v in img.values():
            v.setflags(write=False)
        _rows[(log_n, j)] = (row, img)
    return _rows[(log_n, j)]


def _lin_call(key, p, in_stride, h_stride, rows, out_stride):
    p = [C.c_void_p(v) for v in p]
    return _lib.lib().zk_bn254_plonk_linearize_batch_dev(key["pk"].handle, p[0], p[1], p[2], p[3], C.c_size_t(in_stride), p[4], C.c_size_t(h_stride), C.c_size_t(rows),
                                                         p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12], C.c_size_t(out_stride), None)


def _lin_arrays(imgs, in_stride, h_stride, out_stride):
    rows = len(imgs)
    ins = [_strided([im[k] for im in imgs], in_stride) for k in ("bl", "br", "bo", "bz")] + [_strided([im["h"] for im in imgs], h_stride)]
    ch = [np.concatenate([im[k] for im in imgs] + [SENTINEL[None]]) for k in ("alpha", "beta", "gamma", "zeta")]
    outs = [np.tile(SENTINEL, (rows * 8 + 1, 1))] + [np.tile(SENTINEL, (rows * out_stride + 1, 1)) for _ in range(3)]
    return ins + ch + outs


def _lin_dev(key, imgs, in_stride=None, h_stride=None, out_stride=None):
    """-> the four output buffers as they are afterwards; asserts that the inputs, gaps included, are unchanged"""
    n = key["n"]
    in_stride, h_stride, out_stride = in_stride or n + 3, h_stride or key["keep"], out_stride or n + 3
    host = _lin_arrays(imgs, in_stride, h_stride, out_stride)
    with _Dev() as d:
        bufs = [d.up(a) for a in host]
        _lib.check(_lin_call(key, [b.ptr for b in bufs], in_stride, h_stride, len(imgs), out_stride))
        for buf, a in zip(bufs[:9], host[:9]):
            assert (buf.to_numpy(np.uint64, a.shape) == a).all(), "an input changed"
        return [b.to_numpy(np.uint64, a.shape) for b, a in zip(bufs[9:], host[9:])]


def _lin_check(got, imgs, out_stride, what):
    for k, g, stride in zip(OUT_KEYS, got, (8, out_stride, out_stride, out_stride)):
        _check_rows(g, [im[k] for im in imgs], stride, what + (k,))


def _open_call(key, p, in_stride, rows, out_stride):
    p = [C.c_void_p(v) for v in p]
    return _lib.lib().zk_bn254_plonk_open_batch_dev(key["pk"].handle, p[0], p[1], p[2], p[3], p[4], C.c_size_t(in_stride), C.c_size_t(rows), p[5], p[6], p[7],
                                                    C.c_size_t(out_stride), p[8], None)


def _open_arrays(imgs, in_stride, out_stride):
    rows = len(imgs)
    ins = [_strided([im[k] for im in imgs], in_stride) for k in ("fh", "lin", "bl", "br", "bo")]
    ch = [np.concatenate([im[k] for im in imgs] + [SENTINEL[None]]) for k in ("zeta", "kzg_gamma")]
    return ins + ch + [np.tile(SENTINEL, (rows * out_stride + 1, 1)), np.tile(SENTINEL, (rows + 1, 1))]


def _open_batch_dev(key, imgs, in_stride=None, out_stride=None):
    n = key["n"]
    in_stride, out_stride = in_stride or n + 3, out_stride or n + 2
    host = _open_arrays(imgs, in_stride, out_stride)
    with _Dev() as d:
        bufs = [d.up(a) for a in host]
        _lib.check(_open_call(key, [b.ptr for b in bufs], in_stride, len(imgs), out_stride))
        for buf, a in zip(bufs[:7], host[:7]):
            assert (buf.to_numpy(np.uint64, a.shape) == a).all(), "an input changed"
        return [b.to_numpy(np.uint64, a.shape) for b, a in zip(bufs[7:], host[7:])]


def _open_check(got, imgs, out_stride, what):
    _check_rows(got[0], [im["q"] for im in imgs], out_stride, what + ("q",))
    _check_rows(got[1], [im["value"] for im in imgs], 1, what + ("value",))


# ---------------------------------------------------------------------------------------------------- 2^2 .. 2^12
@pytest.mark.parametrize("log_n", LOG_N)
def test_linearize_every_row_count_and_stride(log_n):
    """1, 2, 3 and 5 rows at input, h and output strides at their minimum and one above: every row equals the restatement -- and hence its one-row call, made
    for every pool row as well; sentinels and inputs untouched"""
    key = _key(log_n)
    n, keep = key["n"], key["keep"]
    pool = [_row(log_n, j)[1] for j in range(po.POOL)]
    for j, im in enumerate(pool):
        _lin_check(_lin_dev(key, [im]), [im], n + 3, (log_n, "one row", j))
    for rows in ROW_COUNTS:
        imgs = [pool[j] for j in po.rows_of(rows)]
        for in_stride, h_stride, out_stride in ((n + 3, keep, n + 3), (n + 4, keep, n + 3), (n + 3, keep + 1, n + 3), (n + 3, keep, n + 4), (n + 5, keep + 2, n + 6)):
            _lin_check(_lin_dev(key, imgs, in_stride, h_stride, out_stride), imgs, out_stride, (log_n, rows, in_stride, h_stride, out_stride))


@pytest.mark.parametrize("log_n", LOG_N)
def test_open_every_row_count_and_stride(log_n):
    key = _key(log_n)
    n = key["n"]
    pool = [_row(log_n, j)[1] for j in range(po.POOL)]
    for j, im in enumerate(pool):
        _open_check(_open_batch_dev(key, [im]), [im], n + 2, (log_n, "one row", j))
    for rows in ROW_COUNTS:
        imgs = [pool[j] for j in po.rows_of(rows)]
        for in_stride, out_stride in ((n + 3, n + 2), (n + 4, n + 2), (n + 3, n + 3), (n + 5, n + 4)):
            _open_check(_open_batch_dev(key, imgs, in_stride, out_stride), imgs, out_stride, (log_n, rows, in_stride, out_stride))


# ---------------------------------------------------------------------------------------------------- against the device prover
@pytest.mark.parametrize("lagrange", (False, True))
@pytest.mark.parametrize("log_n", (6, 10, 12))
def test_values_and_quotients_are_the_device_provers(log_n, lagrange):
    """zp.prove with the five challenges of each satisfied pool row pinned: the batched values are bytes 260 .. 484 and 516 .. 548 of Proof.WriteTo, the
    commitments of zquot and q over the key's SRS bytes 484 .. 516 and 224 .. 256 -- with the key's Lagrange-form SRS absent and present"""
    key = _key(log_n)
    n, spr = key["n"], key["spr"]
    pk, rb = _device_key(spr, n) if lagrange else (key["pk"], key["rb"])
    try:
        if lagrange:
            pk.lagrange_srs()
        srs = zkzg.SRS(rb, None)
        commit = lambda a: ref.g1_compress(pl.g1_from_np(srs.commit(np.ascontiguousarray(a))))
        sat = [_row(log_n, j) for j in range(po.POOL) if j != 2]
        stack = lambda k: np.ascontiguousarray(np.stack([im[k] for _, im in sat]))
        cat = lambda k: np.ascontiguousarray(np.concatenate([im[k] for _, im in sat]))
        values, zquot, lin, fh = pk.linearize_batch(stack("bl"), stack("br"), stack("bo"), stack("bz"), stack("h"), cat("alpha"), cat("beta"), cat("gamma"), cat("zeta"))
        q, value = pk.open_batch(fh, lin, stack("bl"), stack("br"), stack("bo"), cat("zeta"), cat("kzg_gamma"))
        for v, (row, im) in enumerate(sat):
            pin = [row[k] for k in ("gamma", "beta", "alpha", "zeta", "kzg_gamma")]
            proof = zp.prove(pk, M(row["sol"]), M(row["blinders"]), challenges=M(pin))
            assert len(proof) == 548
            be = lambda a: b"".join(pl.fr_bytes(x) for x in pl.mont_np_to_ints(a))
            assert be(values[v, :7]) == proof[260:484] and be(values[v, 7:]) == proof[516:548], (log_n, v)
            assert commit(zquot[v]) == proof[484:516] and commit(q[v]) == proof[224:256], (log_n, v)
            assert (values[v] == im["values"]).all() and (q[v] == im["q"]).all() and (value[v] == im["value"][0]).all()
    finally:
        if lagrange:
            pk.free()
            rb.free()


# ---------------------------------------------------------------------------------------------------- chunks
def test_more_rows_than_one_launch_takes():
    """65,537 rows at n = 4, the pool's rows repeated: a launch takes 65,535, so two rows go in a second chunk.  Every row equals its pool row's expectation"""
    log_n, rows = 2, 65537
    key = _key(log_n)
    n, keep = key["n"], key["keep"]
    pool = [_row(log_n, j)[1] for j in range(po.POOL)]
    which = np.arange(rows) % po.POOL
    tile = lambda k, width: np.ascontiguousarray(np.stack([np.concatenate([im[k], np.tile(SENTINEL, (width - len(im[k]), 1))]) for im in pool])[which].reshape(-1, 4))
    ins = [tile(k, n + 3) for k in ("bl", "br", "bo", "bz")] + [tile("h", keep)] + [tile(k, 1) for k in ("alpha", "beta", "gamma", "zeta")]
    outs = [np.tile(SENTINEL, (rows * 8 + 1, 1))] + [np.tile(SENTINEL, (rows * (n + 3) + 1, 1)) for _ in range(3)]
    want = lambda k, width: np.stack([np.concatenate([im[k], np.tile(SENTINEL, (width - len(im[k]), 1))]) for im in pool])[which].reshape(-1, 4)
    with _Dev() as d:
        bufs = [d.up(a) for a in ins + outs]
        _lib.check(_lin_call(key, [b.ptr for b in bufs], n + 3, keep, rows, n + 3))
        got = [b.to_numpy(np.uint64, a.shape) for b, a in zip(bufs[9:], outs)]
        for k, g, width in zip(OUT_KEYS, got, (8, n + 3, n + 3, n + 3)):
            assert (g[:-1] == want(k, width)).all() and (g[-1] == SENTINEL).all(), k
        kg = d.up(tile("kzg_gamma", 1))
        oq, ov = d.up(np.tile(SENTINEL, (rows * (n + 2) + 1, 1))), d.up(np.tile(SENTINEL, (rows + 1, 1)))
        # the outputs of round 4 as they lie on the device are the inputs of round 5
        _lib.check(_open_call(key, [bufs[12].ptr, bufs[11].ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[8].ptr, kg.ptr, oq.ptr, ov.ptr], n + 3, rows, n + 2))
        gq, gv = oq.to_numpy(np.uint64, (rows * (n + 2) + 1, 4)), ov.to_numpy(np.uint64, (rows + 1, 4))
        assert (gq[:-1] == want("q", n + 2)).all() and (gq[-1] == SENTINEL).all()
        assert (gv[:-1] == want("value", 1)).all() and (gv[-1] == SENTINEL).all()


# ---------------------------------------------------------------------------------------------------- the Python doors
@pytest.mark.parametrize("log_n", (6, 10))
def test_host_form_equals_the_device_form(log_n):
    key = _key(log_n)
    pk, n, keep = key["pk"], key["n"], key["keep"]
    pool = [_row(log_n, j)[1] for j in range(po.POOL)]
    stack = lambda k: np.ascontiguousarray(np.stack([im[k] for im in pool]))
    cat = lambda k: np.ascontiguousarray(np.concatenate([im[k] for im in pool]))
    res = pk.linearize_batch(stack("bl"), stack("br"), stack("bo"), stack("bz"), stack("h"), cat("alpha"), cat("beta"), cat("gamma"), cat("zeta"))
    assert [a.shape for a in res] == [(po.POOL, 8, 4), (po.POOL, n + 2, 4), (po.POOL, n + 3, 4), (po.POOL, n + 2, 4)]
    for k, a in zip(OUT_KEYS, res):
        assert (a == stack(k)).all(), k
    q, value = zk.open_batch(pk, stack("fh"), stack("lin"), stack("bl"), stack("br"), stack("bo"), cat("zeta"), cat("kzg_gamma"), rows=po.POOL)
    assert (q == stack("q")).all() and (value == cat("value")).all()
    # the device doors of the same methods: buffers in, buffers out
    host = _lin_arrays(pool, n + 4, keep + 1, n + 5)
    with _Dev() as d:
        b = [d.up(a) for a in host]
        out = pk.linearize_batch(*b[:9], rows=po.POOL, in_stride=n + 4, h_stride=keep + 1, out_stride=n + 5, out=b[9:])
        assert out == tuple(b[9:])
        _lin_check([x.to_numpy(np.uint64, a.shape) for x, a in zip(out, host[9:])], pool, n + 5, (log_n, "door"))
        made = zk.linearize_batch(pk, *b[:9], rows=po.POOL, in_stride=n + 4, h_stride=keep + 1)
        try:
            assert (made[0].to_numpy(np.uint64, (po.POOL, 8, 4)) == res[0]).all() and (made[2].to_numpy(np.uint64, (po.POOL, n + 3, 4)) == res[2]).all()
        finally:
            for x in made:
                x.free()
        host5 = _open_arrays(pool, n + 4, n + 3)
        b5 = [d.up(a) for a in host5]
        out5 = pk.open_batch(*b5[:7], rows=po.POOL, in_stride=n + 4, out_stride=n + 3, out=b5[7:])
        assert out5 == tuple(b5[7:])
        _open_check([x.to_numpy(np.uint64, a.shape) for x, a in zip(out5, host5[7:])], pool, n + 3, (log_n, "door 5"))
        mq, mv = pk.open_batch(*b5[:7], rows=po.POOL, in_stride=n + 4)
        try:
            assert (mq.to_numpy(np.uint64, q.shape) == q).all() and (mv.to_numpy(np.uint64, value.shape) == value).all()
        finally:
            mq.free()
            mv.free()


def test_no_rows_and_argument_errors_that_need_the_keys_sizes():
    """rows = 0 returns at once; a stride below its minimum or an output over an input or another output is ZK_ERR_ARG, an unknown key ZK_ERR_HANDLE, with
    nothing written"""
    key = _key(3)
    n, keep = key["n"], key["keep"]
    imgs = [_row(3, j)[1] for j in (0, 1)]
    host, host5 = _lin_arrays(imgs, n + 3, keep, n + 3), _open_arrays(imgs, n + 3, n + 2)
    stranger = dict(key, pk=zp.ProvingKey(987654321, None, None, 0))
    with _Dev() as d:
        bufs, bufs5 = [d.up(a) for a in host], [d.up(a) for a in host5]
        p, p5 = [b.ptr for b in bufs], [b.ptr for b in bufs5]
        assert _lin_call(key, p, n + 3, keep, 0, n + 3) == _lib.ZK_OK and _lin_call(key, p, 0, 0, 0, 0) == _lib.ZK_OK
        assert _open_call(key, p5, n + 3, 0, n + 2) == _lib.ZK_OK and _open_call(key, p5, 0, 0, 0) == _lib.ZK_OK
        swap = lambda q, i, v: q[:i] + [v] + q[i + 1:]
        bad = {"in_stride": _lin_call(key, p, n + 2, keep, 2, n + 3), "h_stride": _lin_call(key, p, n + 3, keep - 1, 2, n + 3),
               "out_stride": _lin_call(key, p, n + 3, keep, 2, n + 2), "values = l": _lin_call(key, swap(p, 9, p[0]), n + 3, keep, 2, n + 3),
               "zquot inside z": _lin_call(key, swap(p, 10, p[3] + 32), n + 3, keep, 2, n + 3), "lin over h": _lin_call(key, swap(p, 11, p[4]), n + 3, keep, 2, n + 3),
               "fh over zeta": _lin_call(key, swap(p, 12, p[8]), n + 3, keep, 2, n + 3), "fh = lin": _lin_call(key, swap(p, 12, p[11]), n + 3, keep, 2, n + 3),
               "zquot inside values": _lin_call(key, swap(p, 10, p[9] + 64), n + 3, keep, 2, n + 3),
               "5 in_stride": _open_call(key, p5, n + 2, 2, n + 2), "5 out_stride": _open_call(key, p5, n + 3, 2, n + 1),
               "q = fh": _open_call(key, swap(p5, 7, p5[0]), n + 3, 2, n + 2), "q inside lin": _open_call(key, swap(p5, 7, p5[1] + 32), n + 3, 2, n + 2),
               "value = kzg gamma": _open_call(key, swap(p5, 8, p5[6]), n + 3, 2, n + 2), "value inside q": _open_call(key, swap(p5, 8, p5[7] + 64), n + 3, 2, n + 2)}
        assert {k: v for k, v in bad.items() if v != _lib.ZK_ERR_ARG} == {}
        assert _lin_call(stranger, p, n + 3, keep, 2, n + 3) == _lib.ZK_ERR_HANDLE and _open_call(stranger, p5, n + 3, 2, n + 2) == _lib.ZK_ERR_HANDLE
        for buf, a in zip(bufs + bufs5, host + host5):
            assert (buf.to_numpy(a.dtype, a.shape) == a).all(), "something was written"
    stranger["pk"].handle = C.c_uint64(0)


# --------------------------------------------------------------------------------------------------------------------- 2^16
def test_one_row_at_2p16_equals_the_restatement():
    key = _key(BIG)
    n = key["n"]
    row, im = _row(BIG, 4)
    _lin_check(_lin_dev(key, [im], n + 4, key["keep"] + 1, n + 4), [im], n + 4, (BIG, "round 4"))
    _open_check(_open_batch_dev(key, [im], n + 4, n + 3), [im], n + 3, (BIG, "round 5"))
