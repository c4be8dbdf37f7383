"""The row-batched quotient of PLONK's round 3 (csrc/plonk.hip quotient_rows_dev: spread, one transform over the 4 * rows polynomials, qk, k_quotient29_rows,
the inverse transform, the tail) through zk_bn254_plonk_quotient_batch_dev and ProvingKey.quotient_batch  (-m gpu).  Everything is bit-exact.

Sizes, one per shape a launch can take: 2^2 (N4 = 32, rho = 8: all eight 1 / (x^n - 1) in use), 2^3 (N4 = 32, rho = 4), 2^6 (N4 = 2^8: one workgroup of the
quotient kernel), 2^9 (N4 = 2^11: exactly one transform tile), 2^10 (N4 = 2^12: the first strided pass), 2^12, 2^16.  Row counts 1, 2, 3, 5 (2^16: 1 and 2).
Rows: all rows of a call are witnesses of ONE circuit (tests/plonk_quotient_ref.py forward_circuit), each with its own blinders, public inputs and challenges
(pool_row): one has alpha = 0, one beta = 0, one gamma = 0, one the `max` family's values, and one is VIOLATED, with alpha = beta = gamma = r - 1; from three
rows on it sits between satisfied ones.  Strides at their minimum and minimum + 1 for inputs, public inputs and output independently; the gaps and one
element behind the last row hold a sentinel that must survive; the inputs must be unchanged.
Expectation up to 2^12: tests/plonk_quotient_ref.quotient (Python integers; tests/test_plonk_quotient_cpu.py holds it against the oracle prover's h).  At 2^16:
two rows, the reference for one of them, each row equal to its one-row call."""
import ctypes as C

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
from tests import plonk_quotient_ref as qr

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
SENTINEL = qr.SENTINEL
STATUS_SENTINEL = 0x5A5A5A5A
LOG_N = (2, 3, 6, 9, 10, 12)
ROW_COUNTS = (1, 2, 3, 5)
BIG = 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback
    yield
    for k in list(_keys):
        key = _keys.pop(k)
        key["pk"].free()
        key["rb"].free()


# ---------------------------------------------------------------------------------------------------- keys, rows and expectations, computed once
_keys, _rows = {}, {}


def _circuit(spr) -> zp.Circuit:
    g = spr.constraints
    col = lambda k: M([c[k] for c in g])
    return zp.Circuit(spr.n_public, spr.n_vars, col(0), col(1), col(2), col(3), col(4), [c[5] for c in g], [c[6] for c in g], [c[7] for c in g])


def _device_key(spr, n):
    rb = zb.ResidentBases(orc.g1_gen_points(0x9F0 + n, n + 3))
    return zp.setup(_circuit(spr), rb), rb


def _key(log_n, npub=1):
    """one circuit per (size, number of public inputs): its device key and the oracle's polynomials of the same key"""
    if (log_n, npub) not in _keys:
        n = 1 << log_n
        spr, n_in = qr.forward_circuit(n, npub, 0x7C0 + 64 * npub + log_n)
        pk, rb = _device_key(spr, n)
        assert pk.domain_size == n and pk.n_public == npub
        _keys[(log_n, npub)] = dict(spr=spr, n_in=n_in, n=n, npub=npub, keep=3 * (n + 2), opk=qr.setup_polys(spr, fast=True), pk=pk, rb=rb)
    return _keys[(log_n, npub)]


def _image(row):
    img = {k: M(row[k]) for k in ("bl", "br", "bo", "bz")}
    img["public"] = M(row["public"]) if row["public"] else np.zeros((0, 4), np.uint64)
    img.update({k: M([row[k]]) for k in ("alpha", "beta", "gamma")})
    for v in img.values():
        v.setflags(write=False)
    return img


def _row(log_n, j, npub=1, want=True):
    """pool row j of the key: (integers, Montgomery images, expected 3 (n + 2) coefficients or None, expected status)"""
    key = _key(log_n, npub)
    k = (log_n, npub, j)
    if k not in _rows:
        row = qr.pool_row(key["opk"], key["n_in"], j, 0xD00 + 16 * npub + log_n, fast=True)
        _rows[k] = [row, _image(row), None, row["violated"]]
    e = _rows[k]
    if want and e[2] is None:
        row = e[0]
        h, status = qr.quotient(key["opk"], row["bl"], row["br"], row["bo"], row["bz"], row["public"], row["alpha"], row["beta"], row["gamma"], fast=True)
        assert status == row["violated"]
        e[2] = M(h[:key["keep"]])
        e[2].setflags(write=False)
    return e


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


def _arrays(key, imgs, in_stride, pub_stride, out_stride):
    """the ten host arrays of a call: l, r, o, z, public (None without public inputs), alpha, beta, gamma, out, status -- gaps and ends hold sentinels"""
    rows, npub = len(imgs), key["npub"]
    ins = [qr.strided([im[k] for im in imgs], in_stride) for k in ("bl", "br", "bo", "bz")]
    pub = qr.strided([im["public"] for im in imgs], pub_stride) if npub else None
    ch = [np.concatenate([im[k] for im in imgs] + [SENTINEL[None]]) for k in ("alpha", "beta", "gamma")]
    out = np.tile(SENTINEL, (rows * out_stride + 1, 1))
    status = np.full(rows + 1, STATUS_SENTINEL, dtype=np.int32)
    return ins + [pub] + ch + [out, status]


def _call(key, ptrs, in_stride, pub_stride, rows, out_stride):
    p = [C.c_void_p(v) for v in ptrs]
    return _lib.lib().zk_bn254_plonk_quotient_batch_dev(key["pk"].handle, p[0], p[1], p[2], p[3], C.c_size_t(in_stride), p[4], C.c_size_t(pub_stride), C.c_size_t(rows),
                                                        p[5], p[6], p[7], p[8], C.c_size_t(out_stride), p[9], None)


def _quot_dev(key, imgs, in_stride=None, pub_stride=None, out_stride=None):
    """rows = len(imgs) through zk_bn254_plonk_quotient_batch_dev -> (the output buffer as it is afterwards, (rows * out_stride + 1, 4); the status buffer,
    (rows + 1,)); asserts that the inputs, gaps included, are unchanged"""
    n, npub, keep = key["n"], key["npub"], key["keep"]
    in_stride, pub_stride, out_stride = in_stride or n + 3, npub if pub_stride is None else pub_stride, out_stride or keep
    host = _arrays(key, imgs, in_stride, pub_stride, out_stride)
    with _Dev() as d:
        bufs = [d.up(a) if a is not None else None for a in host]
        _lib.check(_call(key, [b.ptr if b is not None else 0 for b in bufs], in_stride, pub_stride, len(imgs), out_stride))
        for buf, a in zip(bufs[:8], host[:8]):
            if a is not None:
                assert (buf.to_numpy(np.uint64, a.shape) == a).all(), "an input changed"
        return bufs[8].to_numpy(np.uint64, host[8].shape), bufs[9].to_numpy(np.int32, host[9].shape)


def _check(got, want_rows, want_status, out_stride, keep, what):
    out, status = got
    free = np.ones(out.shape[0], dtype=bool)
    for i, w in enumerate(want_rows):
        assert (out[i * out_stride:i * out_stride + keep] == w).all(), what + ("row", i)
        free[i * out_stride:i * out_stride + keep] = False
    assert (out[free] == SENTINEL).all(), what + ("sentinel",)
    assert status.tolist() == list(want_status) + [STATUS_SENTINEL], what + ("status",)


# ------------------------------------------------------------------------------------------------------------ 2^2 .. 2^12
@pytest.mark.parametrize("log_n", LOG_N)
def test_every_row_count_and_stride(log_n):
    """1, 2, 3 and 5 rows at input, public-input and output strides at their minimum and one above, independently: every row equals the Python expectation
    (the violated one included, with status 1 and its neighbours 0) and hence its one-row call; sentinels and inputs untouched"""
    key = _key(log_n)
    n, keep = key["n"], key["keep"]
    pool = [_row(log_n, j) for j in range(qr.POOL)]
    assert [e[3] for e in pool] == [0, 0, 1, 0, 0]
    for j, e in enumerate(pool):
        _check(_quot_dev(key, [e[1]]), [e[2]], [e[3]], keep, keep, (log_n, "one row", j))
    for rows in ROW_COUNTS:
        idx = qr.rows_of(rows)
        imgs, want, status = [pool[j][1] for j in idx], [pool[j][2] for j in idx], [pool[j][3] for j in idx]
        for in_stride in (n + 3, n + 4):
            for pub_stride in (1, 2):
                for out_stride in (keep, keep + 1):
                    got = _quot_dev(key, imgs, in_stride, pub_stride, out_stride)
                    _check(got, want, status, out_stride, keep, (log_n, rows, in_stride, pub_stride, out_stride))


@pytest.mark.parametrize("npub", (0, 1, 32, 33))
@pytest.mark.parametrize("log_n", (6, 10))
def test_public_inputs_on_both_qk_paths(log_n, npub):
    """no public input, one, 32 (the last count k_qk_coset_rows takes) and 33 (the literal sequence in row form): three rows with different public inputs, the
    middle one violated, against the Python expectation; one row alone; public inputs read from a wider array"""
    key = _key(log_n, npub)
    keep = key["keep"]
    pool = [_row(log_n, j, npub) for j in (1, 2, 3)]
    if npub:
        assert len({e[1]["public"].tobytes() for e in pool}) == 3
    for pub_stride in ((0,) if npub == 0 else (npub, npub + 3)):
        got = _quot_dev(key, [e[1] for e in pool], None, pub_stride, None)
        _check(got, [e[2] for e in pool], [0, 1, 0], keep, keep, (log_n, npub, pub_stride))
    _check(_quot_dev(key, [pool[2][1]]), [pool[2][2]], [0], keep, keep, (log_n, npub, "one row"))


# ------------------------------------------------------------------------------------------------------------ against the device prover
@pytest.mark.parametrize("lagrange", (False, True))
@pytest.mark.parametrize("log_n", (6, 10, 12))
def test_thirds_of_h_commit_to_the_device_provers_digests(log_n, lagrange):
    """zp.prove with pinned challenges on a satisfied witness; the oracle's bl, br, bo, bz for the same blinders through quotient_batch; the three thirds of h,
    committed against the key's SRS, compress to H[0..2] of Proof.WriteTo (bytes 128 .. 224) -- with the key's Lagrange-form SRS absent and present"""
    key = _key(log_n)
    n, spr, opk = key["n"], key["spr"], key["opk"]
    g = ref.SplitMix64(0xFACE + log_n)
    sol = qr.solve(spr, [g.felt() for _ in range(key["n_in"])])
    blinders, pin = [g.felt() for _ in range(9)], [g.felt() for _ in range(5)]     # gamma, beta, alpha, zeta, kzg gamma
    pk, rb = _device_key(spr, n) if lagrange else (key["pk"], key["rb"])
    try:
        if lagrange:
            pk.lagrange_srs()
        proof = zp.prove(pk, M(sol), M(blinders), challenges=M(pin))
        bl, br, bo, bz = qr.rounds_1_2(opk, sol, blinders, pin[1], pin[0], fast=True)
        one = lambda v: np.ascontiguousarray(M(v)[None])
        h, status = pk.quotient_batch(one(bl), one(br), one(bo), one(bz), one(sol[:1]), M([pin[2]]), M([pin[1]]), M([pin[0]]))
        assert status.tolist() == [0] and h.shape == (1, 3 * (n + 2), 4)
        srs = zkzg.SRS(rb, None)
        got = b"".join(ref.g1_compress(pl.g1_from_np(srs.commit(np.ascontiguousarray(h[0, k * (n + 2):(k + 1) * (n + 2)])))) for k in range(3))
        assert got == proof[128:224]
    finally:
        if lagrange:
            pk.free()
            rb.free()


# ------------------------------------------------------------------------------------------------------------ chunks
def test_more_rows_than_one_chunk_of_workspace():
    """2^12: 5 * 2^14 * 32 B = 2.5 MiB of workspace per row against 1 GiB at a time is 409 rows per chunk, so 412 rows run as 409 + 3.  The rows cycle through
    the pool's five witnesses; rows 0 .. 4 have the pool's challenges (held against the Python expectation), every later row has its own alpha, and every seventh
    its own beta and gamma as well (Z no longer fits them: status 1).  Every row equals its one-row call."""
    log_n, rows = 12, 412
    key = _key(log_n)
    n, keep = key["n"], key["keep"]
    per_chunk = (1 << 30) // (5 * (4 * n) * 32)
    assert per_chunk == 409 and per_chunk < rows < 2 * per_chunk
    pool = [_row(log_n, j) for j in range(qr.POOL)]
    g = ref.SplitMix64(0xC4C4)
    imgs = []
    for v in range(rows):
        im = dict(pool[v % qr.POOL][1])
        if v >= qr.POOL:
            im["alpha"] = M([g.felt()])
            if v % 7 == 0:
                im["beta"], im["gamma"] = M([g.felt()]), M([g.felt()])
        imgs.append(im)
    in_stride, out_stride = n + 3, keep
    host = _arrays(key, imgs, in_stride, 1, out_stride)
    single = np.tile(SENTINEL, (host[8].shape[0], 1))
    single_status = np.full(rows + 1, STATUS_SENTINEL, dtype=np.int32)
    with _Dev() as d:
        bufs = [d.up(a) for a in host]
        ptrs = [b.ptr for b in bufs]
        _lib.check(_call(key, ptrs, in_stride, 1, rows, out_stride))
        out, status = bufs[8].to_numpy(np.uint64, host[8].shape), bufs[9].to_numpy(np.int32, host[9].shape)
        one_out, one_status = d.up(single), d.up(single_status)
        step = [in_stride * 32] * 4 + [32] * 4 + [out_stride * 32, 4]
        for v in range(rows):
            at = [p + v * s for p, s in zip(ptrs[:8] + [one_out.ptr, one_status.ptr], step)]
            _lib.check(_call(key, at, in_stride, 1, 1, out_stride))
        single, single_status = one_out.to_numpy(np.uint64, single.shape), one_status.to_numpy(np.int32, single_status.shape)
    assert (out == single).all() and (status == single_status).all()
    assert (out[-1] == SENTINEL).all() and status[-1] == STATUS_SENTINEL
    for j, e in enumerate(pool):
        assert (out[j * out_stride:(j + 1) * out_stride] == e[2]).all() and status[j] == e[3], j
    want_status = [1 if (v % qr.POOL == 2 or (v >= qr.POOL and v % 7 == 0)) else 0 for v in range(rows)]
    assert status[:rows].tolist() == want_status


# ------------------------------------------------------------------------------------------------------------ the Python doors
@pytest.mark.parametrize("log_n", (6, 10))
def test_host_form_equals_the_device_form(log_n):
    key = _key(log_n)
    pk, n, keep = key["pk"], key["n"], key["keep"]
    pool = [_row(log_n, j) for j in range(qr.POOL)]
    stack = lambda k: np.ascontiguousarray(np.stack([e[1][k] for e in pool]))
    cat = lambda k: np.ascontiguousarray(np.concatenate([e[1][k] for e in pool]))
    h, status = pk.quotient_batch(stack("bl"), stack("br"), stack("bo"), stack("bz"), stack("public"), cat("alpha"), cat("beta"), cat("gamma"))
    assert h.shape == (qr.POOL, keep, 4) and status.dtype == np.int32 and status.tolist() == [0, 0, 1, 0, 0]
    for j, e in enumerate(pool):
        assert (h[j] == e[2]).all(), j
    # l, r, o may come with n + 3 coefficients a row, the last one unread
    wide = lambda k: np.ascontiguousarray(np.concatenate([stack(k), np.tile(SENTINEL, (qr.POOL, 1, 1))], axis=1))
    h2, status2 = pk.quotient_batch(wide("bl"), wide("br"), wide("bo"), stack("bz"), stack("public"), cat("alpha"), cat("beta"), cat("gamma"), rows=qr.POOL)
    assert (h2 == h).all() and (status2 == status).all()
    # the device door of the same method: buffers in, buffers out
    host = _arrays(key, [e[1] for e in pool], n + 4, 2, keep + 1)
    with _Dev() as d:
        b = [d.up(a) for a in host]
        out, st = pk.quotient_batch(*b[:8], rows=qr.POOL, in_stride=n + 4, pub_stride=2, out_stride=keep + 1, out=b[8], status=b[9])
        assert out is b[8] and st is b[9]
        _check((out.to_numpy(np.uint64, host[8].shape), st.to_numpy(np.int32, host[9].shape)), [e[2] for e in pool], [0, 0, 1, 0, 0], keep + 1, keep, (log_n, "door"))
        made, made_st = pk.quotient_batch(*b[:8], rows=qr.POOL, in_stride=n + 4, pub_stride=2)
        try:
            assert (made.to_numpy(np.uint64, h.shape) == h).all() and (made_st.to_numpy(np.int32, (qr.POOL,)) == status).all()
        finally:
            made.free()
            made_st.free()


def test_no_rows_and_argument_errors_that_need_the_keys_sizes():
    """rows = 0 returns at once and touches nothing; a stride below its minimum or an output over an input is ZK_ERR_ARG, with nothing written"""
    key = _key(3)
    n, keep = key["n"], key["keep"]
    imgs = [_row(3, j)[1] for j in (0, 1)]
    host = _arrays(key, imgs, n + 3, 1, keep)
    with _Dev() as d:
        bufs = [d.up(a) for a in host]
        ptrs = [b.ptr for b in bufs]
        assert _call(key, ptrs, n + 3, 1, 0, keep) == _lib.ZK_OK
        assert _call(key, ptrs, 0, 0, 0, 0) == _lib.ZK_OK
        swap = lambda i, v: ptrs[:i] + [v] + ptrs[i + 1:]
        bad = {"in_stride": _call(key, ptrs, n + 2, 1, 2, keep), "pub_stride": _call(key, ptrs, n + 3, 0, 2, keep), "out_stride": _call(key, ptrs, n + 3, 1, 2, keep - 1),
               "h = l": _call(key, swap(8, ptrs[0]), n + 3, 1, 2, keep), "h inside z": _call(key, swap(8, ptrs[3] + 32), n + 3, 1, 2, keep),
               "h over gamma": _call(key, swap(8, ptrs[7]), n + 3, 1, 2, keep), "status = alpha": _call(key, swap(9, ptrs[5]), n + 3, 1, 2, keep),
               "status inside h": _call(key, swap(9, ptrs[8] + 64), n + 3, 1, 2, keep), "no public inputs": _call(key, swap(4, 0), n + 3, 1, 2, keep)}
        assert {k: v for k, v in bad.items() if v != _lib.ZK_ERR_ARG} == {}
        for buf, a in zip(bufs, host):
            assert (buf.to_numpy(a.dtype, a.shape) == a).all(), "something was written"
    z = lambda *shape: np.zeros(shape, np.uint64)
    h, status = key["pk"].quotient_batch(z(0, n + 2, 4), z(0, n + 2, 4), z(0, n + 2, 4), z(0, n + 3, 4), z(0, 1, 4), z(0, 4), z(0, 4), z(0, 4))
    assert h.shape == (0, keep, 4) and status.shape == (0,)


# --------------------------------------------------------------------------------------------------------------------- 2^16
@pytest.fixture(scope="module")
def big():
    """two rows at 2^16 (N4 = 2^18): the `max` row and the alpha = 0 row, each alone and both in one call at strides one above the minimum; the Python
    expectation for the second (some 20 s, the slow part of this module: computed once)"""
    key = _key(BIG)
    rows = [_row(BIG, 3, want=False), _row(BIG, 0, want=True)]
    single = [_quot_dev(key, [e[1]]) for e in rows]
    both = _quot_dev(key, [e[1] for e in rows], key["n"] + 4, 2, key["keep"] + 1)
    return dict(key=key, rows=rows, single=single, both=both)


def test_2p16_rows_equal_their_one_row_calls(big):
    keep = big["key"]["keep"]
    for out, status in big["single"]:
        assert status.tolist() == [0, STATUS_SENTINEL] and (out[keep] == SENTINEL).all() and out[:keep].any()
    _check(big["both"], [s[0][:keep] for s in big["single"]], [0, 0], keep + 1, keep, (BIG, "two rows"))


def test_2p16_row_equals_the_python_expectation(big):
    keep = big["key"]["keep"]
    assert (big["single"][1][0][:keep] == big["rows"][1][2]).all()
