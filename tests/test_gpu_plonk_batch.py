"""The batch PLONK prover (csrc/plonk_batch.hip; zk_bn254_plonk_prove_batch, zk_bn254_plonk_challenges_batch_dev) on the device (-m gpu).  Everything is
bit-exact: row v's 548 bytes are zp.prove's for the same solution, blinders and challenges (and the C oracle's up to 2^6), and every transcript stage gives the
challenge and the raw digest of tests/plonk_batch_ref.py, which tests/test_plonk_batch_cpu.py holds against oracle/plonk_ref.py.

The rows of one call must satisfy ONE circuit with different values: _free_rows() appends a gate without selectors over three fresh variables and takes the
last public variable out of every gate, so those four values are free in every row (they enter l, r, o, the public inputs' share of qk and the transcript)."""
import ctypes as C
import threading

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import plonk as zp
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_batch_ref as br
from tests import plonk_shapes as ps
from tests.test_gpu_plonk import _circuit, _device_srs

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
INF = bytes([0x40]) + bytes(31)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def bases():
    return orc.g1_gen_points(0x9E0, (1 << 12) + 3)


def _free_rows(log_n, npub, rows, seed, family="random"):
    """-> (spr, [solution per row]): a circuit that fills its domain of 2^log_n rows and `rows` solutions of it that differ in three secret values and in the last
    public input"""
    n = 1 << log_n
    spr, sol = ps.circuit(family, n, npub, n - 1, seed)
    nv = len(sol)
    gates = [list(c) for c in spr.constraints]
    if npub:
        for c in gates:
            for k in (5, 6, 7):
                if c[k] == npub - 1: c[k] = npub     # the first secret variable instead
    gates.append([0, 0, 0, 0, 0, nv, nv + 1, nv + 2])
    spr = ps.with_solution(pl.SparseR1CS(npub, nv + 3 - npub, [tuple(c) for c in gates]), list(sol) + [0, 0, 0])
    assert ps.domain_size(spr) == n
    g = ref.SplitMix64(seed ^ 0xF4EE)
    sols = []
    for v in range(rows):
        s = list(sol) + [g.felt(), (0, R - 1)[v & 1] if v < 2 else g.felt(), g.felt()]
        if npub and v:
            s[npub - 1] = g.felt()
        assert spr.is_satisfied(s)
        sols.append(s)
    return spr, sols


def _inputs(sols, seed):
    """Montgomery rows: solutions (rows, n_vars, 4), blinders (rows, 9, 4), pinned challenges (rows, 5, 4)"""
    rows = len(sols)
    return (np.stack([M(s) for s in sols]), np.stack([M(ps.blinders("random", seed + v)) for v in range(rows)]),
            np.stack([M(ref.rand_felts(0xC4A + seed + v, 5)) for v in range(rows)]))


def _prove_c(pk, sol, bl, ch, *, stride=None, on_device=False, chunk_rows=0):
    """zk_bn254_plonk_prove_batch itself: rows sol_stride apart (the gaps hold r - 1 patterns the prover must not read as values)"""
    rows, nv = sol.shape[0], sol.shape[1]
    stride = nv if stride is None else stride
    wide = np.full((rows, stride, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
    wide[:, :nv] = sol
    dev = _lib.DeviceBuffer.from_numpy(wide) if on_device else None
    out, st = np.full((rows, 548), 0xA5, np.uint8), np.full(rows, -1, np.int32)
    try:
        _lib.check(_lib.lib().zk_bn254_plonk_prove_batch(pk.handle, C.c_void_p(dev.ptr) if on_device else _lib.vp(wide), C.c_size_t(nv), C.c_size_t(stride),
                                                         C.c_size_t(rows), C.c_int(int(on_device)), _lib.vp(bl), _lib.vp(ch) if ch is not None else None,
                                                         C.c_size_t(chunk_rows), _lib.vp(out), _lib.vp(st)))
    finally:
        if dev is not None:
            dev.free()
    return [out[v].tobytes() for v in range(rows)], list(st)


def _single(pk, sol, bl, ch=None):
    return [zp.prove(pk, sol[v], bl[v], None if ch is None else ch[v]) for v in range(sol.shape[0])]


# ------------------------------------------------------------------------------------------------ the transcript alone
def _point_rows(bases, rows, k, seed):
    """(rows, k, 8) affine Montgomery images and the same as integer pairs; row 1 (where there is one) is all infinity, as is the last point of the last row"""
    g = ref.SplitMix64(seed)
    a = np.stack([np.stack([bases[int(g.next() % len(bases))] for _ in range(k)]) for _ in range(rows)])
    if rows > 1:
        a[1] = 0
    a[rows - 1, k - 1] = 0
    return a, [[pl.g1_from_np(a[v, j]) for j in range(k)] for v in range(rows)]


@pytest.mark.parametrize("npub,log_n", [(0, 3), (1, 3), (2, 3), (33, 6)])
def test_every_transcript_stage_is_the_reference_transcript(npub, log_n, bases):
    """gamma's message is 517 + 32 npub + 192 bytes: its length modulo 64 takes the two values npub = 0 and 1 give, and npub = 2 and 33 repeat them with more
    blocks; 65 rows are a second workgroup of 64 lanes; a row binds the point at infinity for [L], [R], [O] (and [Z], the quotient's and kzg's digests); the
    claimed values include 0 and r - 1"""
    n = 1 << log_n
    spr, sol = ps.circuit("random", n, npub, "full", 0x7A + npub)
    rb = zb.ResidentBases(bases[:n + 3])
    pk = zp.setup(_circuit(spr), rb)
    vk = pk.vk
    key = [pl.g1_from_np(p) for p in vk["s"]] + [pl.g1_from_np(vk[k]) for k in ("ql", "qr", "qm", "qo", "qk")]
    g = ref.SplitMix64(0x5EED + npub)
    for rows in (1, 2, 3, 65):
        pub = [[(0, R - 1, g.felt())[(v + j) % 3] for j in range(npub)] for v in range(rows)]
        vals = [[(0, R - 1)[(v + j) & 1] if j < 2 else g.felt() for j in range(8)] for v in range(rows)]
        zeta = [R - 1 if v == 0 else g.felt() for v in range(rows)]
        prev = np.frombuffer(bytes(int(g.next() & 0xFF) for _ in range(32 * rows)), np.uint8).reshape(rows, 32).copy()
        prev[0] = 0xFF                                        # a digest above r: bound as it is, never reduced
        for stage, k in enumerate((3, 0, 1, 3, 5)):
            pts, ipts = _point_rows(bases, rows, k, 0x90 + stage + rows) if k else (None, [[]] * rows)
            kw = dict(points=pts)
            if stage == 0:
                kw["public"] = np.stack([M(p) for p in pub]) if npub else None
            elif stage == 4:
                kw.update(prev=M(zeta), values=np.stack([M(v) for v in vals]))
            else:
                kw["prev"] = prev
            got, raw = zp.challenges_rows(pk, stage, **kw)
            for v in range(rows):
                want, digest = br.stage(stage, key, public=pub[v], points=ipts[v], prev=zeta[v] if stage == 4 else prev[v].tobytes(), values=vals[v])
                assert raw[v].tobytes() == digest, (rows, stage, v)
                assert pl.mont_np_to_ints(got[v:v + 1]) == [want], (rows, stage, v)
    pk.free()
    rb.free()


# ------------------------------------------------------------------------------------------------ proofs
@pytest.mark.parametrize("log_n,npub", [(2, 1), (3, 0), (6, 33), (10, 1), (11, 0), (12, 33)])
def test_rows_are_the_single_provers_bytes(log_n, npub, bases):
    """1, 2, 3 and 5 rows, from host rows, from rows with gaps between them, from device rows, with the transcript and with pinned challenges; two identical rows;
    at 2^11 s1 and s2 fill a scan workgroup exactly; at 2^12 again with the Lagrange form of the bases (l, r, o committed from the values) -- and up to 2^6 the
    single prover's bytes are the C oracle's"""
    n = 1 << log_n
    spr, sols = _free_rows(log_n, npub, 5, 0xB0 + log_n)
    pts = bases[:n + 3]
    rb = zb.ResidentBases(pts)
    pk = zp.setup(_circuit(spr), rb)
    sol, bl, ch = _inputs(sols, log_n)
    want, want_pinned = _single(pk, sol, bl), _single(pk, sol, bl, ch)
    assert len(set(want)) == 5 and all(len(p) == 548 for p in want)
    if log_n <= 6:
        ck = ps.c_key(orc, spr, pts)
        assert [ck.prove(sol[v], bl[v]) for v in range(5)] == want
        ck.free()
    info = zp.prove_batch_info(pk)
    assert info["lin_by_linearity"] == 1 and info["chunk_rows"] >= 5 and info["commits_batched"] == zb.msm_rows_info(rb, n + 3)["batched"]
    for rows in (1, 2, 3, 5):
        assert zp.prove_batch(pk, sol[:rows], bl[:rows]) == want[:rows], rows
        assert zp.prove_batch(pk, sol[:rows], bl[:rows], ch[:rows]) == want_pinned[:rows], rows
        assert _prove_c(pk, sol[:rows], bl[:rows], None, stride=sol.shape[1] + 5) == (want[:rows], [0] * rows), rows
        assert _prove_c(pk, sol[:rows], bl[:rows], ch[:rows], stride=sol.shape[1] + 1, on_device=True) == (want_pinned[:rows], [0] * rows), rows
    dev = _lib.DeviceBuffer.from_numpy(sol)
    assert zp.prove_batch(pk, dev, bl, on_device=True) == want
    assert zp.prove_batch(pk, dev.ptr, bl[:3], ch[:3], on_device=True) == want_pinned[:3]
    dev.free()
    twice = zp.prove_batch(pk, sol[[1, 3, 1]], bl[[1, 3, 1]])
    assert twice == [want[1], want[3], want[1]]
    if n + 2 >= ps.WINDOW_TABLE_MIN:
        pk.lagrange_srs()
        assert _single(pk, sol[:3], bl[:3]) == want[:3]
        assert zp.prove_batch(pk, sol, bl) == want
        assert zp.prove_batch(pk, sol[:1], bl[:1], ch[:1]) == want_pinned[:1]
    pk.free()
    rb.free()


def test_commitments_at_infinity(bases):
    """all-zero values, the identity permutation and zero blinders at 2^3: l = r = o = 0 and a zero quotient, so [L], [R], [O], [H0..2] and the opening of z are
    the point at infinity -- in the transcript, in the digests taken by linearity and in the proof"""
    n = 8
    spr, sol = ps.circuit("zeros+identity_perm", n, 0, "full", 0x57 + 3)
    rb = zb.ResidentBases(bases[:n + 3])
    pk = zp.setup(_circuit(spr), rb)
    msol, bl = M(sol), M(ps.blinders("zeros"))
    want = zp.prove(pk, msol, bl)
    assert [want[32 * k:32 * k + 32] == INF for k in range(7)] == [True, True, True, False, True, True, True] and want[484:516] == INF
    other = M(ps.blinders("random", 3))
    got = zp.prove_batch(pk, np.stack([msol, msol, msol]), np.stack([bl, other, bl]))
    assert got == [want, zp.prove(pk, msol, other), want]
    pk.free()
    rb.free()


@pytest.mark.parametrize("where", ps.VIOLATIONS)
def test_violated_row_between_two_good_ones(where, bases):
    """the middle row's solution violates one gate: its verdict is 1 and its bytes are zero; its neighbours are the single prover's proofs"""
    n = 64
    spr, sol, var = ps.violation_circuit(n, 3, 0xBAD0 + 6)
    rb = zb.ResidentBases(bases[:n + 3])
    pk = zp.setup(_circuit(spr), rb)
    bad = list(sol)
    bad[var[where]] = (bad[var[where]] + 1) % R
    assert not spr.is_satisfied(bad)
    rows, bl, ch = _inputs([sol, bad, sol], 6)
    want = [zp.prove(pk, rows[0], bl[0]), zp.prove(pk, rows[2], bl[2])]
    with pytest.raises(_lib.ZkmiError, match="does not satisfy"):
        zp.prove(pk, rows[1], bl[1])
    assert zp.prove_batch(pk, rows, bl) == [want[0], None, want[1]]
    assert _prove_c(pk, rows, bl, None) == ([want[0], bytes(548), want[1]], [0, 1, 0])
    pinned = zp.prove_batch(pk, rows, bl, ch)
    assert pinned == [zp.prove(pk, rows[0], bl[0], ch[0]), None, zp.prove(pk, rows[2], bl[2], ch[2])]
    pk.free()
    rb.free()


def test_chunks_change_no_byte(bases):
    """five rows at 2^4 in chunks of two: three chunks, the last of one row"""
    spr, sols = _free_rows(4, 2, 5, 0xC4)
    rb = zb.ResidentBases(bases[:16 + 3])
    pk = zp.setup(_circuit(spr), rb)
    sol, bl, ch = _inputs(sols, 4)
    want = _single(pk, sol, bl)
    assert zp.prove_batch(pk, sol, bl, chunk_rows=2) == want
    assert zp.prove_batch(pk, sol, bl, chunk_rows=1) == want
    assert _prove_c(pk, sol, bl, ch, stride=sol.shape[1] + 3, on_device=True, chunk_rows=2) == (_single(pk, sol, bl, ch), [0] * 5)
    pk.free()
    rb.free()


def test_key_from_its_wire_image_commits_the_linearised_polynomial(bases):
    """a key that no single proof has checked: the batch commits the linearised polynomial through the row MSM and never marks the key; after a single proof has,
    the digest is taken by linearity -- the same bytes"""
    log_n, n = 5, 32
    spr, sols = _free_rows(log_n, 1, 3, 0xD1)
    rb = zb.ResidentBases(bases[:n + 3])
    pk = zp.setup(_circuit(spr), rb)
    sol, bl, _ = _inputs(sols, 5)
    want = _single(pk, sol, bl)
    g = spr.constraints
    pk2 = zp.read_proving_key(pk.write(), spr.n_vars, [c[5] for c in g], [c[6] for c in g], [c[7] for c in g], rb)
    assert zp.prove_batch_info(pk2)["lin_by_linearity"] == 0
    assert zp.prove_batch(pk2, sol, bl) == want
    assert zp.prove_batch_info(pk2)["lin_by_linearity"] == 0
    assert zp.prove(pk2, sol[0], bl[0]) == want[0]
    assert zp.prove_batch_info(pk2)["lin_by_linearity"] == 1
    assert zp.prove_batch(pk2, sol, bl) == want
    pk2.free()
    pk.free()
    rb.free()


def test_batch_proofs_are_accepted_by_the_batch_verifier():
    log_n, n, rows = 6, 64, 8
    spr, sols = _free_rows(log_n, 2, rows, 0xE6)
    rb, _, g2 = _device_srs(n + 3, 0xA1FA0123456789)
    pk = zp.setup(_circuit(spr), rb)
    sol, bl, _ = _inputs(sols, 6)
    proofs = zp.prove_batch(pk, sol, bl)
    assert proofs == _single(pk, sol, bl)
    pub = np.ascontiguousarray(sol[:, :2])
    assert list(zv.plonk_verify_batch(proofs, pk.write()[:368], g2, pub)) == [True] * rows
    assert list(zv.plonk_verify_batch(proofs, pk.write()[:368], g2, np.ascontiguousarray(pub[::-1]))) != [True] * rows
    pk.free()
    rb.free()


def test_batches_overlap_each_other_and_a_single_proof(bases):
    """two threads each run prove_batch on one key while a third runs the single prover: the bytes are those of the serial runs"""
    log_n, n = 8, 256
    spr, sols = _free_rows(log_n, 1, 4, 0xF8)
    rb = zb.ResidentBases(bases[:n + 3])
    pk = zp.setup(_circuit(spr), rb)
    sol, bl, _ = _inputs(sols, 8)
    want = _single(pk, sol, bl)
    got, errs = {}, []

    def run(name, fn):
        try:
            got[name] = [fn() for _ in range(3)]
        except Exception as e:  # noqa: BLE001
            errs.append((name, e))

    threads = [threading.Thread(target=run, args=("a", lambda: zp.prove_batch(pk, sol, bl))),
               threading.Thread(target=run, args=("b", lambda: zp.prove_batch(pk, sol[::-1].copy(), bl[::-1].copy()))),
               threading.Thread(target=run, args=("single", lambda: zp.prove(pk, sol[2], bl[2])))]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not errs, errs
    assert got["a"] == [want] * 3 and got["b"] == [want[::-1]] * 3 and got["single"] == [want[2]] * 3
    pk.free()
    rb.free()
