"""Batch PLONK verification against many keys in one device call (zk_bn254_plonk_verify_batch_keys and its _dev form; -m gpu).  Every expected verdict comes
from tests/plonk_forge.py and tests/plonk_keys_cases.py -- a case's own verdict under its own key, 0 under another -- which tests/test_plonk_forge_cpu.py and
tests/test_plonk_verify_keys_cpu.py hold against the host verifier; never from the device.  The launch name pvk_single means "the per-lane fallback ran":
an all-accept batch must be decided WITHOUT it, because a wrong S1, S2, omega or n_public per lane still gives right verdicts through the fallback."""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from tests import plonk_forge as pf
from tests import plonk_keys_cases as kc

pytestmark = pytest.mark.gpu
CHUNK = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _profiled(fn):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        out = fn()
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    return out, prof


def _combined_only(prof):
    return "pvk_kzg" in prof and "pvk_single" not in prof and "pv_kzg" not in prof and "pv_single" not in prof


def _fell_back(prof):
    return "pvk_single" in prof


def _run(rows, stride=None, extra=(), again=True, wide=False, fill=0xBADC0FFEE0DDF00D):
    """one batch through the host form: every lane's verdict is the expected one, *n_accepted their count, a second call gives the same bytes"""
    b = rows if isinstance(rows, kc.Batch) else kc.Batch(rows, stride, extra)
    (rc, acc, n_acc), prof = _profiled(lambda: kc.call_host_form(b, b.pubs(fill, wide)))
    assert rc == _lib.ZK_OK, (_lib.lib().zk_last_error() or b"").decode()
    wrong = ["lane %d of %d: %s under %s: got %d, expected %d" % (i, b.n, c.label, k.name, acc[i], b.expect[i]) for i, (c, k) in enumerate(b.rows)
             if acc[i] != b.expect[i]]
    assert not wrong, wrong[:12]
    assert n_acc == int(acc.sum()) == int(b.expect.sum())
    if again:
        rc2, acc2, n_acc2 = kc.call_host_form(b, b.pubs(fill, wide))
        assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc
    return prof


def _rows_on_device(rows, stride, lead, poison):
    buf = np.full(lead + max(len(rows), 1) * stride + 64, poison, np.uint8)
    for v, r in enumerate(rows):
        buf[lead + v * stride:lead + v * stride + len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
    d = _lib.DeviceBuffer.from_numpy(buf)
    return d, d.ptr + lead


def _call_dev_form(b, p0, proof_stride, d_pub, pub_stride):
    """zk_bn254_plonk_verify_batch_keys_dev itself, its output buffers poisoned -> (rc, accepted bytes, *n_accepted)"""
    acc, n_acc = np.full(max(b.n, 1), 0xEE, np.uint8), C.c_size_t(1 << 40)
    ptrs, lens = b.key_args()
    g2 = np.ascontiguousarray(pf.srs_g2()[1], dtype=np.uint64)
    ko = np.ascontiguousarray(b.key_of, dtype=np.uint32)
    rc = _lib.lib().zk_bn254_plonk_verify_batch_keys_dev(p0, proof_stride, b.n, ptrs, lens, len(b.keys), 0, _lib.vp(g2), _lib.vp(ko),
                                                         d_pub.ptr if d_pub is not None else None, pub_stride, _lib.vp(acc), C.addressof(n_acc))
    return rc, acc[:b.n], n_acc.value


def _run_dev(rows, proof_stride, pub_stride, extra=()):
    """the same batch through the device form, rows `proof_stride` bytes apart with poison between them: the host form's verdicts, and the expected ones;
    *n_accepted their count; a second call gives the same bytes; the Python wrapper says the same"""
    b = kc.Batch(rows, pub_stride, extra)
    rc, host, _ = kc.call_host_form(b, b.pubs())
    assert rc == _lib.ZK_OK
    d_proofs, p0 = _rows_on_device([c.proof for c, _ in b.rows], proof_stride, proof_stride % 4, 0xD7)
    d_pub = _lib.DeviceBuffer.from_numpy(b.pubs(0x0DDBA11C0FFEE000)) if b.stride else None
    (rc, dev, n_acc), prof = _profiled(lambda: _call_dev_form(b, p0, proof_stride, d_pub, pub_stride))
    assert rc == _lib.ZK_OK, (_lib.lib().zk_last_error() or b"").decode()
    wrong = ["lane %d of %d: %s: device form %d, host form %d, expected %d" % (i, b.n, c.label, dev[i], host[i], b.expect[i])
             for i, (c, _) in enumerate(b.rows) if not (int(dev[i]) == int(host[i]) == int(b.expect[i]))]
    assert not wrong, wrong[:12]
    assert n_acc == int(dev.sum()) == int(b.expect.sum())
    assert "rows_digest_keys" in prof
    rc2, dev2, n_acc2 = _call_dev_form(b, p0, proof_stride, d_pub, pub_stride)
    assert rc2 == _lib.ZK_OK and dev2.tobytes() == dev.tobytes() and n_acc2 == n_acc
    wrapped = zv.plonk_verify_batch_keys_dev(p0, proof_stride, b.n, [k.bytes for k in b.keys], b.key_of, pf.srs_g2()[1], d_pub, pub_stride)
    assert (wrapped == dev.astype(bool)).all()
    return prof


def _mixed(n, how):
    ks = kc.np1_keys()
    K = len(ks)
    key_of = [i % K for i in range(n)] if how == "interleaved" else [min(i * K // max(n, 1), K - 1) if n >= K else i for i in range(n)]
    return kc.tiled_accepts(ks, key_of)


def _npub_rows(seed=0):
    """two accepts of every key of pf.N_PUBLIC, keys interleaved"""
    ks = [pf.n_public_key(n) for n in pf.N_PUBLIC]
    return kc.tiled_accepts(ks, [(i + seed) % len(ks) for i in range(2 * len(ks))])


def _reject_rows():
    """176 mixed-key accepts (every key with one public input, and the base key), each key's opening reject, and ALL of the base key's rejects that are invalid
    before the pairing: the identity rejects, every flag-loss representative (nine slots, four classes of encoding each) and the header rejects"""
    rows = _mixed(160, "interleaved") + kc.tiled_accepts([pf.base_key()], [0] * 16)
    opening = [(pf.opening_reject(k), None) for k in kc.np1_keys()]
    early = [c for c in pf.identity_rejects() + pf.flag_loss_representatives() + pf.header_rejects() if c.key is pf.base_key()]
    assert len(early) == 3 + 36 + 2 and len(opening) == 16
    return rows, opening, [(c, None) for c in early]


def _put(cases, rejects, first, step):
    """rejects[j] on lane first + step * j, each on a lane of its own"""
    assert first + step * (len(rejects) - 1) < len(cases)
    for j, r in enumerate(rejects):
        cases[first + step * j] = r


# ---------------------------------------------------------------------------------------------------------------- one key
def test_one_key_is_the_single_key_verifier():
    """K = 1: the base key's table, verdicts as expected; its accepts alone are decided by the combined check"""
    cases = pf.table()["base"]
    good = [c for c in cases if c.expect]
    assert good and len(good) < len(cases)
    assert _combined_only(_run([(c, None) for c in good]))
    assert _combined_only(_run([(good[0], None)], again=False))
    prof = _run([(c, None) for c in cases])
    assert _fell_back(prof)
    _run([(c, None) for c in cases], again=False, wide=True)


# ---------------------------------------------------------------------------------------------------------------- mixed keys
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_mixed_keys_all_accepts(n):
    """every key with one public input -- S1 and S2 at infinity, Ql = Qr, 2 to 2^28 rows -- in one batch, interleaved and in blocks: all accepted, and by the
    combined check alone (each lane read its own key's S1, S2, omega, u, log_n)"""
    for how in ("interleaved", "blocks"):
        rows = _mixed(n, how)
        assert len({k.name for _, k in rows}) == min(n, 16)
        assert _combined_only(_run(rows, again=how == "blocks")), (n, how)
    if n <= 3:                                       # every key as lane 0, and alone
        ks = kc.np1_keys()
        for j in range(len(ks)):
            rows = kc.tiled_accepts(ks, [(j + i) % len(ks) for i in range(n)])
            assert _combined_only(_run(rows, again=False)), (n, j)


@pytest.mark.parametrize("stride", [64, 70])
def test_mixed_n_public(stride):
    """0 to 64 public inputs in one batch at one stride; what lies behind a row's own inputs is garbage that differs between the two calls"""
    rng = np.random.default_rng(stride)
    for wide in (False, True):
        rows = _npub_rows(int(wide))
        assert sorted({k.n_public for _, k in rows}) == sorted(pf.N_PUBLIC)
        assert _combined_only(_run(rows, stride, wide=wide, fill=rng)), (stride, wide)
    # another row's public inputs are refused: rows 1 and 8 are of one key
    b = kc.Batch(_npub_rows(), stride)
    assert b.key_of[1] == b.key_of[8] and b.keys[b.key_of[1]].n_public == 1
    pubs = b.pubs()
    pubs[[1, 8]] = pubs[[8, 1]]
    rc, acc, n_acc = kc.call_host_form(b, pubs)
    want = np.ones(b.n, np.uint8)
    want[[1, 8]] = 0
    assert rc == _lib.ZK_OK and (acc == want).all() and n_acc == b.n - 2
    # only the LAST public input of the widest row differs
    at = next(i for i, (_, k) in enumerate(b.rows) if k.n_public == 64)
    pubs = b.pubs()
    pubs[at, 63] = pf.limbs([5])[0]
    rc, acc, n_acc = kc.call_host_form(b, pubs)
    assert rc == _lib.ZK_OK and list(np.flatnonzero(acc == 0)) == [at] and n_acc == b.n - 1


# ---------------------------------------------------------------------------------------------------------------- rejects
def test_rejects_stay_local():
    rows, opening, early = _reject_rows()
    # invalid before the pairing, every one beside lanes of other keys, the first and the last lane among them: the combined check still decides
    cases = list(rows)
    _put(cases, early, 3, 4)
    cases[0], cases[-1] = early[0], early[-1]
    assert _combined_only(_run(cases, stride=2))
    # one opening reject at a time, first, in the middle and last: the chunk falls back, every other lane keeps its verdict
    for j, r in enumerate(opening):
        cases = list(rows)
        cases[(0, len(rows) // 2 + j, len(rows) - 1)[j % 3]] = r
        assert _fell_back(_run(cases, stride=2, again=j == 0)), r[0].label
    # every kind at once: the early rejects on odd lanes, the opening rejects on even ones
    cases = list(rows)
    _put(cases, early, 3, 4)
    _put(cases, opening, 2, 4)
    assert _fell_back(_run(cases, stride=2))
    # no valid lane at all
    _run(early, again=False)
    _run(opening, again=False)


def test_wrong_key():
    """rows that are accepts for their own key, verified against another key of as many public inputs: rejected (on which path is the row's business)"""
    wrong = kc.wrong_key_rows()
    right = [(c, None) for c, _ in wrong[:16]]
    _run(wrong)
    for j in (0, 5, 9, 15, 16, 31):
        _run([wrong[j]], again=False)
    # two rows with their keys swapped: key 9's accept under key 10 and key 10's under key 9
    swap = [wrong[9], wrong[16 + 10]]
    assert swap[0][0].key is swap[1][1] and swap[1][0].key is swap[0][1]
    _run(swap, again=False)
    _run(right[:4] + swap + right[4:8], again=False)
    # one wrong row among 64 right ones
    fill = _mixed(64, "interleaved")
    for at in (0, 33, 64):
        _run(fill[:at] + [wrong[(at + 2) % len(wrong)]] + fill[at:], again=False)


def test_cross_key_cancelling_pairs():
    """two lanes under two keys whose opening errors cancel when the lanes share a coefficient: both rejected, wherever they stand, by the fallback"""
    fill = _mixed(257, "interleaved")
    for i, p in enumerate(kc.cross_key_pairs()):
        a, b = [(m, None) for m in p.members]
        for at_a, at_b in ((100, 101), (70 + i, 134 + i), (0, 256)):
            cases = list(fill)
            cases[at_a], cases[at_b] = a, b
            assert _fell_back(_run(cases, again=False)), (p.label, at_a, at_b)
        assert _fell_back(_run([a, b])), p.label
        assert _fell_back(_run([b, a], again=False)), p.label


# ---------------------------------------------------------------------------------------------------------------- the key table
def test_many_keys():
    """300 keys, one row each, key_of a fixed permutation: the table is indexed per lane, far past a wave's 64 lanes"""
    keys, rej = kc.many_keys()
    perm = np.random.default_rng(300).permutation(kc.MANY)
    extra = tuple(k for k, _ in keys)
    rows = [(keys[j][1], keys[j][0]) for j in perm]
    b = kc.Batch(rows, extra=extra)
    assert len(b.keys) == 300 and (b.key_of == perm).all()
    assert _combined_only(_run(b))
    at = int(np.flatnonzero(perm == kc.MANY - 1)[0])
    rows[at] = (rej, None)
    b = kc.Batch(rows, extra=extra)
    assert b.expect.sum() == 299 and b.expect[at] == 0
    assert _fell_back(_run(b))


def test_unused_and_repeated_keys():
    ks = kc.np1_keys()
    five = (ks[2], ks[0], pf.n_public_key(33), ks[9], ks[12])        # only keys 1 and 3 are referred to; an unused key sets the least stride
    rows = kc.tiled_accepts(five, [1, 3, 3, 1, 1, 3, 1])
    b = kc.Batch(rows, extra=five)
    assert len(b.keys) == 5 and sorted(set(b.key_of)) == [1, 3] and b.stride == 33
    assert _combined_only(_run(b))
    # the same key's bytes twice, the rows split between the two indices
    k = ks[0]
    rows = kc.tiled_accepts([k], [0] * 6) + [(pf.opening_reject(k), None)]
    b = kc.Batch(rows)
    b.keys = [k, k]
    for key_of in ([0, 1, 0, 1, 0, 1, 1], [1, 1, 1, 0, 0, 0, 0]):
        b.key_of = np.array(key_of, np.uint32)
        (rc, acc, n_acc), prof = _profiled(lambda: kc.call_host_form(b, b.pubs()))
        assert rc == _lib.ZK_OK and list(acc) == [1] * 6 + [0] and n_acc == 6 and _fell_back(prof)
    b = kc.Batch(rows[:6])
    b.keys, b.key_of = [k, k], np.array([0, 1, 1, 0, 1, 0], np.uint32)
    (rc, acc, n_acc), prof = _profiled(lambda: kc.call_host_form(b, b.pubs()))
    assert rc == _lib.ZK_OK and acc.all() and n_acc == 6 and _combined_only(prof)


# ---------------------------------------------------------------------------------------------------------------- chunks
def _chunk_batch(with_pair):
    """2^16 + 3 rows tiled from a few accepts of two keys, key_of alternating (so the key changes across the chunk boundary): a cross-key cancelling pair on
    lanes 1 and 2^16 + 1, an identity reject (of a third key) as the last lane"""
    pair = kc.cross_key_pairs()[0].members
    ka, kb = pair[0].key, pair[1].key
    ident = pf.identity_rejects()[0]
    assert ident.key.n_public == 2
    distinct = kc.accepts_of(ka)[:2] + kc.accepts_of(kb)[:2] + list(pair) + [ident]
    keys = [ka, kb, ident.key]
    n = CHUNK + 3
    idx = np.where(np.arange(n) % 2 == 0, (np.arange(n) // 2) % 2, 2 + (np.arange(n) // 2) % 2)        # even lanes: key A's accepts, odd lanes: key B's
    if with_pair:
        idx[1], idx[CHUNK + 1] = 5, 4                 # lane 1 is odd: key B's member; lane 2^16 + 1 is odd too: put key A's member there
    idx[n - 1] = 6
    key_of = np.array([0, 0, 1, 1, 0, 1, 2], np.uint32)[idx]
    assert key_of[CHUNK - 1] != key_of[CHUNK]
    blob = np.frombuffer(b"".join(c.proof for c in distinct), np.uint8).reshape(-1, 548)[idx].tobytes()
    pubs = np.full((len(distinct), 2, 4), 0x5EED5EED5EED5EED, np.uint64)
    for j, c in enumerate(distinct):
        pubs[j, :c.key.n_public] = c.pub
    want = np.array([c.expect for c in distinct], np.uint8)[idx]
    return keys, key_of, blob, np.ascontiguousarray(pubs[idx]), want


def _call_chunk(keys, key_of, blob, pubs):
    b = kc.Batch([])
    b.keys, b.key_of, b.blob, b.n = keys, key_of, blob, len(key_of)
    return kc.call_host_form(b, pubs)


def test_chunk_edge():
    keys, key_of, blob, pubs, want = _chunk_batch(True)
    assert want.sum() == CHUNK + 3 - 3
    (rc, acc, n_acc), prof = _profiled(lambda: _call_chunk(keys, key_of, blob, pubs))
    assert rc == _lib.ZK_OK
    assert (acc == want).all(), np.flatnonzero(acc != want)[:12]
    assert n_acc == int(acc.sum()) == CHUNK
    assert prof["pvk_kzg"][0] == 2 and prof["pvk_single"][0] == 2          # both chunks fell back: each holds one member of the pair
    rc2, acc2, n_acc2 = _call_chunk(keys, key_of, blob, pubs)
    assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc


def test_chunk_edge_without_an_opening_error():
    keys, key_of, blob, pubs, want = _chunk_batch(False)
    assert want.sum() == CHUNK + 2
    (rc, acc, n_acc), prof = _profiled(lambda: _call_chunk(keys, key_of, blob, pubs))
    assert rc == _lib.ZK_OK and (acc == want).all(), np.flatnonzero(acc != want)[:12]
    assert n_acc == CHUNK + 2 and prof["pvk_kzg"][0] == 2 and "pvk_single" not in prof
    rc2, acc2, n_acc2 = _call_chunk(keys, key_of, blob, pubs)
    assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc


# ---------------------------------------------------------------------------------------------------------------- the device form
@pytest.mark.parametrize("proof_stride, pub_stride", [(548, 64), (551, 70)])
def test_device_form(proof_stride, pub_stride):
    """the mixed-keys, mixed-n_public and rejects batches where they lie in HBM, aligned and not: the host form's verdicts"""
    for n in (1, 65):
        assert _combined_only(_run_dev(_mixed(n, "interleaved"), proof_stride, pub_stride))
    assert _combined_only(_run_dev(_npub_rows(), proof_stride, pub_stride))
    rows, opening, early = _reject_rows()
    cases = list(rows)
    _put(cases, early, 3, 4)
    assert _combined_only(_run_dev(cases, proof_stride, pub_stride))
    _put(cases, opening, 2, 4)
    assert _fell_back(_run_dev(cases, proof_stride, pub_stride))
    for p in kc.cross_key_pairs()[:1]:
        assert _fell_back(_run_dev([(m, None) for m in p.members] + rows[:3], proof_stride, pub_stride))


def test_device_form_refuses_a_stride_below_the_row():
    b = kc.Batch(_mixed(2, "interleaved"))
    d_proofs, p0 = _rows_on_device([c.proof for c, _ in b.rows], 548, 0, 0xD7)
    d_pub = _lib.DeviceBuffer.from_numpy(b.pubs())
    ptrs, lens = b.key_args()
    acc, n_acc = np.full(2, 0xEE, np.uint8), C.c_size_t(9)
    g2 = np.ascontiguousarray(pf.srs_g2()[1], dtype=np.uint64)
    fn = _lib.lib().zk_bn254_plonk_verify_batch_keys_dev
    args = lambda ps, qs: (p0, ps, 2, ptrs, lens, 2, 0, _lib.vp(g2), _lib.vp(b.key_of), d_pub.ptr, qs, _lib.vp(acc), C.addressof(n_acc))
    assert fn(*args(547, 1)) == _lib.ZK_ERR_ARG and n_acc.value == 0
    assert fn(*args(548, 0)) == _lib.ZK_ERR_LEN and n_acc.value == 0
    assert (acc == 0xEE).all()
    assert fn(*args(548, 1)) == _lib.ZK_OK and n_acc.value == 2 and acc.all()
