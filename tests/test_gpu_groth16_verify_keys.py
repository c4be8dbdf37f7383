"""Batch Groth16 verification against many keys in one device call (zk_bn254_groth16_verify_batch_keys and its _dev form; -m gpu).  Every expected verdict
comes from tests/groth16_forge.py and tests/groth16_keys_cases.py -- a case's own verdict under its own key, 0 under another -- which
tests/test_groth16_forge_cpu.py and tests/test_groth16_verify_keys_cpu.py hold against the host verifier; never from the device.  The launch name vbk_single
means "the per-lane fallback ran": an all-accept batch must be decided WITHOUT it, because a lane that read another key's alpha, K table, n_public or
G2 points still gets its right verdict through the fallback."""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from tests import groth16_forge as gf
from tests import groth16_keys_cases as kc

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
    return "vbk_prep" in prof and "vbk_single" not in prof and "vb_prep" not in prof and "vb_single" not in prof


def _fell_back(prof):
    return "vbk_prep" in prof and "vbk_single" in prof and "vb_prep" not in prof


def _run(rows, stride=None, extra=(), again=True, wide=False, fill=0xBADC0FFEE0DDF00D):
    """one batch through the host form: every lane's verdict is the expected one, *n_accepted their count, a second call gives the same bytes"""
    b = rows if isinstance(rows, kc.Batch) else kc.Batch(rows, stride, extra)
    (rc, acc, n_acc), prof = _profiled(lambda: kc.call_host_form(b, b.pubs(fill, wide)))
    assert rc == _lib.ZK_OK, (_lib.lib().zk_last_error() or b"").decode()
    wrong = ["lane %d of %d: %s under key %d: got %d, expected %d" % (i, b.n, c.label, b.key_of[i], acc[i], b.expect[i]) for i, (c, k) in enumerate(b.rows)
             if acc[i] != b.expect[i]]
    assert not wrong, wrong[:12]
    assert n_acc == int(acc.sum()) == int(b.expect.sum())
    if again:
        rc2, acc2, n_acc2 = kc.call_host_form(b, b.pubs(fill, wide))
        assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc
    if b.expect.all():                               # all accepts: the combined check alone
        assert _combined_only(prof), sorted(prof)
    return prof


def _rows_on_device(rows, stride, lead, poison):
    buf = np.full(lead + max(len(rows), 1) * stride + 64, poison, np.uint8)
    for v, r in enumerate(rows):
        buf[lead + v * stride:lead + v * stride + len(r)] = np.frombuffer(bytes(r), dtype=np.uint8)
    d = _lib.DeviceBuffer.from_numpy(buf)
    return d, d.ptr + lead


def _call_dev_form(b, p0, proof_stride, d_pub, pub_stride):
    """zk_bn254_groth16_verify_batch_keys_dev itself, its output buffers poisoned -> (rc, accepted bytes, *n_accepted)"""
    acc, n_acc = np.full(max(b.n, 1), 0xEE, np.uint8), C.c_size_t(1 << 40)
    ptrs, lens = b.key_args()
    ko = np.ascontiguousarray(b.key_of, dtype=np.uint32)
    rc = _lib.lib().zk_bn254_groth16_verify_batch_keys_dev(p0, proof_stride, b.n, ptrs, lens, len(b.keys), 0, _lib.vp(ko),
                                                           d_pub.ptr if d_pub is not None else None, pub_stride, _lib.vp(acc), C.addressof(n_acc))
    return rc, acc[:b.n], n_acc.value


def _run_dev(rows, proof_stride, pub_stride, extra=()):
    """the same batch through the device form, rows `proof_stride` bytes apart with poison between them and a misaligned lead: the host form's verdicts, and
    the expected ones; *n_accepted their count; a second call gives the same bytes; the Python wrapper says the same"""
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
    assert "vbk_rows_digest" in prof and "rows_digest" not in prof
    rc2, dev2, n_acc2 = _call_dev_form(b, p0, proof_stride, d_pub, pub_stride)
    assert rc2 == _lib.ZK_OK and dev2.tobytes() == dev.tobytes() and n_acc2 == n_acc
    wrapped = zv.groth16_verify_batch_keys_dev(p0, proof_stride, b.n, [k.bytes for k in b.keys], b.key_of, d_pub, pub_stride)
    assert (wrapped == dev.astype(bool)).all()
    return prof


def _mixed(n, how, first=0):
    ks = kc.np2_keys()
    K = len(ks)
    key_of = [(first + i) % K for i in range(n)] if how == "interleaved" else [min(i * K // max(n, 1), K - 1) if n >= K else i for i in range(n)]
    return kc.tiled_accepts(ks, key_of)


def _npub_rows(seed=0):
    """two accepts of every key of kc.npub_keys(), keys interleaved"""
    ks = kc.npub_keys()
    return kc.tiled_accepts(ks, [(i + seed) % len(ks) for i in range(2 * len(ks))])


def _put(cases, rejects, first, step):
    """rejects[j] on lane first + step * j, each on a lane of its own"""
    assert first + step * (len(rejects) - 1) < len(cases)
    for j, r in enumerate(rejects):
        cases[first + step * j] = r


# ---------------------------------------------------------------------------------------------------------------- one key
def test_one_key_is_the_single_key_verifier():
    """K = 1: the forge's accept table and its rejects; the accepts alone are decided by the combined check; the single-key entry says the same"""
    good = gf.accept_cases()["two public inputs"]
    bad = gf.flag_loss_representatives() + [gf.reject_case(gf.KEY)] + [m for g in gf.coefficient_groups() for m in g.members]
    assert all(c.key is gf.KEY for c in good + bad) and all(c.expect == 0 for c in bad)
    assert _combined_only(_run([(c, None) for c in good]))
    assert _combined_only(_run([(good[0], None)], again=False))
    cases = [(c, None) for pair in zip(good, bad) for c in pair] + [(c, None) for c in bad[len(good):]]
    b = kc.Batch(cases)
    assert len(b.keys) == 1 and 0 < b.expect.sum() < b.n
    assert _fell_back(_run(b))
    single = zv.groth16_verify_batch(b.blob, gf.KEY.bytes, b.pubs())
    assert (single == b.expect.astype(bool)).all()


# ---------------------------------------------------------------------------------------------------------------- mixed keys
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_mixed_keys_all_accepts(n):
    """16 keys with two public inputs -- K_0 and K_1 at infinity among them -- in one batch, interleaved and in blocks: all accepted, and by the combined
    check alone (each lane's sums went to its own key's alpha, K table and G2 points)"""
    for how in ("interleaved", "blocks"):
        rows = _mixed(n, how)
        assert len({id(k) for _, k in rows}) == min(n, 16)
        assert _combined_only(_run(rows, again=how == "blocks")), (n, how)
    if n <= 3:                                       # every key as lane 0
        for j in range(16):
            assert _combined_only(_run(_mixed(n, "interleaved", j), again=False)), (n, j)


SEGMENTS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025)


def test_segment_lengths():
    """one batch in which the keys own 1 .. 1025 rows, every power-of-two tile length up to 1024 straddled (the tiles hold 16 lanes): sorted by key, and
    under a fixed permutation of the rows"""
    keys, _ = kc.many_keys()
    rows = [(keys[j][1], None) for j, m in enumerate(SEGMENTS) for _ in range(m)]
    b = kc.Batch(rows)
    assert b.n == sum(SEGMENTS) and sorted(np.bincount(b.key_of)) == list(SEGMENTS) and (np.diff(b.key_of.astype(int)) >= 0).all()
    assert _combined_only(_run(b))
    perm = np.random.default_rng(0x5E6).permutation(b.n)
    b = kc.Batch([rows[i] for i in perm])
    assert _combined_only(_run(b, again=False))
    # one bad row in the longest segment and one in a segment of a single row: every other lane keeps its verdict
    bad = list(rows)
    bad[0] = (gf.reject_case(keys[0][0]), None)
    bad[-7] = (gf.reject_case(keys[len(SEGMENTS) - 1][0]), None)
    assert _fell_back(_run(bad, again=False))


@pytest.mark.parametrize("stride", [64, 70])
def test_mixed_n_public(stride):
    """0 to 64 public inputs in one batch at one stride; what lies behind a row's own inputs is garbage that differs between the two calls"""
    rng = np.random.default_rng(stride)
    for wide in (False, True):
        rows = _npub_rows(int(wide))
        assert sorted({k.n_public for _, k in rows}) == sorted(kc.N_PUBLIC)
        assert _combined_only(_run(rows, stride, wide=wide, fill=rng)), (stride, wide)
    # another row's public inputs are refused: rows 1 and 6 are of one key
    b = kc.Batch(_npub_rows(), stride)
    assert b.key_of[1] == b.key_of[6] and b.keys[b.key_of[1]].n_public == 1
    pubs = b.pubs()
    pubs[[1, 6]] = pubs[[6, 1]]
    rc, acc, n_acc = kc.call_host_form(b, pubs)
    want = np.ones(b.n, np.uint8)
    want[[1, 6]] = 0
    assert rc == _lib.ZK_OK and (acc == want).all() and n_acc == b.n - 2
    # only the LAST public input of the widest row differs
    at = next(i for i, (_, k) in enumerate(b.rows) if k.n_public == 64)
    pubs = b.pubs()
    pubs[at, 63] = gf.limbs([5])[0]
    rc, acc, n_acc = kc.call_host_form(b, pubs)
    assert rc == _lib.ZK_OK and list(np.flatnonzero(acc == 0)) == [at] and n_acc == b.n - 1


# ---------------------------------------------------------------------------------------------------------------- rejects
def _reject_rows():
    """176 mixed-key accepts, the forge's flag-loss representatives (invalid before the pairing) and one "Krs + D" reject per key"""
    rows = _mixed(176, "interleaved")
    early = [(c, None) for c in gf.flag_loss_representatives()]
    pairing = [(gf.reject_case(k, seed=7 + j), None) for j, k in enumerate(kc.np2_keys())]
    assert 8 <= len(early) <= 40 and len(pairing) == 16
    return rows, early, pairing


def test_rejects_stay_local():
    rows, early, pairing = _reject_rows()
    # (a) invalid before the pairing, each beside lanes of other keys, the first and the last lane among them: the combined check still decides
    cases = list(rows)
    _put(cases, early, 3, 4)
    cases[0], cases[-1] = early[0], early[-1]
    assert _combined_only(_run(cases))
    # (b) one pairing reject at a time, first, in the middle and last: the chunk falls back, every other lane keeps its verdict
    for j, r in enumerate(pairing[:6]):
        cases = list(rows)
        cases[(0, len(rows) // 2 + j, len(rows) - 1)[j % 3]] = r
        assert _fell_back(_run(cases, again=j == 0)), j
    # (c) both kinds at once: the early rejects on odd lanes, the pairing rejects on even ones
    cases = list(rows)
    _put(cases, early, 3, 4)
    _put(cases, pairing, 2, 4)
    assert _fell_back(_run(cases))
    # (d) no valid lane at all
    prof = _run(early, again=False)
    assert "vbk_prep" in prof and "miller_loop" not in prof
    # (e) a key whose only row is a flag-loss reject, beside other keys' accepts
    others = [r for r in rows if r[1] is not gf.KEY]
    for at in (0, 40, len(others)):
        cases = others[:at] + [early[at % len(early)]] + others[at:]
        b = kc.Batch(cases)
        assert list(b.key_of).count(b.key_of[at]) == 1
        assert _combined_only(_run(b, again=False)), at


def test_wrong_key():
    """rows that are accepts for their own key, verified against another key of as many public inputs: rejected"""
    wrong = kc.wrong_key_rows()
    right = [(c, None) for c, _ in wrong[:16]]
    assert _fell_back(_run(wrong))
    for j in (0, 5, 15, 16, 31):
        _run([wrong[j]], again=False)
    # two rows with their keys swapped: key 9's accept under key 10 and key 10's under key 9
    swap = [wrong[9], wrong[16 + 10]]
    assert swap[0][0].key is swap[1][1] and swap[1][0].key is swap[0][1]
    _run(swap, again=False)
    _run(right[:4] + swap + right[4:8], again=False)
    # one wrong row among 64 right ones
    fill = _mixed(64, "interleaved")
    for at in (0, 33, 64):
        assert _fell_back(_run(fill[:at] + [wrong[(at + 2) % len(wrong)]] + fill[at:], again=False))


def test_cross_key_cancelling_groups():
    """two lanes under two keys whose errors cancel when the lanes share a coefficient: both rejected, wherever they stand, by the fallback"""
    fill = _mixed(257, "interleaved")
    for g in kc.cross_key_groups():
        a, b = [(m, None) for m in g.members]
        for at_a, at_b in ((100, 101), (70, 134), (0, 256)):
            cases = list(fill)
            cases[at_a], cases[at_b] = a, b
            assert _fell_back(_run(cases, again=False)), (g.label, at_a, at_b)
        assert _fell_back(_run([a, b])), g.label
        assert _fell_back(_run([b, a], again=False)), g.label


# ---------------------------------------------------------------------------------------------------------------- the key table
def test_many_keys():
    """300 keys, one row each, key_of a fixed permutation: 900 fixed lanes behind the 300 rows, the table indexed far past a wave's 64 lanes"""
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
    ks = kc.np2_keys()
    five = (ks[2], ks[0], kc.npub_keys()[3], ks[9], ks[12])          # only keys 1 and 3 are referred to; an unused key sets the least stride
    rows = kc.tiled_accepts(five, [1, 3, 3, 1, 1, 3, 1])
    b = kc.Batch(rows, extra=five)
    assert len(b.keys) == 5 and sorted(set(b.key_of)) == [1, 3] and b.stride == 33
    assert _combined_only(_run(b))
    # the same key's bytes twice, the rows split between the two indices
    k = ks[0]
    rows = kc.tiled_accepts([k], [0] * 6) + [(gf.reject_case(k), None)]
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
    lanes 1 and 2^16 + 1, a flag-loss reject (of a third key) as the last lane"""
    pair = kc.cross_key_groups()[1].members
    ka, kb = pair[0].key, pair[1].key
    loss = gf.flag_loss_representatives()[0]
    assert loss.key is not ka and loss.key is not kb and loss.key.n_public == 2
    distinct = kc.accepts_of(ka)[:2] + kc.accepts_of(kb)[:2] + list(pair) + [loss]
    keys = [ka, kb, loss.key]
    n = CHUNK + 3
    idx = np.where(np.arange(n) % 2 == 0, (np.arange(n) // 2) % 2, 2 + (np.arange(n) // 2) % 2)        # even lanes: key A's accepts, odd lanes: key B's
    if with_pair:
        idx[1], idx[CHUNK + 1] = 5, 4                 # lane 1 is odd: key B's member; lane 2^16 + 1 is odd too: put key A's member there
    idx[n - 1] = 6
    key_of = np.array([0, 0, 1, 1, 0, 1, 2], np.uint32)[idx]
    assert key_of[CHUNK - 1] != key_of[CHUNK]
    blob = np.frombuffer(b"".join(c.proof for c in distinct), np.uint8).reshape(-1, 128)[idx].tobytes()
    pubs = np.stack([c.pub for c in distinct])
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
    assert prof["vbk_prep"][0] == 2 and prof["vbk_single"][0] == 2          # both chunks fell back: each holds one member of the pair
    rc2, acc2, n_acc2 = _call_chunk(keys, key_of, blob, pubs)
    assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc


def test_chunk_edge_without_the_pair():
    keys, key_of, blob, pubs, want = _chunk_batch(False)
    assert want.sum() == CHUNK + 2
    (rc, acc, n_acc), prof = _profiled(lambda: _call_chunk(keys, key_of, blob, pubs))
    assert rc == _lib.ZK_OK and (acc == want).all(), np.flatnonzero(acc != want)[:12]
    assert n_acc == CHUNK + 2 and prof["vbk_prep"][0] == 2 and "vbk_single" not in prof
    rc2, acc2, n_acc2 = _call_chunk(keys, key_of, blob, pubs)
    assert rc2 == _lib.ZK_OK and acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc


# ---------------------------------------------------------------------------------------------------------------- the device form
@pytest.mark.parametrize("proof_stride, pub_stride", [(128, 64), (131, 70)])
def test_device_form(proof_stride, pub_stride):
    """the mixed-keys, mixed-n_public, rejects and one cross-key batch where they lie in HBM, aligned and not: the host form's verdicts"""
    for n in (1, 65):
        assert _combined_only(_run_dev(_mixed(n, "interleaved"), proof_stride, pub_stride))
    assert _combined_only(_run_dev(_npub_rows(), proof_stride, pub_stride))
    rows, early, pairing = _reject_rows()
    cases = list(rows)
    _put(cases, early, 3, 4)
    assert _combined_only(_run_dev(cases, proof_stride, pub_stride))
    _put(cases, pairing, 2, 4)
    assert _fell_back(_run_dev(cases, proof_stride, pub_stride))
    g = kc.cross_key_groups()[0]
    assert _fell_back(_run_dev([(m, None) for m in g.members] + rows[:3], proof_stride, pub_stride))


def test_device_form_refuses_a_stride_below_the_row():
    b = kc.Batch(_mixed(2, "interleaved"))
    d_proofs, p0 = _rows_on_device([c.proof for c, _ in b.rows], 128, 0, 0xD7)
    d_pub = _lib.DeviceBuffer.from_numpy(b.pubs())
    ptrs, lens = b.key_args()
    acc, n_acc = np.full(2, 0xEE, np.uint8), C.c_size_t(9)
    fn = _lib.lib().zk_bn254_groth16_verify_batch_keys_dev
    args = lambda ps, qs: (p0, ps, 2, ptrs, lens, 2, 0, _lib.vp(b.key_of), d_pub.ptr, qs, _lib.vp(acc), C.addressof(n_acc))
    assert fn(*args(127, 2)) == _lib.ZK_ERR_ARG and n_acc.value == 0
    assert fn(*args(128, 1)) == _lib.ZK_ERR_LEN and n_acc.value == 0
    assert (acc == 0xEE).all()
    assert fn(*args(128, 2)) == _lib.ZK_OK and n_acc.value == 2 and acc.all()
