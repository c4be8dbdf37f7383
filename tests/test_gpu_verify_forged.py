"""Batch Groth16 verification on the device (zk_bn254_groth16_verify_batch) against proofs forged under a key with known discrete logarithms
(tests/groth16_forge.py).  Every expected verdict comes from the forge's integer arithmetic and the reference decoders -- tests/test_groth16_forge_cpu.py
holds the tables against the host verifier -- never from the device.  What the real-proof tests (test_gpu_verify_batch.py) cannot see:
  flag loss      a malformed point in a proof that is consistent with the point at infinity the decoder leaves behind: only the lane's `bad` flag rejects it
  coefficients   groups of rejected proofs whose equations multiply to one: equal or related batch coefficients accept them
  accepts        consistent proofs and keys with points at infinity, a key without public inputs, edge public inputs, through the combined check
                 and through the per-proof fallback
  shapes         odd halvings of the folds over n_public + 1 columns and n (+ 3) lanes; chunk edges; *n_accepted"""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from tests import groth16_forge as gf

pytestmark = pytest.mark.gpu
CHUNK = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _call(key, blob, pubs):
    """the C entry itself: (accepted bytes, *n_accepted)"""
    n = len(blob) // 128
    pubs = np.ascontiguousarray(pubs, dtype=np.uint64)
    assert pubs.shape == (n, key.n_public, 4)
    acc, n_acc = np.full(n, 0xEE, np.uint8), C.c_size_t(1 << 40)
    rc = _lib.lib().zk_bn254_groth16_verify_batch(C.c_char_p(blob), C.c_size_t(n), C.c_char_p(key.bytes), C.c_size_t(len(key.bytes)), C.c_int(0),
                                                  _lib.vp(pubs) if key.n_public else None, C.c_size_t(key.n_public), _lib.vp(acc), C.byref(n_acc))
    assert rc == _lib.ZK_OK, (_lib.lib().zk_last_error() or b"").decode()
    return acc, n_acc.value


def _profiled(key, blob, pubs):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        acc, n_acc = _call(key, blob, pubs)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    return acc, n_acc, prof


def _run(cases, again=True):
    """one batch of cases (one key): every lane's verdict is the case's expected one, *n_accepted their count, a second call gives the same bytes"""
    key = cases[0].key
    assert all(c.key is key for c in cases)
    blob = b"".join(c.proof for c in cases)
    pubs = np.stack([c.pub for c in cases]) if key.n_public else np.zeros((len(cases), 0, 4), np.uint64)
    acc, n_acc, prof = _profiled(key, blob, pubs)
    wrong = ["lane %d of %d: %s: got %d, expected %d" % (i, len(cases), c.label, acc[i], c.expect) for i, c in enumerate(cases) if acc[i] != c.expect]
    assert not wrong, wrong[:12]
    assert n_acc == int(acc.sum())
    if again:
        acc2, n_acc2 = _call(key, blob, pubs)
        assert acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc
    return prof


@pytest.fixture(scope="module")
def good():
    return gf.good_cases(gf.KEY, 16)


@pytest.fixture(scope="module")
def reject():
    return gf.reject_case(gf.KEY)


# ---------------------------------------------------------------------------------------------------------------- flag loss
@pytest.mark.parametrize("slot", ["Ar", "Bs", "Krs"])
def test_flag_loss_every_vector(slot, good, reject):
    """all of a slot's refused encodings in one batch, a good proof every eighth lane: decided by the combined check (a lost flag leaves the lane
    valid, and its points at infinity pass), then again with one well-formed reject, which sends every valid lane through the fallback"""
    cases = []
    for c in gf.flag_loss_cases(slot):
        if len(cases) % 8 == 0:
            cases.append(good[(len(cases) // 8) % len(good)])
        cases.append(c)
    prof = _run(cases)
    assert "vb_prep" in prof and "vb_single" not in prof
    mid = len(cases) // 2
    prof = _run(cases[:mid] + [reject] + cases[mid:])
    assert "vb_single" in prof


@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 257])
def test_flag_loss_at_the_first_and_last_lane(n, good, reject):
    """one representative per slot and class at lane 0 and at lane n - 1 (k_vb_prep: 128 lanes per block, the decoders 128 or 256, the pairing kernels 64);
    from n = 3 on a well-formed reject in the middle sends the batch through the fallback"""
    reps = gf.flag_loss_representatives()
    assert len(reps) == 13
    for i, first in enumerate(reps):
        last = reps[(i + 1) % len(reps)]
        cases = [good[(i + j) % len(good)] for j in range(n)]
        if n >= 3:
            cases[n // 2] = reject
        cases[n - 1] = last
        cases[0] = first if n > 1 else cases[0]
        prof = _run(cases, again=False)
        assert ("vb_single" in prof) == (n >= 3), (n, i)       # n < 3: no valid lane, the chunk is refused whole


# ---------------------------------------------------------------------------------------------------------------- coefficients
def test_coefficients_differ_between_lanes(good):
    n = 257
    for g in gf.coefficient_groups():
        m = g.members
        fill = [good[j % len(good)] for j in range(n)]
        adjacent, apart = list(fill), list(fill)
        adjacent[100:100 + len(m)] = m
        apart[0], apart[n - 1] = m[0], m[-1]           # lanes 0 and 256
        if len(m) == 3:
            apart[n // 2] = m[1]
        for cases in (adjacent, apart, list(m)):
            prof = _run(cases)
            assert "vb_single" in prof, g.label


# ---------------------------------------------------------------------------------------------------------------- accepts
@pytest.mark.parametrize("name", ["two public inputs", "K_1 at infinity", "K_0 at infinity", "no public input"])
def test_accepts_with_points_at_infinity(name):
    cases = gf.accept_cases()[name]
    prof = _run(cases)
    assert "vb_prep" in prof and "vb_single" not in prof          # the combined check alone decided
    for c in cases:                                                # and each one alone
        _run([c], again=False)
    # one reject among them: the fallback (k_vb_single: K_0 or K_j at infinity, no public input) keeps every verdict
    rej = gf.reject_case(cases[0].key)
    for at in (0, len(cases) // 2, len(cases)):
        prof = _run(cases[:at] + [rej] + cases[at:], again=at == 0)
        assert "vb_single" in prof


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_public", [0, 1, 2, 33])
def test_fold_shapes(n_public):
    """k_fr_fold over n rows of n_public + 1 columns, k_g1_fold over n, k_f12_fold over n + 3 lanes: odd counts at some or every halving"""
    key = gf.key(n_public)
    pool, rej = gf.good_cases(key, 8), gf.reject_case(key)
    for n in (1, 2, 3, 5, 129):
        cases = [pool[j % len(pool)] for j in range(n)]
        prof = _run(cases, again=False)
        assert "vb_single" not in prof, (n_public, n)
        prof = _run(cases[:-1] + [rej], again=n == 129)
        assert "vb_single" in prof, (n_public, n)


# ---------------------------------------------------------------------------------------------------------------- chunks
def _tiled(distinct, idx):
    blob = np.frombuffer(b"".join(c.proof for c in distinct), np.uint8).reshape(-1, 128)[idx].tobytes()
    pubs = np.stack([c.pub for c in distinct])[idx]
    want = np.array([c.expect for c in distinct], np.uint8)[idx]
    return blob, pubs, want


def _check_chunks(distinct, idx):
    blob, pubs, want = _tiled(distinct, idx)
    acc, n_acc, prof = _profiled(gf.KEY, blob, pubs)
    wrong = [i for i in np.flatnonzero(acc != want)[:12]]
    assert not wrong, ["lane %d: %s: got %d" % (i, distinct[idx[i]].label, acc[i]) for i in wrong]
    assert n_acc == int(acc.sum()) == int(want.sum())
    acc2, n_acc2 = _call(gf.KEY, blob, pubs)
    assert acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc
    return n_acc, prof


def _chunk_distinct():
    fl = {slot: gf.flag_loss_cases(slot)[at] for slot, at in (("Ar", 5), ("Bs", -1), ("Krs", -1))}   # flags 00, a shifted point, x without a point
    distinct = gf.good_cases(gf.KEY, 8) + [fl["Ar"], fl["Bs"], fl["Krs"]]
    assert len(distinct) <= 64
    return distinct


def test_second_chunk_without_a_valid_lane():
    """2^16 + 3 proofs: the first chunk all valid, the second one three refused encodings, one per slot: sync_valid refuses it whole"""
    distinct = _chunk_distinct()
    idx = np.arange(CHUNK + 3) % 8
    idx[CHUNK:] = [8, 9, 10]
    n_acc, prof = _check_chunks(distinct, idx)
    assert n_acc == CHUNK
    assert prof["vb_prep"][0] == 2 and prof["miller_loop"][0] == 1 and "vb_single" not in prof


def test_flag_loss_at_the_last_lane_of_a_full_chunk():
    """a flag-loss case at lane 2^16 - 1; the second chunk: a good proof, a malformed Bs, a malformed Krs"""
    distinct = _chunk_distinct()
    idx = np.arange(CHUNK + 3) % 8
    idx[CHUNK - 1] = 8
    idx[CHUNK + 1:] = [9, 10]
    n_acc, prof = _check_chunks(distinct, idx)
    assert n_acc == CHUNK
    assert prof["vb_prep"][0] == 2 and prof["miller_loop"][0] == 2 and "vb_single" not in prof
