"""Batch PLONK verification on the device (zk_bn254_plonk_verify_batch) against proofs forged under an SRS whose secret is known (tests/plonk_forge.py).
Every expected verdict comes from the forge's integer arithmetic and the reference decoder -- tests/test_plonk_forge_cpu.py holds the tables against the host
verifier -- never from the device.  What the real-proof tests (test_gpu_plonk_verify_batch.py) cannot see:
  identity       proofs whose two openings are right for the values they claim: only the quotient identity of k_pv_scalars rejects them
  flag loss      a refused encoding in a proof that is accepted with the point at infinity the decoder leaves behind: only the lane's flag rejects it
  coefficients   W and W' errors of one proof that cancel when rho == rho'; W errors of two proofs that cancel when the lanes share their coefficients
  accepts        points at infinity in every proof and key slot and in the two digests, a doubling and a cancellation in the digest's sum, the values 0,
                 r - 1 and non-canonical writings, through the combined check and through the per-proof fallback
  shapes         up to 64 public inputs, domains of 2 to 2^28 rows, lanes invalid before the pairing next to valid ones, a chunk edge, *n_accepted"""
import ctypes as C

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from tests import plonk_forge as pf

pytestmark = pytest.mark.gpu
CHUNK = 1 << 16


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _call(key, blob, pubs):
    """the C entry itself, its output buffers poisoned: (accepted bytes, *n_accepted)"""
    n = len(blob) // 548
    pubs = np.ascontiguousarray(pubs, dtype=np.uint64)
    assert len(blob) == 548 * n and pubs.shape == (n, key.n_public, 4)
    acc, n_acc = np.full(n, 0xEE, np.uint8), C.c_size_t(1 << 40)
    g2 = np.ascontiguousarray(key.g2, dtype=np.uint64)
    rc = _lib.lib().zk_bn254_plonk_verify_batch(C.c_char_p(blob), C.c_size_t(n), C.c_char_p(key.bytes), C.c_size_t(len(key.bytes)), C.c_int(0), _lib.vp(g2),
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


def _run(cases, again=True, wide=False):
    """one batch of cases (one key): every lane's verdict is the case's expected one, *n_accepted their count, a second call gives the same bytes.
    wide: the public inputs as Montgomery images + r"""
    key = cases[0].key
    assert all(c.key is key for c in cases)
    blob = b"".join(c.proof for c in cases)
    pubs = np.stack([pf.plus_r(c.pub) if wide else c.pub for c in cases]) if key.n_public else np.zeros((len(cases), 0, 4), np.uint64)
    acc, n_acc, prof = _profiled(key, blob, pubs)
    wrong = ["lane %d of %d: %s: got %d, expected %d" % (i, len(cases), c.label, acc[i], c.expect) for i, c in enumerate(cases) if acc[i] != c.expect]
    assert not wrong, wrong[:12]
    assert n_acc == int(acc.sum()) == sum(c.expect for c in cases)
    if again:
        acc2, n_acc2 = _call(key, blob, pubs)
        assert acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc
    return prof


def _combined_only(prof):
    """the combined check decided: no per-proof fallback ran"""
    return "pv_kzg" in prof and "pv_single" not in prof


@pytest.fixture(scope="module")
def accepts():
    return pf.base_accepts() + pf.good_cases(pf.base_key(), 8)


# ---------------------------------------------------------------------------------------------------------------- the whole table
@pytest.mark.parametrize("name", pf.KEY_NAMES)
def test_every_case_of_a_key(name):
    """the key's accepts alone (the combined check decides), each of them alone, then all of its cases in one batch (its rejects send it through the fallback)"""
    cases = pf.table()[name]
    good = [c for c in cases if c.expect]
    assert good and len(good) < len(cases)
    assert _combined_only(_run(good))
    if name != "base":                               # (the base key's accepts one by one: test_accepts_at_every_batch_size and the cases below)
        for c in good:
            assert _combined_only(_run([c], again=False))
    prof = _run(cases)
    assert "pv_single" in prof                       # every key has an opening reject: a valid lane that the pairings refuse
    if cases[0].key.n_public:
        _run(cases, again=False, wide=True)


@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 257])
def test_accepts_at_every_batch_size(n, accepts):
    """the base key's accepts tiled to n lanes, starting at another one for each size: all accepted by the combined check alone"""
    for start in ((0, 7, 23) if n <= 3 else (n % len(accepts),)):
        cases = [accepts[(start + j) % len(accepts)] for j in range(n)]
        assert _combined_only(_run(cases, again=n == 257)), (n, start)
    if n == 1:
        for c in accepts:
            assert _combined_only(_run([c], again=False)), c.label


# ---------------------------------------------------------------------------------------------------------------- invalid before the pairing
def test_lanes_invalid_before_the_pairing_leave_the_combined_check_alone(accepts):
    """identity-only, flag-loss and header rejects among accepts: k_pv_smul gives an invalid lane the point at infinity and k_pv_kzg gives it zero
    coefficients, so the valid lanes still pass the combined check and no fallback runs.  Each batch follows an all-accept batch of its size, which leaves
    non-zero scalars where the invalid lanes' are to be written"""
    invalid = pf.identity_rejects() + pf.flag_loss_representatives() + pf.header_rejects()
    invalid = [c for c in invalid if c.key is pf.base_key()]
    assert len(invalid) == 3 + 36 + 2
    for n in (2, 3, 64, 65, 257):
        fill = [accepts[j % len(accepts)] for j in range(n)]
        assert _combined_only(_run(fill, again=False))
        cases = list(fill)
        spots = sorted({0, n - 1, n // 2, 63 % n, 64 % n} | set(range(1, n, 5)))
        for j, at in enumerate(spots):
            cases[at] = invalid[(j + n) % len(invalid)]
        if n <= 3:
            cases[1] = fill[1]
        assert any(c.expect for c in cases)
        assert _combined_only(_run(cases)), n
    # every one of them next to one accept, and the PI cases under their own key
    for j, c in enumerate(invalid):
        assert _combined_only(_run([c, accepts[j % len(accepts)]] if j % 2 else [accepts[j % len(accepts)], c], again=False)), c.label
    pi = [c for c in pf.identity_rejects() if c.key is pf.pi_key()]
    assert len(pi) == 2
    assert _combined_only(_run(pf.good_cases(pf.pi_key(), 3) + pi + pf.good_cases(pf.pi_key(), 2, seed=2)))
    # no valid lane at all: every verdict 0
    _run(invalid)
    for c in pf.identity_rejects():
        _run([c], again=False)


@pytest.mark.parametrize("slot", list(pf.POINT_SLOTS))
def test_flag_loss_every_encoding(slot, accepts):
    """all of a slot's refused encodings in one batch, an accept every eighth lane: decided by the combined check (a lost flag would leave the lane valid and
    its point at infinity would pass), then with one opening reject, which sends every valid lane through the fallback"""
    cases = []
    for c in pf.flag_loss_cases(slot):
        if len(cases) % 8 == 0:
            cases.append(accepts[(len(cases) // 8) % len(accepts)])
        cases.append(c)
    assert _combined_only(_run(cases))
    mid = len(cases) // 2
    prof = _run(cases[:mid] + [pf.opening_rejects()[0]] + cases[mid:], again=False)
    assert "pv_single" in prof


# ---------------------------------------------------------------------------------------------------------------- coefficients
def test_opening_errors_take_the_fallback_and_never_cancel(accepts):
    n = 257
    fill = [accepts[j % len(accepts)] for j in range(n)]
    singles = pf.opening_rejects()
    assert len(pf.rho_cases()) == 2
    for j, c in enumerate(singles):                                       # W + d G, W' + d G, and the two that cancel when rho == rho'
        for at in (0, 100 + j, n - 1):
            cases = list(fill)
            cases[at] = c
            assert "pv_single" in _run(cases, again=at == 0), c.label
        assert "pv_single" in _run([c]), c.label
    for i, p in enumerate(pf.cancelling_pairs()):                           # two lanes that cancel under one coefficient: next to each other, a block
        a, b = p.members                                                  # of 64 apart, at both ends, alone, alone in the other order
        for at_a, at_b in ((100, 101), (70 + i, 134 + i), (0, n - 1), (64, 0)):
            cases = list(fill)
            cases[at_a], cases[at_b] = a, b
            assert "pv_single" in _run(cases, again=False), (p.label, at_a, at_b)
        assert "pv_single" in _run([a, b]), p.label
        assert "pv_single" in _run([b, a], again=False), p.label
        assert "pv_single" in _run([a] + fill[:63] + [b], again=False), p.label        # lanes 0 and 64 of 65
    everything = list(fill)
    for j, c in enumerate(singles + [m for p in pf.cancelling_pairs() for m in p.members]):
        everything[3 + 25 * j] = c
    assert "pv_single" in _run(everything)


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n_public", pf.N_PUBLIC)
def test_public_input_counts(n_public):
    """k_pv_transcript hashes n_public + 6 items and k_pv_scalars sums n_public terms of PI(zeta); public inputs 0, r - 1, random, and as images + r"""
    cases, rej = pf.n_public_cases(n_public), pf.opening_reject(pf.n_public_key(n_public))
    assert cases[0].pub.shape == (n_public, 4)
    for wide in ((False, True) if n_public else (False,)):
        assert _combined_only(_run(cases, again=False, wide=wide))
        assert _combined_only(_run(cases[:1], again=False, wide=wide))
        assert "pv_single" in _run(cases[:2] + [rej] + cases[2:], wide=wide)
    if n_public:                                                           # another proof's public inputs: rejected (the identity, or the transcript)
        key = cases[0].key
        blob = b"".join(c.proof for c in cases)
        pubs = np.stack([cases[(j + 1) % len(cases)].pub for j in range(len(cases))])
        acc, n_acc = _call(key, blob, pubs)
        assert not acc.any() and n_acc == 0
        if n_public >= 2:                                                  # only the LAST public input differs (the first n_public - 1 are the proof's own)
            pubs = np.stack([c.pub for c in cases])
            pubs[0][-1] = pf.limbs([5])[0]
            acc, n_acc = _call(key, blob, pubs)
            assert list(acc) == [0] + [1] * (len(cases) - 1) and n_acc == len(cases) - 1


@pytest.mark.parametrize("log_n", pf.LOG_N)
def test_domain_sizes(log_n):
    """zeta^n by log_n squarings, up to the largest size the key reader takes (2^28)"""
    cases, rej = pf.log_n_cases(log_n), pf.opening_reject(pf.log_n_key(log_n))
    assert cases[0].key.n == 1 << log_n and int.from_bytes(cases[0].key.bytes[:8], "big") == 1 << log_n
    assert _combined_only(_run(cases))
    assert "pv_single" in _run(cases + [rej], again=False)
    assert _combined_only(_run(cases, again=False, wide=True))


# ---------------------------------------------------------------------------------------------------------------- chunks
def test_chunk_edge():
    """2^16 + 3 proofs tiled from a few: a cancelling pair 2^16 lanes apart (lanes 1 and 2^16 + 1), a flag-loss case as the last lane of the first chunk,
    an identity-only reject as the last lane of all"""
    key = pf.base_key()
    pair = pf.cancelling_pairs()[0].members
    distinct = pf.good_cases(key, 8) + list(pair) + [pf.flag_loss_cases("Z")[5], pf.identity_rejects()[0]]
    idx = np.arange(CHUNK + 3) % 8
    idx[1], idx[CHUNK + 1] = 8, 9
    idx[CHUNK - 1] = 10
    idx[CHUNK + 2] = 11
    blob = np.frombuffer(b"".join(c.proof for c in distinct), np.uint8).reshape(-1, 548)[idx].tobytes()
    pubs = np.stack([c.pub for c in distinct])[idx]
    want = np.array([c.expect for c in distinct], np.uint8)[idx]
    assert want.sum() == CHUNK + 3 - 4
    acc, n_acc, prof = _profiled(key, blob, pubs)
    wrong = [i for i in np.flatnonzero(acc != want)[:12]]
    assert not wrong, ["lane %d: %s: got %d" % (i, distinct[idx[i]].label, acc[i]) for i in wrong]
    assert n_acc == int(acc.sum()) == CHUNK - 1
    assert prof["pv_kzg"][0] == 2 and prof["pv_single"][0] == 2            # both chunks fell back: each holds one member of the pair
    acc2, n_acc2 = _call(key, blob, pubs)
    assert acc2.tobytes() == acc.tobytes() and n_acc2 == n_acc


def test_chunk_edge_without_an_opening_error():
    """the same batch without the pair: the flag-loss lane 2^16 - 1 and the identity-only last lane leave both chunks to the combined check"""
    key = pf.base_key()
    distinct = pf.good_cases(key, 8) + [pf.flag_loss_cases("W'")[-1], pf.identity_rejects()[1]]
    idx = np.arange(CHUNK + 3) % 8
    idx[CHUNK - 1] = 8
    idx[CHUNK + 2] = 9
    blob = np.frombuffer(b"".join(c.proof for c in distinct), np.uint8).reshape(-1, 548)[idx].tobytes()
    pubs = np.stack([c.pub for c in distinct])[idx]
    acc, n_acc, prof = _profiled(key, blob, pubs)
    want = np.ones(CHUNK + 3, np.uint8)
    want[[CHUNK - 1, CHUNK + 2]] = 0
    assert (acc == want).all(), np.flatnonzero(acc != want)[:12]
    assert n_acc == CHUNK + 1 and prof["pv_kzg"][0] == 2 and "pv_single" not in prof
