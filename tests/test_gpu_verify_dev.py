"""GPU suite for the device-resident forms of the batch verifiers (-m gpu): zk_bn254_groth16_verify_batch_dev / zk_bn254_plonk_verify_batch_dev take the proofs
and the public inputs where they lie in HBM -- here at a stride, with poison between the rows -- and must say, case for case, what the host-input entries say
for the same bytes and what the forge (tests/groth16_forge.py, tests/plonk_forge.py) expects by construction.  Their coefficients come from the rows' digests
(tests/verify_rows_ref.py states the derivation): pairs of proofs whose errors cancel under equal coefficients must be rejected under them too."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from tests import groth16_forge as gf
from tests import plonk_forge as pf

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 65)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


def _rows_on_device(rows, stride, lead, poison):
    """byte rows `stride` apart behind `lead` bytes, everything between them poison -> (DeviceBuffer, address of row 0)"""
    width = len(rows[0]) if rows else 0
    buf = np.full(lead + max(len(rows), 1) * stride + 64, poison, np.uint8)
    for v, r in enumerate(rows):
        assert len(r) == width <= stride
        buf[lead + v * stride:lead + v * stride + width] = np.frombuffer(bytes(r), dtype=np.uint8)
    d = _lib.DeviceBuffer.from_numpy(buf)
    return d, d.ptr + lead


def _profiled(fn):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        out = fn()
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    return out, prof


def _check(system, cases, gap=(24, 2, 4)):
    """one batch (one key) through the host-input entry and through the device form: the same verdicts, and the forge's.  gap: bytes between the proofs, elements
    between the rows of public inputs, bytes in front of the first proof (a multiple of four keeps the rows word-aligned, any other value does not)"""
    key = cases[0].key
    assert all(c.key is key for c in cases)
    n, np_ = len(cases), key.n_public
    width = 128 if system == "groth16" else 548
    pubs = np.stack([c.pub for c in cases]).reshape(n, np_, 4) if np_ else np.zeros((n, 0, 4), np.uint64)
    proofs = [c.proof for c in cases]
    if system == "groth16":
        host = zv.groth16_verify_batch(proofs, key.bytes, pubs)
    else:
        host = zv.plonk_verify_batch(proofs, key.bytes, key.g2, pubs)
    d_proofs, p0 = _rows_on_device(proofs, width + gap[0], gap[2], 0xD7)
    pub_stride = np_ + gap[1]
    pad = np.full((n, pub_stride, 4), 0xBADC0FFEE0DDF00D, np.uint64)
    pad[:, :np_] = pubs
    d_pub = _lib.DeviceBuffer.from_numpy(pad)
    if system == "groth16":
        dev, prof = _profiled(lambda: zv.groth16_verify_batch_dev(p0, width + gap[0], n, key.bytes, d_pub, pub_stride, np_))
    else:
        dev, prof = _profiled(lambda: zv.plonk_verify_batch_dev(p0, width + gap[0], n, key.bytes, key.g2, d_pub, pub_stride, np_))
    expect = [bool(c.expect) for c in cases]
    wrong = ["lane %d of %d: %s: device form %d, host-input entry %d, expected %d" % (i, n, c.label, dev[i], host[i], c.expect)
             for i, c in enumerate(cases) if not (dev[i] == host[i] == expect[i])]
    assert not wrong, wrong[:12]
    assert "rows_digest" in prof                     # the coefficients came from the rows' digests
    return prof


def _fallback_ran(system, prof):
    return ("vb_single" if system == "groth16" else "pv_single") in prof


def _sets(system):
    """(valid cases, well-formed rejects, malformed encodings) of one key"""
    if system == "groth16":
        k = gf.KEY
        good = gf.good_cases(k, 8) + [c for c in gf.accept_cases()["two public inputs"]]
        bad = [gf.reject_case(k, seed=s) for s in (7, 8, 9)]
        malformed = gf.flag_loss_representatives()
    else:
        k = pf.base_key()
        good = pf.good_cases(k, 8) + pf.base_accepts()[:12]
        bad = [pf.opening_reject(k, seed=s) for s in (5, 6, 7)] + [c for c in pf.identity_rejects() if c.key is k]
        malformed = [c for c in pf.flag_loss_representatives() + pf.header_rejects() if c.key is k]
    assert all(c.expect for c in good) and not any(c.expect for c in bad + malformed) and len(malformed) >= 8
    return good, bad, malformed


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("system", ["groth16", "plonk"])
def test_device_form_agrees_with_the_host_input_entry(system, n):
    good, bad, malformed = _sets(system)
    tile = lambda cs, start=0: [cs[(start + j) % len(cs)] for j in range(n)]
    # all valid: the combined check decides
    for gap in ((24, 2, 4), (5, 0, 1), (0, 0, 0)):
        assert not _fallback_ran(system, _check(system, tile(good, n), gap)), gap
    # one invalid among valid -- every point of it decodes, only the pairings refuse it: the fallback decides (at n = 1 it is the one proof)
    cases = tile(good)
    cases[n // 2] = bad[0]
    assert _fallback_ran(system, _check(system, cases))
    if n > 2:
        cases[0], cases[n - 1] = bad[1], bad[2]
        assert _fallback_ran(system, _check(system, cases, (3, 1, 2)))
    # all invalid
    _check(system, tile(bad))
    _check(system, tile(bad + malformed, 3), (7, 3, 3))
    # malformed encodings beside valid ones: their lanes are out before the pairing, the valid ones still pass the combined check
    cases = tile(good, 5)
    for j, at in enumerate(sorted({0, n - 1, n // 2} | set(range(1, n, 6)))):
        cases[at] = malformed[(j + n) % len(malformed)]
    if n == 2:
        cases[1] = good[1]
    prof = _check(system, cases)
    if n > 1:
        assert not _fallback_ran(system, prof)
    if n == 1:
        for c in malformed:
            _check(system, [c])


def test_keys_without_public_inputs_and_with_three():
    """n_public = 0: the rows' digests are the proofs' alone and no public-input pointer is read; three public inputs under PLONK's PI(zeta)"""
    cs = gf.accept_cases()["no public input"]
    assert cs[0].key.n_public == 0
    _check("groth16", cs + [gf.reject_case(cs[0].key)] + cs[:2])
    k0 = pf.n_public_key(0)
    _check("plonk", pf.n_public_cases(0) + [pf.opening_reject(k0)])
    k3 = pf.pi_key()
    _check("plonk", pf.good_cases(k3, 3) + [c for c in pf.identity_rejects() if c.key is k3] + pf.key_accepts()[k3.name])


def test_errors_that_cancel_under_equal_coefficients_are_rejected():
    """The forge's groups and pairs are built for equal coefficients (rho = 1 in every lane): each member is rejected alone and the errors multiply to one, so a
    verifier whose lanes shared a coefficient would accept them together.  The rows' coefficients are 128 bits of a digest over the very bytes of the rows, so
    no pair can be built FOR them (its errors would have to be known before the digest that fixes them); under them every member is rejected, as under the
    host-input entry's."""
    for g in gf.coefficient_groups():
        assert not any(c.expect for c in g.members)
        assert _fallback_ran("groth16", _check("groth16", list(g.members))), g.label
        assert _fallback_ran("groth16", _check("groth16", list(g.members) + gf.good_cases(gf.KEY, 3))), g.label
    for p in pf.cancelling_pairs():
        assert _fallback_ran("plonk", _check("plonk", list(p.members))), p.label
        assert _fallback_ran("plonk", _check("plonk", pf.good_cases(pf.base_key(), 2) + list(p.members))), p.label
    for c in pf.rho_cases():                         # W and W' errors of ONE proof that cancel when rho == rho'
        assert _fallback_ran("plonk", _check("plonk", [c]))
        assert _fallback_ran("plonk", _check("plonk", [c] + pf.good_cases(pf.base_key(), 1)))


def test_device_form_crosses_nothing_between_calls():
    """the same rows twice, then in another order: verdicts follow the rows"""
    good, bad, _ = _sets("plonk")
    cases = good[:3] + bad[:1] + good[3:5]
    _check("plonk", cases)
    _check("plonk", cases[::-1])
    good, bad, _ = _sets("groth16")
    cases = good[:3] + bad[:1] + good[3:5]
    _check("groth16", cases)
    _check("groth16", cases[::-1])
