"""The device PLONK prover (csrc/plonk.hip) against the C oracle at every domain size from 2^2 to 2^16, on both sides of every per-size and per-count
decision it takes, and on structured circuits (-m gpu).  Everything is bit-exact: verifying-key digests, exported key polynomials and the 548 proof
bytes for the same circuit, solution, blinders and base array.  Circuits, blinders and the shared constants come from tests/plonk_shapes.py;
tests/test_plonk_shapes_cpu.py holds the two oracles against each other on the same families, so a mismatch here points at the device.

What runs: test_every_domain_size -- `random`, 3 public inputs, fills "full" and "half" at each log n in 2..16; test_public_input_counts -- 0, 1, 31,
32, 33, 64 public inputs at 2^7, 32 / 33 / 64 at 2^12, 40 public inputs over 3 gates at 2^6; test_structured_wires_and_wiring -- six families and
zeros+identity_perm x three blinder families at 2^6 and 2^11, one_cycle and max with random blinders at 2^13 and 2^15;
test_violations_are_reported -- three places x 2^6, 2^11, 2^14.  Not run: the other families above 2^11 (they add time, no new path), and scan plans
with K > 8, which need n >= 2^21 and stay with the 2^22 test of tests/test_gpu_plonk.py."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import plonk as zp
from noir_backend_using_gnark_amd import verify as zv
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_shapes as ps
from tests.test_gpu_plonk import _circuit, _device_srs, _vk_hex, ref_g1_decompress

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
EXPORTS = ((0, "ql"), (2, "qm"), (4, "cqk"), (5, "s1"), (7, "s3"), (8, "lqk"))


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()


@pytest.fixture(scope="module")
def bases():
    """valid points for every size of the sweep (commitments are MSMs over any bases); a case takes the first n + 3"""
    return orc.g1_gen_points(0x9E0, (1 << max(ps.SWEEP_LOG_N)) + 3)


def _oracle_key(spr, pts):
    ck = ps.c_key(orc, spr, pts)
    dig = [d.tobytes().hex() for d in ck.vk_digests()]
    return ck, dict(s=dig[0:3], ql=dig[3], qr=dig[4], qm=dig[5], qo=dig[6], qk=dig[7])


def _profiled_prove(pk, sol, bl):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        proof = zp.prove(pk, sol, bl)
        kern, _ = _lib.split_profile(_lib.profile_read())
    finally:
        _lib.profile(False)
    return proof, kern


@pytest.mark.parametrize("log_n", list(ps.SWEEP_LOG_N))
def test_every_domain_size(log_n, bases):
    """The domain filled exactly and barely more than half (n = 8: the big domain is 4 n and 8 n): setup's digests and polynomials, the proof of the
    device-built key, of the same key loaded from gnark's fields (its linearised digest by MSM, then by linearity), and with l, r, o committed against the
    Lagrange form of the bases -- from the wire values through plonk_blind_tail exactly when n + 2 >= 4096."""
    n = 1 << log_n
    for fill in ("full", "half"):
        npub = min(3, ps.rows_of(n, fill) - 1)      # 3, except on the three rows of n = 4 "half": one gate has to remain
        spr, sol = ps.circuit("random", n, npub, fill, 0x5133 + 2 * log_n + (fill == "half"))
        pts = bases[:n + 3]
        rb = zb.ResidentBases(pts)
        pk = zp.setup(_circuit(spr), rb)
        ck, want_vk = _oracle_key(spr, pts)
        assert ck.n == n and pk.vk["size"] == n and pk.vk["n_public"] == npub
        assert _vk_hex(pk.vk) == want_vk, fill
        polys = {k: ck.poly(k) for k in ck.NAMES}
        for which, name in EXPORTS:
            assert (pk.export(which, n) == polys[name]).all(), (fill, name)
        bl = M(ps.blinders("random", log_n))
        msol = M(sol)
        want = ck.prove(msol, bl)
        assert zp.prove(pk, msol, bl) == want, fill
        g = spr.constraints
        pk2 = zp.load_proving_key(log_n, npub, spr.n_vars, polys, ck.perm(), [c[5] for c in g], [c[6] for c in g], [c[7] for c in g], pk.vk, rb)
        assert zp.prove(pk2, msol, bl) == want, fill
        assert zp.prove(pk2, msol, bl) == want, fill
        pk2.lagrange_srs()
        proof, kern = _profiled_prove(pk2, msol, bl)
        assert proof == want, fill
        assert ("plonk_blind_tail" in kern) == (n + 2 >= ps.WINDOW_TABLE_MIN), (fill, sorted(kern))
        ck.free()
        pk2.free()
        pk.free()
        rb.free()


PI_CASES = ([(7, p, "full" if p & 1 else "half") for p in ps.NPUB_CASES]
            + [(12, 32, "full"), (12, 33, "half"), (12, 64, "one_short")]
            + [(6, 40, 43)])                     # more public inputs than gates: 40 and 3


@pytest.mark.parametrize("log_n,npub,fill", PI_CASES)
def test_public_input_counts(log_n, npub, fill, bases):
    """qk completed with the public inputs point by point (plonk_qk_coset, up to PLONK_PI_DIRECT_MAX of them) or by transforms (above); public values
    r - 1, 0, random in turn, so the per-point differences d_i = w_i - LQk[i] include both extremes."""
    n = 1 << log_n
    spr, sol = ps.edge_public_values(*ps.circuit("random", n, npub, fill, 0xC0 + npub + log_n))
    assert ps.domain_size(spr) == n
    pts = bases[:n + 3]
    rb = zb.ResidentBases(pts)
    pk = zp.setup(_circuit(spr), rb)
    ck, want_vk = _oracle_key(spr, pts)
    assert _vk_hex(pk.vk) == want_vk
    bl = M(ps.blinders("random", npub))
    proof, kern = _profiled_prove(pk, M(sol), bl)
    assert proof == ck.prove(M(sol), bl)
    assert ("plonk_qk_coset" in kern) == (npub <= ps.PI_DIRECT_MAX), sorted(kern)
    ck.free()
    pk.free()
    rb.free()


STRUCT_CASES = ([(f, b, k, "one_short", 0 if f == "one_cycle" else 2) for f in ps.FAMILIES for b in ps.BLINDER_FAMILIES for k in (6, 11)]
                + [("zeros+identity_perm", b, k, "full", 0) for b in ps.BLINDER_FAMILIES for k in (6, 11)]      # the permutation IS the identity: z = 1
                + [(f, "random", k, "one_short", 0 if f == "one_cycle" else 2) for f in ("one_cycle", "max") for k in (13, 15)])


@pytest.mark.parametrize("family,blinders,log_n,fill,npub", STRUCT_CASES)
def test_structured_wires_and_wiring(family, blinders, log_n, fill, npub, bases):
    """All-zero and all-(r - 1) values, the identity permutation, one cycle through all 3 n slots, gates without selectors, with random, zero and r - 1
    blinders.  Zero values with zero blinders make l, r, o the zero polynomial (MSMs whose scalars are all zero, the point at infinity in the proof);
    with the identity permutation the quotient is zero too.  Those proofs are made over an SRS of real powers and also go through the oracle's
    verifier, the host verifier and the device batch verifier."""
    n = 1 << log_n
    degenerate = family in ps.DEGENERATE and blinders == "zeros"
    spr, sol = ps.circuit(family, n, npub, fill, 0x57 + log_n)
    alpha = 0xA1FA0123456789
    if degenerate:
        rb, pts, g2 = _device_srs(n + 3, alpha)
    else:
        pts = bases[:n + 3]
        rb = zb.ResidentBases(pts)
    pk = zp.setup(_circuit(spr), rb)
    ck, want_vk = _oracle_key(spr, pts)
    assert _vk_hex(pk.vk) == want_vk
    if "identity_perm" in family:
        assert list(ck.perm()) == ps.expected_identity_perm(n, npub, ps.rows_of(n, fill))
    bl = M(ps.blinders(blinders, log_n))
    proof = zp.prove(pk, M(sol), bl)
    assert proof == ck.prove(M(sol), bl)
    if degenerate:
        inf = bytes([0x40]) + bytes(31)
        identity = family == "zeros+identity_perm"
        for k in range(7):
            assert (proof[32 * k:32 * k + 32] == inf) == (k < 3 or (identity and k > 3)), k
        assert (proof[484:516] == inf) == identity
        pr = ps.decode_proof(proof, ref_g1_decompress)
        P = pl.g1_from_np
        vkd = pk.vk
        vk = dict(size=n, size_inv=ref.inv(n, R), generator=pl.mont_np_to_ints(vkd["generator"])[0], n_public=npub, coset_shift=5,
                  srs_g2=[ref.G2_GEN, ref.g2_mul(ref.G2_GEN, alpha)], s=[P(p) for p in vkd["s"]], ql=P(vkd["ql"]), qr=P(vkd["qr"]), qm=P(vkd["qm"]), qo=P(vkd["qo"]), qk=P(vkd["qk"]))
        assert pl.plonk_verify(vk, pr, sol[:npub])
        vk_wire = pk.write()[:368]
        pub = M(sol[:npub]) if npub else np.zeros((0, 4), np.uint64)
        tampered = proof[:547] + bytes([proof[547] ^ 1])       # zu
        host = [zv.plonk_verify(p, vk_wire, g2, pub) for p in (proof, tampered)]
        assert host == [True, False]
        assert list(zv.plonk_verify_batch([proof, tampered], vk_wire, g2, np.stack([pub, pub]))) == host
        assert list(zv.plonk_verify_batch([proof], vk_wire, g2, pub[None])) == host[:1]
    ck.free()
    pk.free()
    rb.free()


@pytest.mark.parametrize("log_n", [6, 11, 14])
@pytest.mark.parametrize("where", ps.VIOLATIONS)
def test_violations_are_reported(where, log_n, bases):
    """One value changed that only the last gate (row n - 1), only the first gate, or a gate naming a public input sees: the quotient's tail
    (n - 6 coefficients: one workgroup at 2^6, 8 and 64 above) is not zero and the prover says so; the oracle refuses the same witness; the next proof
    against the same key is the oracle's, so key and workspace survive the error."""
    n = 1 << log_n
    spr, sol, var = ps.violation_circuit(n, 3, 0xBAD0 + log_n)
    pts = bases[:n + 3]
    rb = zb.ResidentBases(pts)
    pk = zp.setup(_circuit(spr), rb)
    ck, want_vk = _oracle_key(spr, pts)
    assert _vk_hex(pk.vk) == want_vk
    bl = M(ps.blinders("random", log_n))
    bad = list(sol)
    bad[var[where]] = (bad[var[where]] + 1) % R
    assert not spr.is_satisfied(bad)
    with pytest.raises(AssertionError, match="not satisfied"):
        ck.prove(M(bad), bl)
    with pytest.raises(_lib.ZkmiError, match="does not satisfy"):
        zp.prove(pk, M(bad), bl)
    assert zp.prove(pk, M(sol), bl) == ck.prove(M(sol), bl)
    ck.free()
    pk.free()
    rb.free()
