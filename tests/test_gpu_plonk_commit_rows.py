"""The digests PLONK's rounds end in, for many witnesses per call (zk_bn254_plonk_commit_batch_dev / ProvingKey.commit_rows), against the bytes of the device
prover's own proof for the same witness, blinders and pinned challenges: L, R, O (Proof.WriteTo bytes 0 .. 96) from the blinded coefficients and from the wire
values + blinders against the Lagrange form, Z (96 .. 128) from ratio_batch's values blinded as the prover blinds them, H[0..2] (128 .. 224) from the thirds of
quotient_batch's h.  Circuits, solutions and the oracle's rounds 1 and 2 are those of tests/plonk_quotient_ref.py; three witnesses per key at 2^2, 2^6, 2^10."""
import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import bn254 as zb
from noir_backend_using_gnark_amd import plonk as zp
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import plonk_quotient_ref as qr

pytestmark = pytest.mark.gpu
R = ref.R
M = pl.ints_to_mont_np
WITNESSES = 3


def _circuit(spr) -> zp.Circuit:
    g = spr.constraints
    col = lambda k: M([c[k] for c in g])  # noqa: E731
    return zp.Circuit(spr.n_public, spr.n_vars, col(0), col(1), col(2), col(3), col(4), [c[5] for c in g], [c[6] for c in g], [c[7] for c in g])


@pytest.fixture(scope="module", params=[2, 6, 10], ids=lambda v: "2^%d" % v)
def case(request):
    """one key with its Lagrange form, three witnesses with their blinders and pinned challenges, the device prover's proof of each, and the oracle's blinded
    polynomials of rounds 1 and 2 for the same inputs"""
    _lib.require_device()
    log_n = request.param
    n = 1 << log_n
    spr, n_in = qr.forward_circuit(n, 1, 0x5E0 + log_n)
    opk = qr.setup_polys(spr, fast=True)
    # an SRS this small gets no window table by default: the smallest key commits row after row (the fallback), the others through the batched path
    rb = zb.ResidentBases(orc.g1_gen_points(0xA70 + n, n + 3), table_window_bits=-1 if log_n == 2 else 8)
    assert zb.msm_rows_info(rb, n + 2)["batched"] == (log_n != 2)
    pk = zp.setup(_circuit(spr), rb)
    pk.lagrange_srs()
    g = ref.SplitMix64(0xC0FFEE + log_n)
    rows = []
    for v in range(WITNESSES):
        sol = qr.solve(spr, [g.felt() for _ in range(n_in)])
        blinders, pin = [g.felt() for _ in range(9)], [g.felt() for _ in range(5)]  # gamma, beta, alpha, zeta, kzg gamma
        proof = zp.prove(pk, M(sol), M(blinders), challenges=M(pin))
        bl, br, bo, bz = qr.rounds_1_2(opk, sol, blinders, pin[1], pin[0], fast=True)
        rows.append(dict(sol=sol, blinders=blinders, pin=pin, proof=proof, bl=bl, br=br, bo=bo, bz=bz, lro=pl.evaluate_lro(spr, n, sol)))
    yield dict(n=n, spr=spr, opk=opk, pk=pk, rb=rb, rows=rows)
    pk.free()
    rb.free()


def _stack(case, key):
    return np.ascontiguousarray(np.stack([M(r[key]) for r in case["rows"]]))


def test_blinded_coefficients_commit_to_the_provers_l_r_o(case):
    pk = case["pk"]
    for k, key in enumerate(("bl", "br", "bo")):
        enc = pk.commit_rows(_stack(case, key), compressed=True, points=False)
        pts, enc2 = pk.commit_rows(_stack(case, key), compressed=True)
        for v, r in enumerate(case["rows"]):
            assert enc[v].tobytes() == r["proof"][32 * k:32 * k + 32], (key, v)
            assert orc.g1_compress(pts[v]) == enc[v].tobytes() == enc2[v].tobytes()


def test_wire_values_and_blinders_commit_to_the_same_bytes(case):
    """from_values: a row is the n wire values followed by b0, b1, against the Lagrange form -- on the host form and on device rows with a stride and poison"""
    pk, n = case["pk"], case["n"]
    for k in range(3):
        m = np.ascontiguousarray(np.stack([M(list(r["lro"][k]) + list(r["blinders"][2 * k:2 * k + 2])) for r in case["rows"]]))
        enc = pk.commit_rows(m, from_values=True, compressed=True, points=False)
        wide = np.full((WITNESSES, n + 5, 4), 0xFFFFFFFFFFFFFFFF, np.uint64)
        wide[:, :n + 2] = m
        d = _lib.DeviceBuffer.from_numpy(wide)
        out, denc = pk.commit_rows(d, from_values=True, length=n + 2, rows=WITNESSES, row_stride=n + 5, compressed=True)
        dev_enc, dev_pts = denc.to_numpy(np.uint8, (WITNESSES, 32)), out.to_numpy(np.uint64, (WITNESSES, 8))
        for b in (d, out, denc):
            b.free()
        for v, r in enumerate(case["rows"]):
            assert enc[v].tobytes() == r["proof"][32 * k:32 * k + 32], (k, v)
            assert dev_enc[v].tobytes() == enc[v].tobytes() and orc.g1_compress(dev_pts[v]) == enc[v].tobytes()


def test_thirds_of_h_and_blinded_z_commit_to_the_provers_digests(case):
    pk, n, opk = case["pk"], case["n"], case["opk"]
    rows = case["rows"]
    col = lambda k: M([r["pin"][k] for r in rows])  # noqa: E731
    # round 2 on the device: Z's values; blinded as the prover blinds it (three scalars), in canonical form
    vals = [np.ascontiguousarray(np.stack([M(r["lro"][k]) for r in rows])) for k in range(3)]
    z = pk.ratio_batch(vals[0], vals[1], vals[2], col(1), col(0))
    be = pl._Backend(True)
    bz = [pl._blind(pl._canonical(be, opk["d0"], pl.mont_np_to_ints(z[v])), n, r["blinders"][6:9]) for v, r in enumerate(rows)]
    assert [list(b) for b in bz] == [list(r["bz"]) for r in rows]
    zenc = pk.commit_rows(np.ascontiguousarray(np.stack([M(b) for b in bz])), compressed=True, points=False)
    # round 3 on the device: h; its thirds are rows of n + 2 coefficients, 3 per witness, contiguous in the output
    pub = np.ascontiguousarray(np.stack([M(r["sol"][:1]) for r in rows]))
    h, status = pk.quotient_batch(_stack(case, "bl"), _stack(case, "br"), _stack(case, "bo"), _stack(case, "bz"), pub, col(2), col(1), col(0))
    assert status.tolist() == [0] * WITNESSES
    henc = pk.commit_rows(np.ascontiguousarray(h.reshape(3 * WITNESSES, n + 2, 4)), compressed=True, points=False)
    for v, r in enumerate(rows):
        assert zenc[v].tobytes() == r["proof"][96:128], v
        assert henc[3 * v:3 * v + 3].tobytes() == r["proof"][128:224], v


def test_values_need_the_lagrange_form(case):
    spr, n = case["spr"], case["n"]
    pk = zp.setup(_circuit(spr), case["rb"])
    try:
        with pytest.raises(_lib.ZkmiError, match="Lagrange") as ei:
            pk.commit_rows(np.zeros((2, n + 2, 4), np.uint64), from_values=True)
        assert ei.value.code == _lib.ZK_ERR_ARG
        with pytest.raises(ValueError, match=r"len\(points\) != len\(scalars\)"):
            pk.commit_rows(np.zeros((2, n + 4, 4), np.uint64))  # longer than the SRS
    finally:
        pk.free()
