"""KZG openings on the device against the oracle (oracle/plonk_ref.py: poly_eval, divide_by_x_minus_a, kzg_derive_gamma; oracle/oracle.py: g1_msm for the
commitment), bit for bit: SRS.open / open_many / batch_open_single_point; the golden PLONK proofs' BatchedProof and ZShiftedOpening rebuilt through them;
kzg.batch_verify_multi_points (zk_bn254_kzg_verify_batch) against the host zk_bn254_kzg_verify, which tests/test_kzg_cpu.py pins to the oracle, and against
openings forged under a known SRS secret (tests/plonk_forge.py): edge values and points, points at infinity, errors that cancel under equal coefficients."""
import json
import os
import random

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests.helpers import from_mont_limbs, h2i

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
R = ref.R
M = pl.ints_to_mont_np
ALPHA = 0x2b7e151628aed2a6abf7158809cf4f3c762e7160f38b4da56a784d9045190cfe % R
SIZE = (1 << 16) + 8  # the SRS's full size: one of the lengths
LENGTHS = (1, 2, 255, 256, 257, (1 << 11) + 3, 1 << 16, SIZE)
BOUNDARY = (8, 9, 2047, 2048, 2049, 2050)  # the scan's lane boundary and workgroup boundary at K = 8 (csrc/scan.hpp scan_plan)


def g1_img(P):
    return np.frombuffer(ref.g1_affine_mont_bytes(P), dtype=np.uint64).copy()


def g2_img(P):
    return np.frombuffer(ref.g2_affine_mont_bytes(P), dtype=np.uint64)


@pytest.fixture(scope="module")
def env():
    o = pl.kzg_new_srs(SIZE, ALPHA, fast=True)
    with_table = kzg.new_srs(SIZE, M([ALPHA])[0])                          # >= 4096 bases: window tables
    without = kzg.new_srs(SIZE, M([ALPHA])[0], table_window_bits=-1)
    yield dict(g1=np.ascontiguousarray(o["g1"]), srs=(with_table, without))
    with_table.free()
    without.free()


def commit(env, p):
    if not p:
        return np.zeros(8, np.uint64)
    return orc.g1_msm(env["g1"][:len(p)], M(p))


def want_open(env, p, z):
    v = pl.poly_eval(p, z)
    return commit(env, pl.divide_by_x_minus_a(p, v, z)), v


def rand_poly(rng, n):
    return [rng.randrange(R) for _ in range(n)]


def poly_with_root(rng, n, root):
    q = rand_poly(rng, n - 1)
    p = [0] * n
    for i, c in enumerate(q):
        p[i] = (p[i] - root * c) % R
        p[i + 1] = (p[i + 1] + c) % R
    return p


def case(rng, n, kind):
    """a polynomial of n coefficients and a point: 0, 1, a root of the polynomial, random"""
    if kind == 2 and n >= 2:
        z = rng.randrange(R)
        return poly_with_root(rng, n, z), z
    return rand_poly(rng, n), (0, 1, rng.randrange(R), rng.randrange(R))[kind]


def check_many(env, srs, cases, on_device):
    polys = [M(p) for p, _ in cases]
    bufs = [_lib.DeviceBuffer.from_numpy(a) for a in polys] if on_device else None
    h, v = srs.open_many(bufs if on_device else polys, M([z for _, z in cases]), [len(p) for p, _ in cases] if on_device else None)
    for k, (p, z) in enumerate(cases):
        wh, wv = want_open(env, p, z)
        assert from_mont_limbs(v[k]) == [wv], (k, len(p))
        assert h[k].tobytes() == wh.tobytes(), (k, len(p))
        if len(p) == 1:
            assert not h[k].any()  # an empty quotient: H = infinity
    if on_device:  # the caller's buffers are not written
        for b, a in zip(bufs, polys):
            assert b.to_numpy(np.uint64, a.shape).tobytes() == a.tobytes()
            b.free()


def test_open_every_length(env):
    rng = random.Random(21)
    for i, n in enumerate(LENGTHS):
        p, z = case(rng, n, i % 4)
        srs = env["srs"][i % 2]
        h, v = srs.open(M(p), M([z])[0])
        wh, wv = want_open(env, p, z)
        assert from_mont_limbs(v) == [wv] and h.tobytes() == wh.tobytes(), n
        if n in (257, SIZE):  # the same from a DeviceBuffer, on the other SRS
            b = _lib.DeviceBuffer.from_numpy(M(p))
            h2, v2 = env["srs"][1 - i % 2].open(b, M([z])[0], n)
            b.free()
            assert h2.tobytes() == wh.tobytes() and v2.tobytes() == v.tobytes()


@pytest.mark.parametrize("count", [1, 2, 3, 7, 8, 9, 20])
def test_open_many_unequal_rows(env, count):
    rng = random.Random(100 + count)
    small = (1, 2, 255, 256, 257, (1 << 11) + 3, 33, 1000)
    lens = [small[(k * 3 + count) % len(small)] for k in range(count)]
    lens[count // 2] = 1 << 16 if count in (3, 9) else (SIZE if count == 20 else lens[count // 2])
    cases = [case(rng, n, (k + count) % 4) for k, n in enumerate(lens)]
    for t, srs in enumerate(env["srs"]):
        check_many(env, srs, cases, on_device=(t + count) % 2 == 1)


def test_open_at_lane_and_workgroup_boundaries(env):
    """K = 8 coefficients per lane, 2048 per workgroup: a row that ends with a lane, with a workgroup, one coefficient either side -- alone, and in one call next to
    a long row, whose workgroups above the short rows' ends contribute nothing"""
    rng = random.Random(24)
    cases = [case(rng, n, k % 4) for k, n in enumerate(BOUNDARY)]
    for k, (p, z) in enumerate(cases):
        h, v = env["srs"][k % 2].open(M(p), M([z])[0])
        wh, wv = want_open(env, p, z)
        assert from_mont_limbs(v) == [wv] and h.tobytes() == wh.tobytes(), len(p)
    cases.insert(3, case(rng, 1 << 16, 3))  # between 2047 and 2048
    for t, srs in enumerate(env["srs"]):
        check_many(env, srs, cases, on_device=t == 1)


def test_open_many_same_polynomial_or_same_point(env):
    rng = random.Random(23)
    p, q = rand_poly(rng, 300), rand_poly(rng, 257)
    z1, z2 = rng.randrange(R), rng.randrange(R)
    for srs in env["srs"]:
        check_many(env, srs, [(p, z1), (p, z2)], on_device=False)
        check_many(env, srs, [(p, z1), (q, z1)], on_device=True)
        check_many(env, srs, [(p, z1), (p, z1), (p, z1)], on_device=False)


def check_batch(env, polys, z, flip):
    """batch_open_single_point of polys at z on both SRS forms, from host arrays on one and from DeviceBuffers on the other, against the oracle's fold and division"""
    lens = [len(p) for p in polys]
    digests = np.stack([commit(env, p) for p in polys])
    claimed = [pl.poly_eval(p, z) for p in polys]
    kg = pl.kzg_derive_gamma(z, [pl.g1_from_np(d) for d in digests], claimed)
    folded, fe, acc = [0] * max(lens), 0, 1
    for p, v in zip(polys, claimed):
        for j, c in enumerate(p):
            folded[j] = (folded[j] + c * acc) % R
        fe = (fe + v * acc) % R
        acc = acc * kg % R
    want_h = commit(env, pl.divide_by_x_minus_a(folded, fe, z))
    for t, srs in enumerate(env["srs"]):
        arrs = [M(p) for p in polys]
        on_device = (t + flip) % 2 == 1
        bufs = [_lib.DeviceBuffer.from_numpy(a) for a in arrs] if on_device else None
        h, v = srs.batch_open_single_point(bufs if on_device else arrs, digests, M([z])[0], lens if on_device else None)
        assert from_mont_limbs(v) == claimed
        assert h.tobytes() == want_h.tobytes()
        for b in bufs or []:
            b.free()


@pytest.mark.parametrize("count", [1, 2, 3, 7, 8, 9, 20])
def test_batch_open_single_point(env, count):
    rng = random.Random(200 + count)
    small = (1, 2, 255, 256, 257, (1 << 11) + 3, 33, 1000)
    lens = [small[(k * 5 + count) % len(small)] for k in range(count)]
    if count in (7, 20):
        lens[1] = 1 << 16 if count == 7 else SIZE
    polys = [rand_poly(rng, n) for n in lens]
    z = (rng.randrange(R), 0, 1, rng.randrange(R), rng.randrange(R), rng.randrange(R))[count % 6]
    if count == 8:
        polys[3] = poly_with_root(rng, len(polys[3]), z)
    check_batch(env, polys, z, count)


@pytest.mark.parametrize("root_of", [None, 3])
def test_batch_open_single_point_at_lane_and_workgroup_boundaries(env, root_of):
    """the evaluation scan over rows that end at a lane's last coefficient and at a workgroup's (K = 8: 2048 is one workgroup exactly), then the division of their
    fold; the point a root of the 2048-coefficient row, or random.  The first m rows alone make the divided fold end at each of the boundaries in turn."""
    rng = random.Random(300 + (root_of or 0))
    z = rng.randrange(R)
    polys = [poly_with_root(rng, n, z) if k == root_of else rand_poly(rng, n) for k, n in enumerate(BOUNDARY)]
    if root_of is not None:
        assert BOUNDARY[root_of] == 2048 and pl.poly_eval(polys[root_of], z) == 0
        check_batch(env, polys, z, 1)
        return
    for m in range(1, len(polys) + 1):
        check_batch(env, polys[:m], z, m)


def test_constant_polynomials_and_length_errors(env):
    srs = env["srs"][0]
    h, v = srs.batch_open_single_point([M([5]), M([7])], np.stack([commit(env, [5]), commit(env, [7])]), M([9])[0])
    assert not h.any() and from_mont_limbs(v) == [5, 7]
    too_long = np.zeros((SIZE + 1, 4), np.uint64)
    for call in (lambda: srs.open(too_long, M([3])[0]), lambda: srs.open_many([M([1, 2]), too_long], M([3, 4])),
                 lambda: srs.batch_open_single_point([too_long], np.zeros((1, 8), np.uint64), M([3])[0])):
        with pytest.raises(ValueError, match="kzg: invalid polynomial size"):
            call()
    assert srs.open(np.zeros((SIZE, 4), np.uint64), M([3])[0])[1].tobytes() == bytes(32)  # the full size is allowed
    with pytest.raises(_lib.ZkmiError) as ei:
        kzg.SRS(type("H", (), {"handle": _lib.C.c_uint64(0x00ffffffffffff)})(), None).open(M([1, 2]), M([3])[0])
    assert ei.value.code == _lib.ZK_ERR_HANDLE


def test_plonk_last_round_through_the_kzg_entries():
    with open(os.path.join(HERE, "golden", "plonk_golden.json")) as f:
        golden = json.load(f)
    for e in golden:
        spr, sol = pl.sparse_r1cs_from_acir(e["acir"], [h2i(v) for v in e["values"]])
        opk, ovk = pl.plonk_setup(spr, pl.kzg_new_srs(e["srs_size"], h2i(e["srs_alpha"])))
        t = {}
        proof = pl.plonk_prove(opk, sol, [h2i(v) for v in e["blinders"]], trace=t)
        n, zeta = opk["n"], t["zeta"]
        zp = pow(zeta, n + 2, R)
        h1, h2, h3 = t["h"][:n + 2], t["h"][n + 2:2 * (n + 2)], t["h"][2 * (n + 2):3 * (n + 2)]
        folded_h = [((h3[i] * zp + h2[i]) % R * zp + h1[i]) % R for i in range(n + 2)]
        polys = [folded_h, t["lin"], t["bl"], t["br"], t["bo"], opk["s1"], opk["s2"]]
        digests = [t["folded_h_digest"], t["lin_digest"], *proof["lro"], ovk["s"][0], ovk["s"][1]]
        want = bytes.fromhex(e["proof"])
        srs = kzg.new_srs(e["srs_size"], M([h2i(e["srs_alpha"])])[0])
        try:
            h, claimed = srs.batch_open_single_point([M(p) for p in polys], np.stack([g1_img(d) for d in digests]), M([zeta])[0])
            got = ref.g1_compress(pl.g1_from_np(h)) + (7).to_bytes(4, "big") + b"".join(pl.fr_bytes(v) for v in from_mont_limbs(claimed))
            assert got == want[224:484]
            zh, zu = srs.open(M(t["bz"]), M([zeta * opk["d0"].gen % R])[0])
            assert ref.g1_compress(pl.g1_from_np(zh)) + pl.fr_bytes(from_mont_limbs(zu)[0]) == want[484:548]
        finally:
            srs.free()


# ---- zk_bn254_kzg_verify_batch
def _pool():
    """true openings over mixed polynomials and points (a 64-point SRS), among them a constant (H = infinity) and the zero polynomial (C = H = infinity)"""
    rng = random.Random(31)
    srs = pl.kzg_new_srs(64, ALPHA, fast=True)
    g1 = np.ascontiguousarray(srs["g1"])
    cm = lambda p: orc.g1_msm(g1[:len(p)], M(p)) if p else np.zeros(8, np.uint64)
    cases = [case(rng, n, k % 4) for k, n in enumerate((2, 3, 7, 33, 64, 64, 17, 40, 5, 64, 2, 9))] + [([11], 5), ([0], 6)]
    D, H, V, Z = [], [], [], []
    for p, z in cases:
        v = pl.poly_eval(p, z)
        D.append(cm(p))
        H.append(cm(pl.divide_by_x_minus_a(p, v, z)))
        V.append(v)
        Z.append(z)
    g2 = np.stack([g2_img(srs["g2"][0]), g2_img(srs["g2"][1])])
    return np.stack(D), np.stack(H), M(V), M(Z), g2


def _run(D, H, V, Z, g2):
    _lib.profile(True)
    _lib.profile_reset()
    try:
        got = kzg.batch_verify_multi_points(D, H, V, Z, g2)
        prof = _lib.profile_read()
    finally:
        _lib.profile(False)
    return got, prof


def _tile(a, n):
    return np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))


def test_verify_batch_true_openings_pass_the_combined_check():
    D, H, V, Z, g2 = _pool()
    assert not H[-2].any() and not H[-1].any() and not D[-1].any()
    for i in range(len(D)):
        assert kzg.verify(D[i], H[i], V[i], Z[i], g2), i
    for n in (1, 2, 3, 1000, (1 << 16) + 5):
        got, prof = _run(_tile(D, n), _tile(H, n), _tile(V, n), _tile(Z, n), g2)
        assert got.shape == (n,) and got.all(), n
        chunks = (n + (1 << 16) - 1) >> 16
        # the combined check alone: one kzg_combine, one two-lane Miller loop and one final exponentiation per chunk -- the fallback would add a Miller launch
        assert prof["kzg_combine"][0] == chunks and prof["miller_loop"][0] == chunks and prof["fe_easy"][0] == chunks, prof


def test_verify_batch_bad_openings_get_the_host_verdicts():
    D, H, V, Z, g2 = _pool()
    n = (1 << 16) + 5
    D, H, V, Z = _tile(D, n), _tile(H, n), _tile(V, n), _tile(Z, n)
    G = g1_img(ref.G1_GEN)
    one = M([1])[0]
    e = 12345
    touched = [0, 10, 11, 20, 21, (1 << 16) - 1, 1 << 16, n - 1]
    V[0] = M([(from_mont_limbs(V[0])[0] + 1) % R])[0]                       # first: another claimed value
    V[11] = V[10]
    D[11], H[11], Z[11] = D[10], H[10], Z[10]
    v10 = from_mont_limbs(V[10])[0]
    V[10], V[11] = M([(v10 + e) % R])[0], M([(v10 - e) % R])[0]              # two copies of one opening, off by +e and -e
    H[20] = 0                                                                # H = infinity where it is not
    D[21] = 0                                                                # C = infinity where it is not
    D[(1 << 16) - 1] = G                                                     # chunk boundary, last of the first chunk: another digest
    Z[1 << 16] = one                                                         # first of the second chunk: another point
    H[n - 1] = G                                                             # last: another H
    want = np.ones(n, np.uint8)
    for i in touched:
        want[i] = kzg.verify(D[i], H[i], V[i], Z[i], g2)
    assert not want[touched].any()
    got, prof = _run(D, H, V, Z, g2)
    assert (got == want).all(), np.nonzero(got != want)
    assert prof["miller_loop"][0] == 4  # both chunks fell back: a two-lane and a 2 n-lane launch each
    # small batches: a single bad opening, and the two off-by-e copies alone
    for idx in ([0], [10, 11], [20, 21, 0]):
        got, _ = _run(D[idx], H[idx], V[idx], Z[idx], g2)
        assert not got.any()
    idx = [1, 2, 10, 3]
    got, _ = _run(D[idx], H[idx], V[idx], Z[idx], g2)
    assert got.tolist() == [1, 1, 0, 1]


# ---- zk_bn254_kzg_verify_batch against openings forged under a known tau (tests/plonk_forge.py; tests/test_plonk_forge_cpu.py holds them against the host)
def _forged(lanes):
    from tests import plonk_forge as pf
    D, H, V, Z, want, g2 = pf.kzg_arrays(lanes)
    got, prof = _run(D, H, V, Z, g2)
    wrong = ["lane %d of %d: %s: got %d, expected %d" % (i, len(lanes), l.label, got[i], l.expect) for i, l in enumerate(lanes) if got[i] != l.expect]
    assert not wrong, wrong[:12]
    # the combined check decided exactly when nothing is to be rejected: the fallback adds a Miller launch
    assert prof["kzg_combine"][0] == 1 and prof["miller_loop"][0] == (1 if want.all() else 2), prof
    return got


def test_verify_batch_forged_accepts_at_the_edges():
    """v and z among 0, 1, 2^192 - 1, 2^224, r - 1 and random; C, H and C - v G + z H at infinity; z = tau with c = v and any H"""
    from tests import plonk_forge as pf
    lanes = pf.kzg_accepts()
    assert len(lanes) >= 31
    assert _forged(lanes).all()
    for l in lanes:
        _forged([l])
    for n in (2, 65):
        for start in (0, 5, 24):
            _forged([lanes[(start + j) % len(lanes)] for j in range(n)])


def test_verify_batch_forged_rejects_and_cancelling_pairs():
    """H off by a known multiple of G; two lanes whose errors cancel when lambda_1 == lambda_2: alone, 1 and 64 lanes apart, and in the middle of 1000 lanes"""
    from tests import plonk_forge as pf
    good, bad, pairs = pf.kzg_accepts(), pf.kzg_rejects(), pf.kzg_cancelling_pairs()
    for l in bad:
        _forged([l])
        _forged([good[3], l])
    for a, b in pairs:
        _forged([a, b])
        _forged([b, a])
        fill = [good[j % len(good)] for j in range(65)]
        for at_a, at_b in ((10, 11), (0, 64), (64, 0)):
            lanes = list(fill)
            lanes[at_a], lanes[at_b] = a, b
            _forged(lanes)
    lanes = [good[j % len(good)] for j in range(1000)]
    assert _forged(lanes).all()
    lanes[500:500 + len(bad)] = bad
    (lanes[498], lanes[499]), (lanes[436], lanes[600]), (lanes[0], lanes[999]) = pairs
    got = _forged(lanes)
    assert got.sum() == 1000 - len(bad) - 6
