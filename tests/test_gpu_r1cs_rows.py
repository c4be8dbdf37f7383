"""GPU suite (-m gpu): the row-batched R1CS step (r1cs.hip k_spmv3_rows behind zk_bn254_r1cs_eval_abc_rows_dev) and the step / offset glue of
zk_bn254_groth16_prove_r1cs_batch around it, everything exact.

The stage: a, b, c = L w, R w, O w of every row of one launch against the big-integer model tests/groth16_setup_ref.System.eval_abc (pinned without a GPU by
tests/test_groth16_setup_ref_cpu.py) element by element, and against zk_bn254_r1cs_eval_abc_dev of each row alone -- n_constraints either side of the 256-lane
workgroup, n_wires != n_constraints so that a stride mix-up cannot cancel, rows that differ, poisoned outputs with guard elements behind them, the input image
compared before and after, and the 65535-row limit of the launch.

The edge shapes of the matrices are spread over two of the five systems because no single system can hold them all: the 600-constraint system has empty rows in
each of L, R and O (the first and the last constraint included), a row that names one wire twice, coefficients 0 and r - 1, one row of 1500 entries (above
SPMV_LONG = 1024: the rows form has no long-row list, one lane walks it) and one of exactly 1024; its R names the ONE wire in every row that is not empty.  The
other four systems name the ONE wire in EVERY row of R.

The glue: zk.prove_r1cs_batch byte for byte against zk.prove_r1cs of each row (keys from zk.setup with pinned toxic waste), the first and the last row of each
call also against the oracle's proof over the model's a, b, c with the reference Setup's key; n_constraints < N and == N, more than one step ending in a step of
one row, device pointers (only read; the 1025-row call covers the first * n_wires offset), a key the batched path does not serve, and n_proofs = 1."""
import time

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import groth16 as g16
from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import groth16_setup_ref as gs
from tests.helpers import sha_image

pytestmark = pytest.mark.gpu
R = ref.R
_RINV = pow(ref.MONT_R, -1, R)
POISON = np.uint64(0xA5A5A5A5A5A5A5A5)  # as a limb image it is above the modulus: no reduced element the kernel writes can equal it
GUARD = 64
MAX_ROWS = 64
N_WIRES = {1: 5, 255: 77, 256: 131, 257: 300, 600: 1700}  # never n_constraints
MATRIX = "LRO"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback
    yield
    for k in _KEYS.values():
        k["pk"].free()
    for c in list(_CASES.values()) + list(_SMALL.values()):
        c["dev"].free()
    _KEYS.clear(), _CASES.clear(), _SMALL.clear(), _SINGLES.clear(), _ORACLE.clear()


def _ints(limbs) -> list:
    """Montgomery limbs -> canonical ints"""
    raw = np.ascontiguousarray(limbs, np.uint64).tobytes()
    return [int.from_bytes(raw[o:o + 32], "little") * _RINV % R for o in range(0, len(raw), 32)]


def _sparse(rng, sizes, n_wires, n_coef, one_in_every_row=False):
    sizes = np.asarray(sizes)
    rows = np.repeat(np.arange(sizes.size), sizes)
    wires = rng.integers(0, n_wires, size=rows.size)
    if one_in_every_row:
        first = np.concatenate([[0], np.cumsum(sizes)[:-1]])[sizes > 0]
        wires[first] = 0
    return rows, wires, rng.integers(0, n_coef, size=rows.size)


def plain_system(nc: int, nw: int) -> gs.System:
    """1 to 3 entries per row of L and O, the ONE wire and up to 2 more in every row of R, coefficients 0, 1 and r - 1 among random ones"""
    rng = np.random.default_rng(0xA0 + nc)
    coef = [0, 1, R - 1] + ref.rand_felts(0xA0 + nc, 13)
    return gs.System(nc, nw, min(nw, 3), coef, [_sparse(rng, rng.integers(1, 4, size=nc), nw, len(coef)),
                                               _sparse(rng, rng.integers(1, 4, size=nc), nw, len(coef), one_in_every_row=True),
                                               _sparse(rng, rng.integers(1, 4, size=nc), nw, len(coef))])


def edge_system() -> gs.System:
    """600 constraints over 1700 wires: see the module's docstring"""
    rng = np.random.default_rng(0xED)
    nc, nw = 600, N_WIRES[600]
    coef = [0, 1, R - 1] + ref.rand_felts(0xED, 13)
    sz = [rng.integers(1, 4, size=nc) for _ in range(3)]
    for m, extra in enumerate((300, 1, 2)):
        sz[m][[0, nc - 1, extra]] = 0          # empty rows: the first and the last constraint of every matrix, and one inside
    sz[0][7], sz[0][8] = 1500, 1024            # one lane walks each of them
    sz[1][nc - 2] = 1025                       # and the last row of R that is not empty
    sparse = [list(_sparse(rng, sz[m], nw, len(coef), one_in_every_row=m == 1)) for m in range(3)]
    for m, j, wires, vids in ((0, 5, [7, 7, 9], [3, 4, 5]),      # row 5 of L names wire 7 twice, with two coefficients
                              (2, 9, [3, 4, 0], [0, 2, 2]),      # row 9 of O: coefficients 0 and r - 1, the latter on ONE too
                              (1, 1, [11, 0, 11], [2, 1, 2])):   # row 1 of R (empty so far): wire 11 twice with r - 1, and ONE
        sparse[m][0] = np.concatenate([sparse[m][0], [j] * len(wires)])
        sparse[m][1] = np.concatenate([sparse[m][1], wires])
        sparse[m][2] = np.concatenate([sparse[m][2], vids])
    sy = gs.System(nc, nw, 3, coef, [tuple(s) for s in sparse])
    cnt = [np.bincount(sy.sparse[m][0], minlength=nc) for m in range(3)]
    assert all(cnt[m][0] == 0 and cnt[m][nc - 1] == 0 for m in range(3)) and cnt[0][300] == 0 and cnt[2][2] == 0
    assert cnt[0][7] == 1500 and cnt[0][8] == 1024 and cnt[1][nc - 2] == 1025
    return sy


def witness_rows(n: int, nw: int, seed: int) -> np.ndarray:
    """rows cycle through uniform, witness-like, all zero and every wire r - 1"""
    top = gs.mont_limbs([R - 1])[0]
    out = np.zeros((n, nw, 4), np.uint64)
    for i in range(n):
        if i % 4 < 2:
            out[i] = orc.rand_fr(seed + i, nw, witness_like=bool(i % 4))
        elif i % 4 == 3:
            out[i] = top
    return out


_CASES, _SMALL, _KEYS, _SINGLES, _ORACLE = {}, {}, {}, {}, {}


def _model(sy: gs.System, W: np.ndarray):
    """the model's a, b, c of every row: ints [row][matrix][constraint] and limbs (3, rows, n_constraints, 4)"""
    ints = [sy.eval_abc(_ints(W[z])) for z in range(W.shape[0])]
    limbs = np.stack([np.stack([gs.mont_limbs(ints[z][m]).reshape(-1, 4) for z in range(W.shape[0])]) for m in range(3)])
    return ints, limbs


def _case(nc: int) -> dict:
    """one system per n_constraints, its MAX_ROWS witness rows and the model's a, b, c of them: computed once, shared, never changed"""
    if nc not in _CASES:
        sy = edge_system() if nc == 600 else plain_system(nc, N_WIRES[nc])
        assert sy.n_wires != sy.n_constraints
        W = witness_rows(MAX_ROWS, sy.n_wires, 0x5000 + nc)
        ints, limbs = _model(sy, W)
        W.setflags(write=False), limbs.setflags(write=False)
        _CASES[nc] = dict(name="c%d" % nc, sy=sy, dev=sy.load(nc), W=W, ints=ints, limbs=limbs, single={})
    return _CASES[nc]


def _single(c: dict, z: int):
    if z not in c["single"]:
        c["single"][z] = c["dev"].eval_abc(c["W"][z])
    return c["single"][z]


def _poisoned(n: int):
    return _lib.DeviceBuffer.from_numpy(np.full((n + GUARD, 4), POISON, np.uint64))


def _check_rows(got: np.ndarray, c: dict, m: int, what: str):
    """got (rows, n_constraints, 4) is the model's matrix m of the first rows of the case, element by element"""
    rows = got.shape[0]
    want = c["limbs"][m][:rows]
    bad = np.argwhere((got != want).any(axis=2))
    if bad.size:
        z, j = (int(v) for v in bad[0])
        pytest.fail("%s %s: matrix %s differs in %d of %d elements; first: row %d, constraint %d: expected %d, got %d (limb image %s)"
                    % (c["name"], what, MATRIX[m], bad.shape[0], rows * want.shape[1], z, j, c["ints"][z][m][j], _ints(got[z, j])[0], got[z, j].tolist()))


# ------------------------------------------------------------------------------------------------ the stage
@pytest.mark.parametrize("rows", [1, 2, 3, 64])
@pytest.mark.parametrize("nc", [1, 255, 256, 257, 600])
def test_every_element_of_every_row_is_the_models(nc, rows):
    c = _case(nc)
    dev, W = c["dev"], c["W"][:rows]
    n = rows * nc
    dw = _lib.DeviceBuffer.from_numpy(W)
    before = sha_image(dw.to_numpy(np.uint64, W.shape))
    assert before == sha_image(W)
    outs = [_poisoned(n) for _ in range(3)]
    got = dev.eval_abc_rows(dw, on_device=True, rows=rows, out=outs)
    full = [o.to_numpy(np.uint64, (n + GUARD, 4)) for o in outs]
    for m in range(3):
        assert got[m].shape == (rows, nc, 4)
        assert np.array_equal(full[m][:n].reshape(rows, nc, 4), got[m])
        left = np.flatnonzero((full[m][:n] == POISON).all(axis=1))
        assert left.size == 0, "%s: matrix %s: %d elements not written, first row %d constraint %d" % (c["name"], MATRIX[m], left.size, left[0] // nc, left[0] % nc)
        assert (full[m][n:] == POISON).all(), "%s: matrix %s: written past rows * n_constraints" % (c["name"], MATRIX[m])
        _check_rows(got[m], c, m, "%d rows" % rows)
    assert sha_image(dw.to_numpy(np.uint64, W.shape)) == before, "the input rows were written"
    for z in range(rows):  # each row against the single-vector kernel on that row alone
        one = _single(c, z)
        for m in range(3):
            bad = np.flatnonzero((got[m][z] != one[m]).any(axis=1))
            assert bad.size == 0, "%s: matrix %s row %d differs from eval_abc of the row alone at constraints %s; the model expects %d at the first" \
                % (c["name"], MATRIX[m], z, bad[:8].tolist(), c["ints"][z][m][int(bad[0])])
    host = dev.eval_abc_rows(W)  # host rows, staged by the binding
    for m in range(3):
        _check_rows(host[m], c, m, "%d host rows" % rows)


def test_wrong_width_is_a_length_error_and_nothing_is_written():
    c = _case(255)
    dev, nc = c["dev"], 255
    outs = [_poisoned(2 * nc) for _ in range(3)]
    with pytest.raises(ValueError, match="wires of the constraint system"):
        dev.eval_abc_rows(np.ascontiguousarray(c["W"][:2, :-1]), out=outs)
    for o in outs:
        assert (o.to_numpy(np.uint64, (2 * nc + GUARD, 4)) == POISON).all()


def _one_constraint_system() -> gs.System:
    coef = [1, R - 1] + ref.rand_felts(0x65, 3)
    return gs.System(1, 2, 1, coef, [([0, 0], [0, 1], [2, 3]), ([0], [1], [1]), ([0, 0], [1, 0], [4, 0])])


def test_the_vector_limit_of_one_launch():
    """65535 rows of a system of 1 constraint over 2 wires (4 MB of input) agree with the model; 65536 rows are ZK_ERR_ARG and nothing is written"""
    sy = _one_constraint_system()
    dev = sy.load()
    try:
        n = 65536
        W = np.ascontiguousarray(np.concatenate([orc.rand_fr(0x66, n), orc.rand_fr(0x67, n, witness_like=True)], axis=1).reshape(n, 2, 4))
        W[5], W[6] = 0, gs.mont_limbs([R - 1])[0]
        wi = _ints(W)
        cf = sy.coef
        want = [[(cf[2] * wi[2 * z] + cf[3] * wi[2 * z + 1]) % R for z in range(n)], [cf[1] * wi[2 * z + 1] % R for z in range(n)],
                [(cf[4] * wi[2 * z + 1] + cf[0] * wi[2 * z]) % R for z in range(n)]]
        for z in (0, 5, 6, 65534):  # the closed form above is the model's
            assert tuple(v[0] for v in sy.eval_abc(wi[2 * z:2 * z + 2])) == tuple(want[m][z] for m in range(3))
        dw = _lib.DeviceBuffer.from_numpy(W)
        before = sha_image(dw.to_numpy(np.uint64, W.shape))
        outs = [_poisoned(n) for _ in range(3)]
        with pytest.raises(_lib.ZkmiError, match="wire vectors in one launch") as ei:
            dev.eval_abc_rows(dw, on_device=True, rows=n, out=outs)
        assert ei.value.code == _lib.ZK_ERR_ARG
        for m in range(3):
            assert (outs[m].to_numpy(np.uint64, (n + GUARD, 4)) == POISON).all(), "matrix %s written by a refused call" % MATRIX[m]
        got = dev.eval_abc_rows(dw, on_device=True, rows=n - 1, out=outs)
        for m in range(3):
            exp = gs.mont_limbs(want[m][:n - 1])
            bad = np.flatnonzero((got[m].reshape(n - 1, 4) != exp).any(axis=1))
            assert bad.size == 0, "matrix %s differs in %d rows; first: row %d, constraint 0: expected %d, got %d" \
                % (MATRIX[m], bad.size, bad[0], want[m][int(bad[0])], _ints(got[m][int(bad[0]), 0])[0])
            assert (outs[m].to_numpy(np.uint64, (n + GUARD, 4))[n - 1:] == POISON).all(), "matrix %s: written past the last row" % MATRIX[m]
        assert sha_image(dw.to_numpy(np.uint64, W.shape)) == before
    finally:
        dev.free()


# ------------------------------------------------------------------------------------------------ prove_r1cs_batch
def _small_case() -> dict:
    """3 constraints (domain of 4) over the wires [ONE, out, x, y, u, v]: x y = u, u x = v, (x + 1)(y + 2) = out; 8 distinct satisfying witnesses"""
    if "c3" not in _SMALL:
        sy = gs.System(3, 6, 2, [1, 2], [([0, 1, 2, 2], [2, 4, 2, 0], [0, 0, 0, 0]), ([0, 1, 2, 2], [3, 2, 3, 0], [0, 0, 0, 1]), ([0, 1, 2], [4, 5, 1], [0, 0, 0])])
        xy = [(0, 5), (R - 1, R - 1)] + list(zip(ref.rand_felts(0x31, 6), ref.rand_felts(0x32, 6)))
        wit = [[1, (x + 1) * (y + 2) % R, x, y, x * y % R, x * y * x % R] for x, y in xy]
        for w in wit:
            a, b, c = sy.eval_abc(w)
            assert [x * y % R for x, y in zip(a, b)] == list(c)
        W = np.stack([gs.mont_limbs(w) for w in wit])
        ints, limbs = _model(sy, W)
        _SMALL["c3"] = dict(name="c3", sy=sy, dev=sy.load(3), W=W, ints=ints, limbs=limbs)
    return _SMALL["c3"]


def _prove_case(name: str) -> dict:
    if name == "c3":
        return _small_case()
    c = _case(int(name[1:]))
    if "pool" not in c:
        c["pool"] = [0, 1, 2, 3, 4, 5, 8]  # uniform, witness-like, zero, r - 1, uniform, witness-like, uniform: 7 distinct rows
        assert len({sha_image(c["W"][i]) for i in c["pool"]}) == 7
    return c


def _key(name: str, tables: bool = True) -> dict:
    """zk.setup of the case's system with pinned toxic waste (one key per case and kind, shared), and the reference Setup's key for the oracle"""
    if (name, tables) not in _KEYS:
        c = _prove_case(name)
        tox = ref.rand_felts(0x7000 + c["sy"].n_constraints, 5)
        pk, vk = zk.setup(c["dev"], gs.mont_limbs(tox), precompute_tables=tables)
        _KEYS[(name, tables)] = dict(pk=pk, vk=vk, tox=tox)
    return _KEYS[(name, tables)]


def _oracle_key(name: str) -> dict:
    if ("key", name) not in _ORACLE:
        _ORACLE[("key", name)] = gs.setup(_prove_case(name)["sy"], _key(name)["tox"])["key"]
    return _ORACLE[("key", name)]


def _call_rows(name: str, n: int):
    """the call's w rows (cycling through the case's distinct rows), which of the case's rows each is, and n distinct (r, s).  The cycle shifts by one every 1024
    rows: the row a second step starts with must not be the witness the call starts with, or a dropped offset would read the right values"""
    c = _prove_case(name)
    pool = np.asarray(c.get("pool", range(c["W"].shape[0])))
    pick = pool[(np.arange(n) + np.arange(n) // 1024) % pool.size]
    assert n <= 1024 or pick[1024] != pick[0]
    r, s = orc.rand_fr(0x8000 + n, n), orc.rand_fr(0x9000 + n, n)
    assert len({v.tobytes() for v in r}) == n and len({v.tobytes() for v in s}) == n
    return np.ascontiguousarray(c["W"][pick]), pick, r, s


def _singles(name: str, tables: bool, n: int, idx) -> dict:
    """zk.prove_r1cs of the named rows of the n-row call, each computed once"""
    c, k = _prove_case(name), _key(name, tables)
    W, _, r, s = _call_rows(name, n)
    memo = _SINGLES.setdefault((name, tables, n), {})
    for i in idx:
        if i not in memo:
            memo[i] = zk.prove_r1cs(c["dev"], k["pk"], W[i], r[i], s[i])
    return memo


def _oracle_proof(name: str, n: int, i: int) -> bytes:
    if (name, n, i) not in _ORACLE:
        c = _prove_case(name)
        W, pick, r, s = _call_rows(name, n)
        abc = [np.ascontiguousarray(c["limbs"][m][pick[i]]) for m in range(3)]
        _ORACLE[(name, n, i)] = bytes(orc.groth16_prove(_oracle_key(name), *abc, W[i], r[i], s[i])[0])
    return _ORACLE[(name, n, i)]


def _check_call(name: str, n: int, on_device: bool, tables: bool = True, idx=None):
    c, k = _prove_case(name), _key(name, tables)
    W, _, r, s = _call_rows(name, n)
    if on_device:
        buf = _lib.DeviceBuffer.from_numpy(W)
        before = sha_image(buf.to_numpy(np.uint64, W.shape))
        assert before == sha_image(W)
        got = g16.prove_r1cs_batch(c["dev"], k["pk"], buf, r, s, on_device=True)
        assert sha_image(buf.to_numpy(np.uint64, W.shape)) == before, "the device rows were written"
    else:
        got = g16.prove_r1cs_batch(c["dev"], k["pk"], W, r, s)
    assert len(got) == n
    idx = list(range(n)) if idx is None else idx
    want = _singles(name, tables, n, idx)
    bad = [i for i in idx if got[i] != want[i]]
    assert not bad, "%s, %d rows, on_device=%s: rows %s%s are not the single prover's" % (name, n, on_device, bad[:16], "..." if len(bad) > 16 else "")
    for i in sorted({0, n - 1}):  # the first row, and the last row of the last step
        assert got[i] == _oracle_proof(name, n, i), "%s, %d rows: row %d is not the oracle's proof" % (name, n, i)
    return got


@pytest.mark.parametrize("on_device", [False, True])
@pytest.mark.parametrize("name", ["c257", "c256"])
def test_seven_distinct_rows_below_and_at_the_domain_size(name, on_device):
    """257 constraints in a domain of 512 (n_constraints < N) and 256 in a domain of 256 (n_constraints == N)"""
    sy, pk = _prove_case(name)["sy"], _key(name)["pk"]
    N = 1 << pk.info()["log_domain"]
    assert (sy.n_constraints, N) == ((257, 512) if name == "c257" else (256, 256))
    assert g16.batch_info(pk)["batched"]
    _check_call(name, 7, on_device)


@pytest.mark.parametrize("on_device", [False, True])
def test_two_steps_the_last_of_one_row(on_device):
    """1025 rows of the 3-constraint system: step = min(1025, 4 * 256, ...) = 1024, so the first step is cut into chunks by prove_batch and the last step is one
    row, which prove_batch sends through the single prover; with device pointers the second step reads at w + 1024 * n_wires.  chunk_rows is a power of two up
    to 256, so it always divides the 1024 rows of the first step: what is asserted is that the step is more than one chunk.
    All 1025 rows are compared with the single prover (each single proof is made once and shared by the two variants): measured on an MI355X, 1.3 s for the
    variant that runs first and makes the 1025 single proofs, 0.05 s for the other."""
    info = g16.batch_info(_key("c3")["pk"])
    assert info["batched"] and 1 < info["chunk_rows"] < 1024 and 1024 % info["chunk_rows"] == 0, info
    t0 = time.perf_counter()
    _check_call("c3", 1025, on_device)
    print("1025 rows, on_device=%s: %.2f s" % (on_device, time.perf_counter() - t0))


@pytest.mark.parametrize("on_device", [False, True])
def test_a_key_the_batched_path_does_not_serve(on_device):
    assert not g16.batch_info(_key("c257", tables=False)["pk"])["batched"]
    got = _check_call("c257", 5, on_device, tables=False)
    assert got == [_singles("c257", True, 5, range(5))[i] for i in range(5)]  # and the key with tables writes the same bytes


@pytest.mark.parametrize("on_device", [False, True])
def test_one_proof(on_device):
    _check_call("c257", 1, on_device)


def test_a_system_without_constraints():
    """Defined for the single prover, by its code: zk_bn254_r1cs_load takes n_constraints = 0 (row pointers of one entry), Setup builds a domain of 1 whose
    transposed products are all zero (every A, B, K point is the point at infinity, which the fixed-base multiplication, the table build and the accumulate
    kernels handle per point), zk_bn254_groth16_prove_r1cs allocates one element for a, b, c, launches no product and calls zk_bn254_groth16_prove with
    n_constraints = 0 <= N = 1, which pads a, b, c with zeros.  A domain of 1 is not batched, so the batch entry sends the rows through the same prover:
    same bytes, or the same error."""
    sy = gs.System(0, 4, 2, [1], [((), (), ())] * 3)
    dev = sy.load()
    pk = None

    def outcome(fn):
        try:
            return ("proofs", fn())
        except _lib.ZkmiError as ex:
            return ("error", ex.code)

    try:
        pk, _ = zk.setup(dev, gs.mont_limbs(ref.rand_felts(0x7100, 5)))
        assert pk.log_domain == 0 and not g16.batch_info(pk)["batched"]
        W = witness_rows(3, 4, 0x7200)
        r, s = orc.rand_fr(0x7201, 3), orc.rand_fr(0x7202, 3)
        got = dev.eval_abc_rows(W)
        assert all(v.shape == (3, 0, 4) for v in got)
        want = outcome(lambda: [zk.prove_r1cs(dev, pk, W[i], r[i], s[i]) for i in range(3)])
        print("no constraints: the single prover gives", want[0], want[1] if want[0] == "error" else [p.hex()[:16] for p in want[1]])
        assert outcome(lambda: g16.prove_r1cs_batch(dev, pk, W, r, s)) == want
        buf = _lib.DeviceBuffer.from_numpy(W)
        assert outcome(lambda: g16.prove_r1cs_batch(dev, pk, buf, r, s, on_device=True)) == want
        assert sha_image(buf.to_numpy(np.uint64, W.shape)) == sha_image(W)
    finally:
        if pk is not None:
            pk.free()
        dev.free()
