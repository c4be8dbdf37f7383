"""CPU checks behind tests/test_gpu_groth16_shapes.py: the two references -- the C oracle (orc.groth16_prove) and Python integers (bn254_ref.groth16_prove) --
give the same 128 bytes on the cases small enough for the latter; the table reaches every branch of csrc/groth16.hip it names; and the expectation can catch
the errors the shapes are there for (K paired one wire off, padding that is not zero, a point at infinity that is not skipped)."""
import functools
import importlib

import numpy as np
import pytest

from oracle import bn254_ref as ref
from oracle import oracle as orc
from tests import groth16_shapes as gs
from tests.helpers import from_mont_limbs

CASES = gs.CASES
SMALL = [c for c in CASES if c.n_wires <= 40 and c.N <= 32]   # the Python reference takes 0.03 s per case at N <= 8, seconds beyond this bound


@functools.lru_cache(maxsize=None)
def _key(case):
    """the case's key, generated once; callers change it through dict(...) copies only"""
    pkd = gs.key_dict(case)
    for v in pkd.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return pkd


@functools.lru_cache(maxsize=None)
def _oracle(case):
    return orc.groth16_prove(_key(case), *gs.inputs(case))[0]


def _g1(arr):
    v = from_mont_limbs(np.asarray(arr, np.uint64).reshape(-1, 4), ref.Q)
    return [None if (v[i], v[i + 1]) == (0, 0) else (v[i], v[i + 1]) for i in range(0, len(v), 2)]


def _g2(arr):
    v = from_mont_limbs(np.asarray(arr, np.uint64).reshape(-1, 4), ref.Q)
    return [None if v[i:i + 4] == [0, 0, 0, 0] else ((v[i], v[i + 1]), (v[i + 2], v[i + 3])) for i in range(0, len(v), 4)]


def _ref_key(pkd):
    pk = {k: _g1(pkd[k]) for k in ("g1_a", "g1_b", "g1_k", "g1_z")}
    pk.update({k: _g1(pkd[k])[0] for k in ("g1_alpha", "g1_beta", "g1_delta")})
    pk.update({k: _g2(pkd[k])[0] for k in ("g2_beta", "g2_delta")})
    pk["g2_b"] = _g2(pkd["g2_b"])
    pk["domain"] = ref.Domain(1 << pkd["log_domain"])
    return pk


def test_names_are_unique_and_seeds_depend_on_the_name_only():
    assert 60 <= len(CASES) <= 90
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES[::7]:
        twin = gs.Case(c.name, *c[1:])
        for x, y in zip(gs.inputs(c), gs.inputs(twin)):
            assert (x == y).all()
        # another name, the same shape: other data; the same key part: the same key
        other = gs.make_case(c.log_domain, c.n_wires, c.n_public, c.n_constraints, c.w, c.abc, c.rs, c.inf, tag="other_")
        assert other.key_part == c.key_part and other.name != c.name
        if c.w == "uniform":
            assert not (gs.inputs(other)[3] == gs.inputs(c)[3]).all()
        k0, k1 = gs.key_dict(c), gs.key_dict(other)
        assert all(np.array_equal(k0[k], k1[k]) for k in k0)


def test_the_table_holds_what_it_promises():
    shapes = {(c.log_domain, c.n_wires, c.n_public) for c in CASES}
    for ld in range(9):
        N = 1 << ld
        for nw in (N - 1, N, N + 1):
            if nw >= 1:
                assert any(c.log_domain == ld and c.n_wires == nw and c.n_public == min(2, nw) and c.n_constraints == N and (c.w, c.abc, c.inf) == ("uniform", "sat", "none")
                           for c in CASES), (ld, nw)
    for ld in (1, 3, 6):
        for nw in (1, 2, 3 << ld):
            for npub in {1, 2, nw - 1, nw}:
                if 1 <= npub <= nw:
                    assert (ld, nw, npub) in shapes
    for ld in (1, 4, 7):
        assert {0, 1, (1 << ld) - 1, 1 << ld} <= {c.n_constraints for c in CASES if c.log_domain == ld}
    for w in gs.W_KINDS:   # the Latin square: every kind at both domains and at both splits
        at = {(c.log_domain, c.n_public) for c in CASES if c.w == w and c.log_domain in (2, 5) and c.n_public in (1, 3)}
        assert {ld for ld, _ in at} == {2, 5} and {p for _, p in at} == {1, 3}, w
    assert {c.abc for c in CASES} == set(gs.ABC_KINDS) and {c.rs for c in CASES} == set(gs.RS_KINDS) and {c.inf for c in CASES} == set(gs.INF_KINDS)
    assert {(1, 5000, 3), (12, 2, 1), (12, 2, 2)} <= shapes
    assert all(c.log_domain <= 8 and c.n_wires <= 768 for c in CASES if (c.log_domain, c.n_wires, c.n_public) not in {(1, 5000, 3), (12, 2, 1), (12, 2, 2)})


def test_predicates_are_true_of_the_data():
    for c in CASES:
        a, b, cc, w, _, _ = gs.inputs(c)
        p = gs.predicates(c)
        assert p["w_has_no_pairs"] == (not w.any()), c.name
        assert a.shape == b.shape == cc.shape == (c.n_constraints, 4) and w.shape == (c.n_wires, 4)
        h = orc.groth16_compute_h(a, b, cc, c.log_domain) if c.n_constraints else np.zeros((c.N, 4), np.uint64)
        if c.N > 1:   # (at N = 1 Z's multi-exp is over N - 1 = 0 points whatever h is)
            assert p["h_is_zero"] == (not h[:c.N - 1].any()), c.name
        ia, ib = gs.infinity_bitmaps(c)
        pkd = _key(c)
        assert ((pkd["g1_a"] == 0).all(axis=1) == ia).all() and ((pkd["g1_b"] == 0).all(axis=1) == ib).all() and ((pkd["g2_b"] == 0).all(axis=1) == ib).all()
        assert pkd["g1_k"].shape[0] == c.n_wires - c.n_public and pkd["g1_z"].shape[0] == c.N
        assert (ia.any() or ib.any()) == (c.inf != "none")


def test_coverage_of_every_branch():
    assert len(SMALL) * 4 >= len(CASES) * 3
    for name in gs.PREDICATES:
        on = [c for c in CASES if gs.predicates(c)[name]]
        assert len(on) >= 2 and len(CASES) - len(on) >= 2, name
        assert any(gs.predicates(c)[name] for c in SMALL), name
    for what, hit in (("nk == 0", lambda c: c.n_public == c.n_wires), ("n_public == 1", lambda c: c.n_public == 1),
                      ("w_has_no_pairs", lambda c: gs.predicates(c)["w_has_no_pairs"]), ("h_is_zero", lambda c: gs.predicates(c)["h_is_zero"])):
        assert {gs.predicates(c)["tables_possible"] for c in CASES if hit(c)} == {False, True}, what
    assert any(c.n_wires == 1 and c.n_public == 1 and c.N == 2 for c in CASES)


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_the_two_references_agree(case):
    pkd = _key(case)
    a, b, c, w, r, s = (from_mont_limbs(v) for v in gs.inputs(case))
    ar, bs, krs = ref.groth16_prove(_ref_key(pkd), case.n_public, a, b, c, w, r[0], s[0])
    want = ref.groth16_proof_bytes(ar, bs, krs)
    got = _oracle(case)
    assert got == want, (case.name, gs.differing_parts(got, want))


def test_a_shifted_k_pairing_changes_the_bytes():
    """K paired with w[n_public - 1:] instead of w[n_public:] -- the oracle is given that prover as a key with one public wire fewer whose K ends with a point at
    infinity.  A witness that is constant from wire n_public - 1 on (ones, max) equals its own shift: those cases cannot see this error and are left out."""
    hits = 0
    for c in CASES:
        a, b, cc, w, r, s = gs.inputs(c)
        tail = w[c.n_public - 1:]
        if c.n_wires == c.n_public or not w[c.n_public].any() or (tail == tail[0]).all():
            continue
        pkd = _key(c)
        shifted = dict(pkd, n_public=c.n_public - 1, g1_k=np.concatenate([pkd["g1_k"], np.zeros((1, 8), np.uint64)]))
        bad = orc.groth16_prove(shifted, a, b, cc, w, r, s)[0]
        assert bad[:96] == _oracle(c)[:96] and bad[96:] != _oracle(c)[96:], c.name
        hits += 1
    assert hits >= 5


def test_a_one_in_the_padding_changes_the_bytes():
    hits = 0
    for c in CASES:
        if not 0 < c.n_constraints < c.N:
            continue
        a, b, cc, w, r, s = gs.inputs(c)
        pad = np.tile(gs.ONE, (c.N - c.n_constraints, 1))
        bad = orc.groth16_prove(_key(c), *(np.concatenate([v, pad]) for v in (a, b, cc)), w, r, s)[0]
        assert bad[:96] == _oracle(c)[:96] and bad[96:] != _oracle(c)[96:], c.name
        hits += 1
    assert hits >= 5


def test_an_infinity_in_a_that_is_not_skipped_changes_the_bytes():
    hits = 0
    for c in CASES:
        ia, _ = gs.infinity_bitmaps(c)
        if not ia.any():
            continue
        full = gs.key_dict(c, with_infinity=False)
        pkd = dict(_key(c), g1_a=full["g1_a"])
        bad = orc.groth16_prove(pkd, *gs.inputs(c))[0]
        assert bad[:32] != _oracle(c)[:32] and bad[32:96] == _oracle(c)[32:96], c.name
        hits += 1
    assert hits >= 5


def test_the_gpu_file_runs_every_case_and_every_case_is_a_batch_row():
    mod = importlib.import_module("tests.test_gpu_groth16_shapes")
    for fn, want in ((mod.test_every_door_gives_the_oracles_bytes, list(CASES)), (mod.test_the_cases_of_one_key_as_rows_of_a_batch, gs.batch_groups())):
        marks = [m for m in fn.pytestmark if m.name == "parametrize"]
        assert len(marks) == 1 and list(marks[0].args[1]) == want
        assert not [m for m in fn.pytestmark if m.name in ("skip", "skipif", "xfail")]
    assert not [m for m in getattr(mod.pytestmark, "__iter__", lambda: [mod.pytestmark])() if m.name in ("skip", "skipif", "xfail")]
    rows = [c for _, group in gs.batch_groups() for c in group]
    assert {c.name for c in rows} >= {c.name for c in CASES} and len({c.name for c in rows}) == len(rows)
    for _, group in gs.batch_groups():
        assert len(group) >= 2 and len({(c.key_part, c.n_constraints) for c in group}) == 1
        for i, c in enumerate(group):
            if c.w == "zero":
                assert 0 < i < len(group) - 1 and group[i - 1].w != "zero" and group[i + 1].w != "zero", c.name
