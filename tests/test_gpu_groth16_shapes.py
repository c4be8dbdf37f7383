"""The device Groth16 prover at every small domain and wire split (-m gpu), bit-exact against the C oracle: every case of tests/groth16_shapes.py through every
door of the prover -- host inputs, device inputs, a key without window tables and with tables built afterwards, gnark's compact key layout from host and from
device memory -- and, grouped by key, as the rows of one zk.prove_batch call.  tests/test_groth16_shapes_cpu.py holds the table and its expectation."""
import ctypes as C
import functools

import numpy as np
import pytest

import noir_backend_using_gnark_amd as zk
from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import groth16 as g16
from oracle import oracle as orc
from tests import groth16_shapes as gs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    _lib.require_device()  # fail loudly: no silent fallback


_KEYS = {}


@functools.lru_cache(maxsize=None)
def _data(case):
    """(pkd, inputs, the oracle's 128 bytes): computed once per case (the key once per key part), shared by both tests, never written to"""
    if case.key_part not in _KEYS:
        _KEYS[case.key_part] = gs.key_dict(case)
    pkd = _KEYS[case.key_part]
    ins = gs.inputs(case)
    for v in ins:
        v.setflags(write=False)
    return pkd, ins, orc.groth16_prove(pkd, *ins)[0]


def _same(got, want, case, door):
    assert got == want, "%s through %s: %s differ" % (case.name, door, gs.differing_parts(got, want))


def _build_tables(pk):
    built = C.c_int(0)
    _lib.check(_lib.lib().zk_bn254_groth16_pk_build_tables(pk.handle, C.c_int(0), C.byref(built)))
    return bool(built.value)


@pytest.mark.parametrize("case", gs.CASES, ids=lambda c: c.name)
def test_every_door_gives_the_oracles_bytes(case):
    pkd, (a, b, c, w, r, s), want = _data(case)
    p = gs.predicates(case)
    geometry = dict(n_wires=case.n_wires, n_public=case.n_public, log_domain=case.log_domain)
    compact = gs.compact_key(case, pkd) if case.inf != "none" else None
    # ---- load 1 (the compact arrays from host memory where the key has a point at infinity): host inputs twice, then device inputs
    pk = zk.ProvingKey(**(compact or pkd))
    assert pk.info() == dict(geometry, tables=p["tables_possible"]), case.name
    _same(zk.prove(pk, a, b, c, w, r, s, n_constraints=case.n_constraints), want, case, "host inputs" + (", compact key" if compact else ""))
    _same(zk.prove(pk, a, b, c, w, r, s, n_constraints=case.n_constraints), want, case, "host inputs, second call on the key")
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (a, b, c, w)]
    _same(zk.prove(pk, *dev, r, s, n_constraints=case.n_constraints, on_device=True), want, case, "device inputs")
    for d, v, nm in zip(dev, (a, b, c, w), "abcw"):  # `direct` lets the first transform read a, b, c in place
        assert (d.to_numpy(np.uint64, v.shape) == v).all(), "%s: device inputs: %s was written to" % (case.name, nm)
    pk.free()
    # ---- load 2: no tables; then tables built on the resident key
    pk = zk.ProvingKey(**pkd, precompute_tables=False)
    assert pk.info() == dict(geometry, tables=False), case.name
    _same(zk.prove(pk, a, b, c, w, r, s, n_constraints=case.n_constraints), want, case, "no tables, host inputs")
    _same(zk.prove(pk, *dev, r, s, n_constraints=case.n_constraints, on_device=True), want, case, "no tables, device inputs")
    assert _build_tables(pk) == p["tables_possible"], case.name
    assert pk.info() == dict(geometry, tables=p["tables_possible"]), case.name
    _same(zk.prove(pk, a, b, c, w, r, s, n_constraints=case.n_constraints), want, case, "tables built after the load, host inputs")
    _same(zk.prove(pk, *dev, r, s, n_constraints=case.n_constraints, on_device=True), want, case, "tables built after the load, device inputs")
    pk.free()
    # ---- load 3: the compact arrays already in device memory
    if compact:
        D = _lib.DeviceBuffer.from_numpy
        bases = {k: D(compact[k]) for k in ("g1_a", "g1_b", "g1_k", "g1_z", "g2_b")}
        pk = zk.ProvingKey(**dict(compact, **bases), bases_on_device=True)
        assert pk.info() == dict(geometry, tables=p["tables_possible"]), case.name
        _same(zk.prove(pk, a, b, c, w, r, s, n_constraints=case.n_constraints), want, case, "compact key, bases on the device")
        pk.free()
        for d in bases.values():
            d.free()
    for d in dev:
        d.free()


@pytest.mark.parametrize("group", gs.batch_groups(), ids=lambda g: g[0])
def test_the_cases_of_one_key_as_rows_of_a_batch(group):
    name, cases = group
    pkd = _data(cases[0])[0]
    rows = [_data(c)[1] for c in cases]
    want = [_data(c)[2] for c in cases]
    nc = cases[0].n_constraints
    a, b, c, w, r, s = (np.ascontiguousarray(np.stack([row[k] for row in rows])) for k in range(6))
    pk = zk.ProvingKey(**pkd)
    assert g16.batch_info(pk)["batched"] == gs.predicates(cases[0])["batched_possible"], name
    single = [zk.prove(pk, *row, n_constraints=nc) for row in rows]
    for i, case in enumerate(cases):
        _same(single[i], want[i], case, "the single prover on the batch's key")
    got = zk.prove_batch(pk, a, b, c, w, r, s)
    assert len(got) == len(cases)
    for i, case in enumerate(cases):
        _same(got[i], single[i], case, "row %d of %d of a batch, host inputs" % (i, len(cases)))
    dev = [_lib.DeviceBuffer.from_numpy(v) for v in (a, b, c, w)]
    got = zk.prove_batch(pk, *dev, r, s, on_device=True, n_constraints=nc)
    for i, case in enumerate(cases):
        _same(got[i], single[i], case, "row %d of %d of a batch, device inputs" % (i, len(cases)))
    for d, v, nm in zip(dev, (a, b, c, w), "abcw"):
        assert (d.to_numpy(np.uint64, v.shape) == v).all(), "%s: device inputs: %s was written to" % (name, nm)
        d.free()
    pk.free()
