"""CPU suite: the fast Setup reference of tests/groth16_setup_ref.py (which the device Setup is compared with in test_gpu_groth16_setup.py) against
the slow big-integer one, oracle/bn254_ref.groth16_setup, and against the committed key images of tests/golden/groth16_wire_golden.json."""
import json
import os

import pytest

from oracle import bn254_ref as ref
from oracle import oracle as orc
from oracle import plonk_ref as pl
from tests import groth16_setup_ref as gs
from tests.golden.gen_golden import small_r1cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nthreads", [1, 0])
def test_batched_generator_multiplication(nthreads):
    """orc_g1_mul_gen_many / orc_g2_mul_gen_many = orc_g1_mul / orc_g2_mul = bn254_ref, canonical and Montgomery scalars, zero -> (0,0)"""
    ks = [0, 1, 2, 15, 16, 255, ref.R - 1, ref.R - 2, (1 << 252) + 17] + ref.rand_felts(0x9A, 7)
    can, mont = gs.canon_limbs(ks), gs.mont_limbs(ks)
    g1, g2 = orc.g1_mul_gen_many(can, scalars_mont=False, nthreads=nthreads), orc.g2_mul_gen_many(can, scalars_mont=False, nthreads=nthreads)
    assert (orc.g1_mul_gen_many(mont, nthreads=nthreads) == g1).all() and (orc.g2_mul_gen_many(mont, nthreads=nthreads) == g2).all()
    assert not g1[0].any() and not g2[0].any()
    gen1, gen2 = g1[1], g2[1]
    assert gs._g1_tuples(gen1) == [ref.G1_GEN] and gs._g2_tuples(gen2) == [ref.G2_GEN]
    for i, k in enumerate(ks):
        assert (orc.g1_mul(gen1, mont[i]) == g1[i]).all() and (orc.g2_mul(gen2, mont[i]) == g2[i]).all(), k
    assert gs._g1_tuples(g1) == [ref.g1_mul(ref.G1_GEN, k) for k in ks]
    assert gs._g2_tuples(g2[:9]) == [ref.g2_mul(ref.G2_GEN, k) for k in ks[:9]]
    big = orc.rand_fr(0x9B, 3000)
    big[::97] = 0
    assert (orc.g1_mul_gen_many(big, nthreads=nthreads) == orc.g1_mul_gen_many(big, nthreads=1)).all()


def test_lagrange_basis_and_batch_inversion():
    tau = ref.rand_felts(0x9C, 1)[0]
    for n in (1, 2, 8):
        dom = ref.Domain(n)
        zt = (pow(tau, n, ref.R) - 1) % ref.R
        want = [zt * dom.card_inv * pow(dom.gen, j, ref.R) * pow(tau - pow(dom.gen, j, ref.R), -1, ref.R) % ref.R for j in range(n)]
        assert gs.lagrange_at(tau, n) == want
        assert sum(want) % ref.R == 1  # the basis sums to the constant polynomial 1
    with pytest.raises(AssertionError):
        gs.lagrange_at(ref.Domain(8).gen, 8)


def test_reference_reproduces_the_committed_key_images():
    with open(os.path.join(ROOT, "tests", "golden", "groth16_wire_golden.json")) as f:
        gold = {e["name"]: e for e in json.load(f)}
    toy = ref.R1CS(3, 1, [({3: 1}, {1: 1}, {2: 1})])
    for name, r1, tox in (("toy_x3_y2_z6", toy, (12345, 111, 222, 333, 444)),
                          ("seq_r1cs_13", small_r1cs(0x51, 3, 13)[0], tuple(ref.rand_felts(0x70, 5)))):
        out = gs.setup(gs.System.from_ref(r1), tox)
        assert out["pk_bytes"].hex() == gold[name]["pk_hex"], name
        assert out["vk_bytes"].hex() == gold[name]["vk_hex"], name


def test_reference_equals_the_big_integer_setup_on_a_skewed_system():
    """64 constraints: an empty column, an O-only wire, a duplicate wire in a row, ONE in every row, range columns -- byte for byte with
    bn254_ref.groth16_setup + plonk_ref.groth16_pk_bytes, the solver step with R1CS.eval_abc, and a proof with the key dict"""
    sy = gs.skewed_small()
    r1 = sy.to_ref()
    assert r1.constraints[5][0][7] == sum(sy.coef[v] for j, i, v in zip(*sy.sparse[0]) if j == 5 and i == 7) % ref.R
    tox = tuple(ref.rand_felts(0x65, 5))
    out = gs.setup(sy, tox, nthreads=2)
    pk, vk = ref.groth16_setup(r1, *tox)
    assert out["pk_bytes"] == pl.groth16_pk_bytes(pk)
    assert out["vk_bytes"] == pl.groth16_vk_bytes(dict(vk, g1_beta=pk["g1_beta"], g1_delta=pk["g1_delta"]))
    assert pk["g1_a"][23] is None and pk["g2_b"][23] is None and pk["g1_a"][22] is None and pk["g1_k"][22 - 3] is not None
    assert gs._g1_tuples(out["vk"]["g1_k"]) == vk["g1_ic"]
    w = [1] + ref.rand_felts(0x66, sy.n_wires - 1)
    w[4], w[5] = 0, ref.R - 1
    abc = sy.eval_abc(w)
    assert abc == tuple(r1.eval_abc(w))
    # the key dict proves as the oracle's own key does
    r, s = ref.rand_felts(0x67, 2)
    m = lambda xs: gs.mont_limbs(xs)
    got, _ = orc.groth16_prove(out["key"], *(m(v) for v in abc), m(w), m([r])[0], m([s])[0])
    assert got == ref.groth16_proof_bytes(*ref.groth16_prove(pk, r1.n_public, *abc, w, r, s))


def test_csr_form_holds_every_entry():
    """the CSR arrays handed to the device: row pointers, and (row, wire, value) as a multiset equal to the System's entries"""
    sy = gs.skewed_small()
    for m in range(3):
        ptr, idx, val = sy.csr(m, seed=m)
        got = sorted((j, int(idx[k]), gs.limbs_int(val[k]) * pow(ref.MONT_R, -1, ref.R) % ref.R)
                     for j in range(sy.n_constraints) for k in range(ptr[j], ptr[j + 1]))
        assert got == sorted(sy._entries(m)) and ptr[-1] == idx.size == val.shape[0]
