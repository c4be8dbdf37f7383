"""The host model of the Horner scan's stages (tests/hscan_ref.py) against the oracle's polynomial code (oracle/plonk_ref.py: poly_eval,
divide_by_x_minus_a) and against the scan plan (tests/plonk_shapes.py scan_plan = csrc/scan.hpp scan_plan); the bound that keeps the chunk loop of the blocks
pass out of every planned scan; and the argument errors of zk_bn254_hscan_inspect, which are decided before a device is looked for.  No device."""
import random

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib, kzg
from oracle import plonk_ref as pl
from tests import hscan_ref as hr
from tests.plonk_shapes import scan_plan

R = hr.R


def _points(rng, f):
    return (0, 1, R - 1, rng.randrange(R))


@pytest.mark.parametrize("K", [1, 2, 3, 8, 9])
def test_every_stage_is_a_polynomial_evaluation(K):
    """each stage is, by its definition, the value at a of a slice of the row: poly_eval says the same"""
    rng = random.Random(K)
    W = 256 * K
    for n in hr.lengths_for(K):
        f = [rng.randrange(R) for _ in range(n)]
        for a in _points(rng, f)[:2 if n > W else 4] + (rng.randrange(R),):
            for nb in (0, hr.scan_blocks(n, K) + 1):
                m = hr.stages(f, a, K, nb)
                assert m["nb"] == (nb or hr.scan_blocks(n, K)) and len(m["btot"]) == len(m["btot_local"]) == len(m["tcarry"]) == m["nb"]
                assert m["total"] == pl.poly_eval(f, a)
                assert m["q"][:-1] == pl.divide_by_x_minus_a(f, m["total"], a) and m["q"][-1] == 0 and len(m["q"]) == n
                for b in range(m["nb"]):
                    lo, hi = W * b, W * (b + 1)
                    assert m["btot_local"][b] == pl.poly_eval(f[lo:hi], a), (n, b)
                    assert m["btot"][b] == pl.poly_eval(f[hi:], a), (n, b)
                    assert m["tcarry"][b][255] == 0
                    for t in (0, 1, 2, 127, 253, 254) if n > W else range(255):
                        assert m["tcarry"][b][t] == pl.poly_eval(f[lo + (t + 1) * K:hi], a), (n, b, t)


def test_stages_recombine_to_the_suffix_values():
    """S at a lane's end = its lane carry + a^(distance to the workgroup's end) * the workgroup's carry: the identity pass 3 rests on"""
    rng = random.Random(5)
    K, n = 3, 2 * 768 + 4
    f, a = [rng.randrange(R) for _ in range(n)], rng.randrange(R)
    m, S = hr.stages(f, a, K), hr.suffix(f, a)
    for b in range(m["nb"]):
        for t in range(256):
            i = 768 * b + (t + 1) * K
            if i <= n:
                assert S[i] == (m["tcarry"][b][t] + pow(a, 768 * (b + 1) - i, R) * m["btot"][b]) % R, (b, t)


def test_root_and_degenerate_points():
    rng = random.Random(6)
    f = hr.poly_with_root(rng, 2000, 12345)
    m = hr.stages(f, 12345, 3)
    assert m["total"] == 0 and any(m["btot"]) and any(m["btot_local"]) and any(any(t) for t in m["tcarry"])
    m = hr.stages(f, 0, 3)
    assert m["q"] == f[1:] + [0] and m["total"] == f[0]
    w = hr.element_of_order(256)
    assert pow(w, 256, R) == 1 and pow(w, 128, R) != 1
    w3 = hr.element_of_order(3)
    assert w3 not in (None, 1) and pow(w3, 3, R) == 1
    assert hr.element_of_order(17) is None  # 17 does not divide r - 1: Fr has no 17th root of unity but 1


def test_scan_plan_matches_and_never_needs_the_chunk_loop():
    """scan_plan gives K = max(8, ceil(len / 2^18)), so len <= K 2^18: at most 2^18 lanes, 1024 workgroups of 256 -- the blocks pass of a PLANNED scan is one
    chunk of at most 1024 totals.  Around every step of K up to 2^24 (K = 64) and at the small lengths."""
    lengths = set(range(1, 70)) | {2047, 2048, 2049, (1 << 21) + 3}
    for k in range(1, 65):
        lengths |= {k << 18, (k << 18) - 1, (k << 18) + 1}
    seen = set()
    for n in sorted(lengths):
        K, nb = scan_plan(n)
        assert K == max(8, -(-n // (1 << 18))) and nb == hr.scan_blocks(n, K)
        assert 1 <= nb <= 1024 and (nb - 1) * 256 * K < n <= nb * 256 * K, (n, K, nb)
        seen.add(K)
    assert seen == set(range(8, 66))
    assert scan_plan(1 << 24) == (64, 1024) and scan_plan((1 << 21) + 3) == (9, 911)
    # the chunk loop needs nb > 1024, which only a K below the plan's gives: the stage tests force K = 1
    assert hr.scan_blocks(256 * 1024, 1) == 1024 and hr.scan_blocks(256 * 1024 + 1, 1) == 1025 and hr.scan_blocks(256 * 2048 + 1, 1) == 2049


def test_inspection_entry_argument_errors_need_no_device():
    assert "zk_bn254_hscan_inspect" in _lib.SYMBOLS and hasattr(_lib.lib(), "zk_bn254_hscan_inspect")
    f, a = pl.ints_to_mont_np([1, 2, 3, 4, 5]), pl.ints_to_mont_np([7])[0]
    long_row = np.zeros((600, 4), np.uint64)
    bad = [dict(rows=[], K=8), dict(rows=[(f.copy(), a) for _ in range(9)], K=8), dict(rows=[(f, a)], K=0),
           dict(rows=[(long_row, a)], K=1, nb=2),                      # 600 lanes need three workgroups
           dict(rows=[(f, a), (long_row, a)], K=1, nb=1),              # the longest row decides
           dict(rows=[(f, a), (f, a)], K=8, mode="in_place"),          # one array divided in place twice
           dict(rows=[(long_row, a)], K=1, nb=65537)]
    for kw in bad:
        with pytest.raises(_lib.ZkmiError) as ei:
            kzg.hscan_inspect(**kw)
        assert ei.value.code == _lib.ZK_ERR_ARG, kw
    with pytest.raises(ValueError):
        kzg.hscan_inspect([(f, a)], 8, mode="both")
