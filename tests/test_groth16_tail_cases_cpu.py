"""CPU suite for the Groth16 proof tail's case builder (tests/groth16_tail_cases.py) and for the interface of the batched tail: every tagged case is what its
tag says, the builder's expectation (gnark's arrangement) is also the library's arrangement, the two new entries are declared and exported, and the C++
mirror with FinalizeBatch compiles and refuses bad arguments without a device."""
import os
import subprocess

import numpy as np

from noir_backend_using_gnark_amd import _lib
from oracle import bn254_ref as ref
from tests import groth16_tail_cases as tc
from tests.helpers import from_mont_limbs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAGS = {"all_sums_at_infinity", "A_at_infinity", "B1_at_infinity", "K_at_infinity_junk_xy", "Z_at_infinity", "B2_at_infinity_junk_xy", "A_is_minus_alpha",
        "B1_is_minus_beta", "Bs_at_infinity", "Ar_at_infinity", "K_equals_Z", "K_is_minus_Z", "Krs_at_infinity", "r_zero", "s_zero", "r_and_s_zero", "r_one",
        "s_is_r_mod_minus_1", "random_0", "random_1"}


def _fp_ints(limbs):
    return from_mont_limbs(np.asarray(limbs, dtype=np.uint64).reshape(-1, 4), ref.Q)


def _g1_of_record(rec16):
    """affine point of a 16-limb XYZZ image, through its own zz / zzz (None when zz == 0)"""
    x, y, zz, zzz = _fp_ints(rec16)
    if zz == 0:
        return None
    assert zz ** 3 % ref.Q == zzz * zzz % ref.Q and zz != 1, "not an XYZZ image with a projective factor other than 1"
    return (x * ref.inv(zz, ref.Q) % ref.Q, y * ref.inv(zzz, ref.Q) % ref.Q)


def _g2_of_record(rec32):
    v = _fp_ints(rec32)
    x, y, zz, zzz = ((v[2 * i], v[2 * i + 1]) for i in range(4))
    if zz == (0, 0):
        return None
    assert ref.f2_mul(ref.f2_sqr(zz), zz) == ref.f2_sqr(zzz) and zz != (1, 0)
    return (ref.f2_mul(x, ref.f2_inv(zz)), ref.f2_mul(y, ref.f2_inv(zzz)))


def _sums_of(row):
    acc = [None] * 5
    for rec in row.partials:
        for k in range(4):
            acc[k] = ref.g1_add(acc[k], _g1_of_record(rec[16 * k:16 * k + 16]))
        acc[4] = ref.g2_add(acc[4], _g2_of_record(rec[64:96]))
    return tuple(acc)


def _named(pts, sums, r, s):
    A, B1, K, Z, B2 = sums
    ar, bs, krs = tc.library_arrangement(pts, sums, r, s)
    return {"A": A, "B1": B1, "K": K, "Z": Z, "B2": B2, "A+alpha": ref.g1_add(A, pts["alpha"]), "B1+beta": ref.g1_add(B1, pts["beta"]),
            "K+Z": ref.g1_add(K, Z), "Ar": ar, "Bs": bs, "Krs": krs}


def test_the_tagged_cases_are_all_there():
    assert {r.tag for r in tc.tagged_rows()} == TAGS
    assert [r.tag for r in tc.tagged_rows_3()] == ["np3_equal_equal_opposite", "np3_all_at_infinity_junk_xy"]
    assert all(r.expected is not None and len(r.expected) == 128 for r in tc.tagged_rows() + tc.tagged_rows_3())


def test_every_tagged_case_meets_its_precondition():
    for which in ("base", "other"):
        _, pts = tc.key(which)
        assert ref.g1_on_curve(pts["alpha"]) and ref.g1_on_curve(pts["delta"]) and ref.g2_on_curve(pts["delta2"])
        for row in tc.tagged_rows(which) + (tc.tagged_rows_3(which) if which == "base" else ()):
            sums = _sums_of(row)  # from the limbs the library will read, not from the builder's bookkeeping
            assert sums == row.pre["sums"], row.tag
            assert all(ref.g1_on_curve(P) for P in sums[:4]) and ref.g2_on_curve(sums[4]), row.tag
            r, s = from_mont_limbs(row.r)[0], from_mont_limbs(row.s)[0]
            assert (r, s) == (row.pre["r"], row.pre["s"]), row.tag
            named = _named(pts, sums, r, s)
            for name in row.pre["inf"]:
                assert named[name] is None, (row.tag, name)
            if row.pre.get("k_equals_z"):
                assert sums[2] == sums[3] and sums[2] is not None
            if "junk_xy" in row.tag:  # a point at infinity that is not all zeros
                g1s = [rec[16 * k:16 * k + 16] for rec in row.partials for k in range(4)]
                junk = [rec[8:].max() == 0 and rec[:4].max() != 0 and rec[4:8].max() != 0 for rec in g1s]
                junk += [rec[80:96].max() == 0 and rec[64:72].max() != 0 and rec[72:80].max() != 0 for rec in row.partials]
                assert any(junk), row.tag
    by = {r.tag: r for r in tc.tagged_rows()}
    assert by["r_zero"].pre["r"] == 0 and by["s_zero"].pre["s"] == 0 and by["r_and_s_zero"].pre["r"] == by["r_and_s_zero"].pre["s"] == 0
    assert by["r_one"].pre["r"] == 1 and by["s_is_r_mod_minus_1"].pre["s"] == ref.R - 1
    three = tc.tagged_rows_3()[0]
    p = [_g1_of_record(rec[:16]) for rec in three.partials]
    assert p[0] == p[1] and p[2] == ref.g1_neg(p[0]) and not (three.partials[0] == three.partials[1]).all()


def test_gnark_arrangement_and_library_arrangement_agree():
    for which in ("base", "other"):
        _, pts = tc.key(which)
        for row in tc.tagged_rows(which) + tc.tagged_rows_3(which):
            got = ref.groth16_proof_bytes(*tc.library_arrangement(pts, row.pre["sums"], row.pre["r"], row.pre["s"]))
            assert got == row.expected, row.tag
    inf = ref.groth16_proof_bytes(None, None, None)  # gnark's encoding of the point at infinity in all three places
    by = {r.tag: r for r in tc.tagged_rows()}
    assert by["Ar_at_infinity"].expected[:32] == inf[:32] and by["Bs_at_infinity"].expected[32:96] == inf[32:96]
    assert by["Krs_at_infinity"].expected[96:] == inf[96:]
    assert by["random_0"].expected[:32] != inf[:32]


def test_bulk_rows_and_assemble_shapes():
    parts, r, s, placed = tc.assemble(9, 1, 5, tc.tagged_rows(), [0, 4, 8, 12])
    assert parts.shape == (9, 1, 96) and r.shape == s.shape == (9, 4) and sorted(placed) == [0, 4, 8]
    assert (parts[4] == placed[4].partials).all() and (r[8] == placed[8].r).all()
    p3, _, _ = tc.bulk_rows(4, 3, 6)
    assert p3.shape == (4, 3, 96)
    zz_zero = [p3[i, j, 16 * k + 8:16 * k + 12].max() == 0 for i in range(4) for j in range(3) for k in range(4)] + [p3[i, j, 80:88].max() == 0 for i in range(4) for j in range(3)]
    assert sum(zz_zero) == 1  # record 9 of 12 carries one point at infinity


def test_the_two_entries_are_declared_and_exported():
    names = ["zk_bn254_groth16_finalize_batch", "zk_bn254_groth16_finalize_batch_dev"]
    for n in names:
        assert n in _lib.SYMBOLS, n
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for n in names:
        assert n in exported, n
        assert hasattr(_lib.lib(), n)
    hdr = open(os.path.join(ROOT, "include", "zkmi.h")).read()
    assert all(n + "(" in hdr for n in names)
    from noir_backend_using_gnark_amd import groth16 as g16
    assert callable(g16.finalize_batch)


def test_cpp_mirror_with_finalize_batch_compiles_and_refuses_bad_arguments(tmp_path):
    exe = str(tmp_path / "finalize_batch_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "finalize_batch_check.cpp"), "-L" + os.path.join(ROOT, "noir_backend_using_gnark_amd"), "-lzkmi",
                           "-Wl,-rpath," + os.path.join(ROOT, "noir_backend_using_gnark_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_tail_arithmetic_on_the_host_gives_the_pure_python_bytes(tmp_path):
    """csrc/groth16_tail.hpp -- the functions the kernel's four roles and its combine step call -- compiled as host code and run over every tagged row
    (tests/cpp/tail_math_check.cpp): the bytes must be the builder's.  What stays for the GPU tests is the kernel's indexing and its exchange through LDS."""
    csrc = os.path.join(ROOT, "noir_backend_using_gnark_amd", "csrc")
    exe = str(tmp_path / "tail_math_check")
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-O0", "-std=c++17", "-Wno-unused-result", "-I" + csrc,
                           os.path.join(ROOT, "tests", "cpp", "tail_math_check.cpp"), "-o", exe])
    pkd, _ = tc.key()
    for k, rows in enumerate((tc.tagged_rows(), tc.tagged_rows_3())):
        blob = np.array([len(rows), rows[0].partials.shape[0]], np.uint64).tobytes()
        blob += b"".join(np.ascontiguousarray(pkd[name], np.uint64).tobytes() for name in ("g1_alpha", "g1_beta", "g1_delta", "g2_beta", "g2_delta"))
        for row in rows:
            blob += row.partials.tobytes() + row.r.tobytes() + row.s.tobytes() + row.expected
        path = tmp_path / ("rows%d.bin" % k)
        path.write_bytes(blob)
        out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and out.stdout.strip() == "ok %d" % len(rows), out.stdout + out.stderr
