"""bench.py --dump-outputs DIR and --steps: the timed path's last proof written as DIR/proof.npy, and the number of timed steps the line reports."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BARE = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "ZKMI_DIST_BACKEND")}


def bench(*args, timeout=300):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=timeout, env=BARE)


def test_steps_below_one_is_refused():
    run = bench("--steps", "0", "--dry-launch")
    assert run.returncode == 2 and "--steps must be at least 1" in run.stderr


def test_dump_outputs_passes_through_the_launcher():
    run = bench("--gpus", "2", "--steps", "3", "--dump-outputs", "out", "--dry-launch")
    assert run.returncode == 0, run.stderr[-2000:]
    cmd = json.loads(run.stdout.strip().splitlines()[-1])["dry_launch"]["command"]
    assert cmd[-2:] == ["--dump-outputs", "out"]  # rank 0 of the launched ranks writes the file


def test_full_passes_through_the_launcher():
    run = bench("--gpus", "2", "--steps", "3", "--full", "--dry-launch")
    assert run.returncode == 0, run.stderr[-2000:]
    cmd = json.loads(run.stdout.strip().splitlines()[-1])["dry_launch"]["command"]
    assert cmd[-1] == "--full"  # every rank runs the blocks after the timed region: their collectives need all of them


def test_dump_outputs_writes_the_proof_bytes_exactly(tmp_path):
    from bench_blocks.common import dump_outputs
    proof = bytes(range(128))
    dump_outputs(str(tmp_path / "d"), proof)
    got = np.load(tmp_path / "d" / "proof.npy")
    assert got.dtype == np.float64 and got.shape == (128,)
    assert bytes(got.astype(np.uint8)) == proof


@pytest.mark.gpu
def test_dump_outputs_holds_the_timed_proof(tmp_path):
    """One --full bench run at 2^12 constraints: the dumped proof is the one the line's proof_sha names and the one the CPU oracle computes, and the line reports
    exactly the timed steps it was asked for."""
    run = bench("--log-n", "12", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path), "--full", timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    out = json.loads(run.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    got = np.load(tmp_path / "proof.npy")
    assert got.dtype == np.float64 and got.shape == (128,)
    proof = bytes(got.astype(np.uint8))
    assert hashlib.sha256(proof).hexdigest()[:16] == out["proof_sha"]
    assert out["cpu_baseline"]["proof_bytes_match_gpu"] and "parity_error" not in out


@pytest.mark.gpu
def test_plain_run_is_the_headline_only(tmp_path):
    """Without --full a run stops after the timed steps: the line holds the headline and no block of the full run, and its dumped proof is the one a
    --full run of the same seeded instance times."""
    plain = bench("--log-n", "12", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "plain"), timeout=600)
    assert plain.returncode == 0, plain.stdout[-2000:] + plain.stderr[-2000:]
    lines = [l for l in plain.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["higher_is_better"] is True and out["dtype"] == "u32" and out["metric"] and out["unit"]
    assert out["roofline"] is None and "parity_error" not in out
    for k in ("cpu_baseline", "prove_ms_host_inputs", "prove_ms_witness_like_scalars", "inner_boundary_2p12", "go_toolchain"):
        assert k not in out, k
    proof = bytes(np.load(tmp_path / "plain" / "proof.npy").astype(np.uint8))
    assert hashlib.sha256(proof).hexdigest()[:16] == out["proof_sha"]
    full = bench("--log-n", "12", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--full", timeout=600)
    assert full.returncode == 0, full.stdout[-2000:] + full.stderr[-2000:]
    fout = json.loads(full.stdout.strip().splitlines()[-1])
    assert fout["proof_sha"] == out["proof_sha"] and fout["roofline"]["kernel"] and "go_toolchain" in fout
