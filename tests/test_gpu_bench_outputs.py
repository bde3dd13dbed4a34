"""bench.py as a plain run (the headline figure alone) with --dump-outputs: the line carries what it must and nothing of --full, the
files hold the last timed step's proofs and verdict, are identical from run to run, and equal the oracle's prover on the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import cbind as C

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS = 256, 8                 # 8 steps: 4 calls of K = 2 batches, so the last step is the second batch of the last call


class _OracleEngine:
    def msm_many(self, off, scalars, pidx, points, flags=0):
        return C.msm_many(off, scalars, pidx, points, flags)


def _plain_run(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--batch", str(N), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    for j in (_plain_run(a), _plain_run(b)):
        assert j["steps"] == STEPS and j["unit"] == "proofs/s" and j["higher_is_better"] is True and j["dtype"] and j["metric"] == bench.METRIC
        assert abs(j["value"] - N * STEPS / (j["ms_per_step"] * STEPS * 1e-3)) < 1e-6 * j["value"]
        for k in ("cpu_baseline", "parity_checked", "kernel_ms_per_call", "roofline", "pipelined_proofs_per_s", "lone_call", "sustained", "e2e_host_buffers"):
            assert k not in j, k
    names = sorted(os.listdir(a))
    assert names == sorted(x + ".npy" for x in ("challenges", "responses", "commitments", "prove_status", "batch_check", "batch_status"))
    got = {}
    for nm in names:
        x, y = np.load(a / nm), np.load(b / nm)
        assert x.dtype in (np.float32, np.float64) and x.shape == y.shape and (x == y).all(), nm
        got[nm[:-4]] = x
    assert sum(x.nbytes for x in got.values()) <= bench.OUTPUT_BUDGET
    assert not got["batch_check"].any() and not got["batch_status"].any() and not got["prove_status"].any()
    # the same inputs on the host (run_workload's draws from default_rng(seed)), proven by the oracle: the dump is the last batch's proofs
    K, _ = bench.pick_call_shape(STEPS)
    st = bench.cmz_statement()
    rng = np.random.default_rng(1000)
    secrets, inst, common = bench.make_instance(_OracleEngine(), st, K * N, rng)
    ent = rng.integers(0, 256, size=(K * N, 32), dtype=np.uint8)
    secrets_l, points, cons = st
    names_p = [nm.decode() for nm, _ in points]
    cst = C.Statement(b"CMZ cred show n=10", [s.decode() for s in secrets_l], [(nm.decode(), c) for nm, c in points],
                      [(names_p[l], [(secrets_l[s].decode(), names_p[q]) for s, q in lc]) for l, lc in cons])
    com_rank, inst_rank = {}, {}
    for i, (_, c) in enumerate(points):
        (com_rank if c else inst_rank)[i] = len(com_rank if c else inst_rank)
    assert got["challenges"].shape == (N, 32) and got["responses"].shape == (N, len(secrets_l), 32)
    for r_ in range(N):
        j = (K - 1) * N + r_
        pts = np.stack([common[com_rank[i]] if i in com_rank else inst[inst_rank[i], j] for i in range(len(points))])
        ec, er, ek, _ = C.prove(cst, bench.LABEL, secrets[j], pts, ent[j].tobytes())
        assert (got["challenges"][r_] == ec).all() and (got["responses"][r_] == er).all() and (got["commitments"][r_] == ek).all(), r_


def test_plain_run_in_process_ranks(tmp_path):
    """a plain --gpus 3 --in-process run (all three ranks on this box's single GPU): one line from rank 0, its headline only, and rank 0's dump"""
    env = dict(os.environ, ZKP_BENCH_DRYRUN_ONE_GPU="1")
    env.pop("GPU_MAX_HW_QUEUES", None)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--in-process", "--steps", "4", "--warmup", "1", "--batch", "256", "--batches-per-call", "2",
           "--streams", "2", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 3 and j["steps"] == 4 and abs(j["value"] - 3 * 256 * 4 / (j["ms_per_step"] * 4e-3)) < 1e-6 * j["value"]
    assert "configs" not in j and "e2e_host_buffers" not in j and "kernel_ms_per_call" not in j
    assert np.load(tmp_path / "challenges.npy").shape == (256, 32) and not np.load(tmp_path / "batch_check.npy").any()
