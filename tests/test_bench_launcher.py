"""bench.py honours --gpus N (the driver's contract): run directly with N > 1 it starts
N ranks under torch.distributed.run itself, under torchrun it insists WORLD_SIZE == N,
and it refuses N larger than the visible device count. The CPU rehearsal (--dry-run)
runs the real launcher and rendezvous (gloo) and reports n_gpus from the collective."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(MASTER_ADDR="127.0.0.1", **kw)
    return env


def test_launcher_spawns_n_ranks():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "3", "--dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 prints exactly one line
    out = lines[0]
    assert out["n_gpus"] == 3 and out["ranks_seen"] == 3 and out["rank_sum"] == 0 + 1 + 2


def test_eight_rank_rehearsal():
    """The N=8 shape the driver runs on an 8-GPU node, rehearsed on the CPU over gloo: eight ranks
    rendezvous, time a region between barriers, and rank 0 alone reports the whole-job value
    from the summed solutions and the slowest rank's time."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--dry-run"], capture_output=True, text=True,
                       env=_env(), timeout=480)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = lines[0]
    assert out["n_gpus"] == 8 and out["ranks_seen"] == 8 and out["rank_sum"] == sum(range(8))
    assert out["total_solutions"] == sum(100 + r for r in range(8))
    assert out["max_rank_seconds"] >= 0.08 > out["rank0_seconds"]  # the slowest rank (7) sets the time
    assert abs(out["value"] - out["total_solutions"] / out["max_rank_seconds"]) < 1e-6


def test_refuses_more_gpus_than_visible():
    # this container has no GPU: asking for 2 real ranks must fail before anything starts
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1"], capture_output=True, text=True,
                       env=_env(), timeout=240)
    assert p.returncode != 0
    assert "GPU(s) visible" in p.stderr


def test_world_size_must_match():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--dry-run"], capture_output=True, text=True,
                       env=_env(WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"), timeout=240)
    assert p.returncode != 0
    assert "WORLD_SIZE=2" in p.stderr


def test_plain_run_options_and_dump_layout(tmp_path):
    """--full is off by default (a plain run skips the re-verification); --dump-outputs writes
    float32 arrays with each nonce's solutions in lexicographic order, whatever order they came in."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = bench.parse(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full is True and a.dump_outputs == str(tmp_path)
    s0, s1, s2 = bytes([9] * 6), bytes([1, 2, 3, 4, 5, 6]), bytes([1, 2, 3, 4, 5, 7])
    for order in ([s0, s1], [s1, s0]):
        bench.dump_outputs(str(tmp_path), [order, [], [s2]])
        got = {n: np.load(tmp_path / f"{n}.npy") for n in ("solutions_per_nonce", "solution_nonce", "solutions")}
        assert all(v.dtype == np.float32 for v in got.values())
        assert got["solutions_per_nonce"].tolist() == [2, 0, 1]
        assert got["solution_nonce"].tolist() == [0, 0, 2]
        assert got["solutions"].tolist() == [list(s1), list(s0), list(s2)]
    bench.dump_outputs(str(tmp_path / "r"), [[], []], rank=1)
    assert np.load(tmp_path / "r" / "solutions_rank1.npy").shape == (0, 0)
    assert np.load(tmp_path / "r" / "solutions_per_nonce_rank1.npy").tolist() == [0, 0]


@pytest.mark.gpu
def test_dump_outputs_is_the_last_timed_step(tmp_path):
    """A small plain run (2 steps of 16 nonces; 74 solutions, well over the 1.85 per nonce floor):
    --steps sets the timed steps, ms_per_step is reported, and the dump holds exactly the
    solutions of the last timed step's inputs, each valid under the CPU consensus verifier."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from bitcoincashplus_amd import native
    batch, steps = 16, 2
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--batch", str(batch), "--steps", str(steps),
                        "--warmup", "1", "--dump-outputs", str(tmp_path)], capture_output=True, text=True,
                       env=_env(), timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == steps and out["ms_per_step"] > 0 and out["config"]["full"] is False
    assert out["config"]["verified"] is None  # the re-verification belongs to --full
    assert abs(out["value"] * out["ms_per_step"] * steps / 1000
               - out["config"]["solutions_per_nonce"] * batch * steps) < 0.5
    counts = np.load(tmp_path / "solutions_per_nonce.npy")
    slots = np.load(tmp_path / "solution_nonce.npy")
    sols = np.load(tmp_path / "solutions.npy")
    assert counts.dtype == slots.dtype == sols.dtype == np.float32
    assert counts.shape == (batch,) and sols.shape == (len(slots), 1344) and counts.sum() == len(slots)
    states = bench.step_states(native, batch, steps - 1)
    want = native.EquihashGpuSolver(200, 9, batch, 0).solve(states)
    assert counts.tolist() == [len(w) for w in want]
    assert slots.tolist() == [b for b, w in enumerate(want) for _ in w]
    got = [bytes(r) for r in sols.astype(np.uint8)]
    assert got == [s for w in want for s in sorted(w)]
    for b, s in zip(slots.astype(int), got):
        assert native.eh_is_valid_solution(200, 9, states[b], s)[0]


def test_launch_command_shape():
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake(cmd, env):
        seen["cmd"], seen["env"] = cmd, env
        return 7
    rc = bench.launch_ranks(["--gpus", "8", "--steps", "5"], 8, launcher=fake)
    assert rc == 7
    cmd = seen["cmd"]
    assert cmd[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=8" in cmd and "--master-addr=127.0.0.1" in cmd
    assert cmd[-4:] == ["--gpus", "8", "--steps", "5"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
