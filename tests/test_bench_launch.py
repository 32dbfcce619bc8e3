"""bench.py --gpus N must be able to start its own ranks (the driver may run it without torchrun), and must also
work when torchrun already did.  CPU plumbing check with the stand-in step (gloo): spawn, rendezvous on 127.0.0.1,
barrier-bracketed timing, MAX over ranks, exactly ONE JSON line from rank 0."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _json_lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    return env


def test_bench_self_launches_two_ranks():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--standin"], capture_output=True, text=True, timeout=600, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and line["steps"] == 3 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and "STAND-IN" in line["data"]
    # rank 0 explains the line: every rank's own time and the time inside the pixel all-gather, min / max over the ranks
    pr = line["per_rank"]
    assert 0 < pr["ms_per_step_min"] <= pr["ms_per_step_max"] <= line["ms_per_step"] * 1.001
    assert 0 < pr["gather_ms_per_step_min"] <= pr["gather_ms_per_step_max"] <= pr["ms_per_step_max"]


def test_bench_strong_scaling_form_launches_two_ranks():
    """`--workload eval --gpus N`: ONE 147 456-ray frame sharded by shard_bounds over the ranks + the (overlapped) pixel
    all-gather with uneven-shard counts -- the strong-scaling line of BASELINE.md section 4."""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--workload", "eval", "--standin"], capture_output=True, text=True, timeout=600, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    lines = _json_lines(p.stdout)
    assert len(lines) == 1, p.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and line["scaling"] == "strong" and line["config"]["rays_per_frame"] == 512 * 288
    assert line["value"] > 0 and "STAND-IN" in line["data"] and line["per_rank"]["gather_ms_per_step_max"] > 0


def test_bench_single_process_and_torchrun_forms():
    one = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "0", "--standin"],
                         capture_output=True, text=True, timeout=600, env=_env())
    assert one.returncode == 0, one.stderr[-2000:]
    assert len(_json_lines(one.stdout)) == 1 and _json_lines(one.stdout)[0]["n_gpus"] == 1
    tr = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                         "--master-addr", "127.0.0.1", "--master-port", "29655", os.path.join(ROOT, "bench.py"),
                         "--gpus", "2", "--steps", "2", "--warmup", "0", "--standin"],
                        capture_output=True, text=True, timeout=600, env=_env())
    assert tr.returncode == 0, tr.stderr[-2000:]
    lines = _json_lines(tr.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2
    # torchrun with ONE rank: the process group exists, so the step still ends with the (one-rank) collective
    tr1 = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                          "--master-addr", "127.0.0.1", "--master-port", "29656", os.path.join(ROOT, "bench.py"),
                          "--gpus", "1", "--steps", "2", "--warmup", "0", "--standin"],
                         capture_output=True, text=True, timeout=600, env=_env())
    assert tr1.returncode == 0, tr1.stderr[-2000:]
    lines = _json_lines(tr1.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 1 and lines[0]["per_rank"]["gather_ms_per_step_max"] > 0
    assert "per_rank" not in _json_lines(one.stdout)[0]          # plain `python bench.py`: no group, no collective


def test_bench_dumps_what_the_last_step_returned(tmp_path):
    """--dump-outputs DIR: one .npy per array the timed step returns (float32 here), the same in every run."""
    import numpy as np
    runs = []
    for d in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--standin",
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, env=_env())
        assert p.returncode == 0, p.stderr[-2000:]
        assert len(_json_lines(p.stdout)) == 1
        runs.append({f: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    assert sorted(runs[0]) == ["depth_fine.npy", "rgb_fine.npy"]
    for f, a in runs[0].items():
        assert a.dtype == np.float32 and a.shape[0] == 1024 and np.array_equal(a, runs[1][f])


def test_dump_keeps_a_fixed_sample_of_rows_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 20)
    out = {"train/loss": torch.tensor(0.5), "rows": [torch.randn(4096, 128).half(), torch.arange(4096, dtype=torch.float64)]}
    bench.dump_outputs(out, str(tmp_path / "a"))
    bench.dump_outputs(out, str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["rows.0.npy", "rows.1.npy", "train_loss.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert 0 < sum(a.nbytes for a in got.values()) <= 1 << 20
    assert got["rows.0.npy"].dtype == np.float32 and got["rows.1.npy"].dtype == np.float64 and got["train_loss.npy"] == 0.5
    assert all(np.array_equal(a, np.load(tmp_path / "b" / n)) for n, a in got.items())
    rows = got["rows.1.npy"].astype(np.int64)                  # the same rows of every array
    assert 0 < len(rows) < 4096 and np.array_equal(got["rows.0.npy"], out["rows"][0][rows].float().numpy())


def test_launcher_propagates_a_failing_rank():
    from nsff_pl_amd import dist as ndist
    code = "import os,sys,time; r=int(os.environ['RANK']); sys.exit(3) if r==1 else time.sleep(30)"
    rc = ndist.launch_local(2, [sys.executable, "-c", code], timeout=60)
    assert rc == 3
