"""bench.py's multi-rank launch contract on the CPU (gloo): `--gpus N` starts N ranks itself when
torchrun's environment is absent and reports n_gpus = N; a world size other than N exits non-zero
(--gpus was parsed and ignored)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1", **kw)
    return env


def _run(args, env):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                          env=env, capture_output=True, text=True, timeout=240)


def test_gpus_2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--plumbing", "--steps", "3", "--warmup", "1"], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2
    assert rec["config"]["parallelism"] == "dp2"
    assert rec["steps"] == 3 and rec["value"] > 0


def test_world_size_mismatch_exits_nonzero():
    r = _run(["--gpus", "2", "--plumbing", "--steps", "1", "--warmup", "0"],
             _env(WORLD_SIZE="3", RANK="0", LOCAL_RANK="0", MASTER_PORT="29533"))
    assert r.returncode != 0
    assert "WORLD_SIZE=3" in r.stderr


def test_gpus_1_runs_in_process():
    r = _run(["--gpus", "1", "--plumbing", "--steps", "2", "--warmup", "0"], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["n_gpus"] == 1


def _load_bench():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_cli", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per array; under the byte budget every array is whole,
    over it each long array keeps the same seeded sample of its elements on every call."""
    import numpy as np
    import torch

    bench = _load_bench()
    torch.manual_seed(0)
    model = torch.nn.Linear(7, 5)
    x = torch.randn(11, 7)
    pred = model(x)
    loss = pred.abs().sum()
    loss.backward()
    bench.dump_outputs(str(tmp_path / "a"), pred, loss, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad.bias.npy", "grad.weight.npy", "loss.npy", "param.bias.npy",
                     "param.weight.npy", "pred.npy"]
    got = {n: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["pred.npy"], pred.detach().numpy())
    assert np.array_equal(got["grad.weight.npy"], model.weight.grad.numpy())
    assert got["loss.npy"] == np.float32(loss.item())
    # a budget of 6 arrays x 4 elements: longer arrays are sampled, shorter ones stay whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 6 * 4 * 4)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), pred, loss, model)
    small = {n: np.load(tmp_path / "b" / n) for n in names}
    assert sum(a.nbytes for a in small.values()) <= 6 * 4 * 4
    assert small["pred.npy"].shape == (4,) and small["loss.npy"].shape == ()
    assert np.isin(small["pred.npy"], got["pred.npy"]).all()
    for n in names:
        assert np.array_equal(small[n], np.load(tmp_path / "c" / n))


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_outputs(tmp_path):
    """A plain run (no --full) on a small graph: --steps sets the timed steps, the line carries
    ms_per_step and none of the legs that need runs of their own, and --dump-outputs leaves the
    last step's arrays."""
    import numpy as np

    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "1", "--nodes", "500", "--edges",
              "6000", "--dump-outputs", str(out)], _env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["unit"] == "edges/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["config"]["value_is"] == "egnn"
    for leg in ("mace", "gvp", "tfn", "egnn_f32_exact"):
        assert leg not in rec
    assert rec["forward"] is None and rec["cpu_baseline"] is None
    names = sorted(os.listdir(out))
    assert "pred.npy" in names and "loss.npy" in names
    assert any(n.startswith("grad.") for n in names) and any(n.startswith("param.") for n in names)
    arrays = [np.load(out / n) for n in names]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays)
    assert sum(a.nbytes for a in arrays) <= 64 * 10 ** 6
