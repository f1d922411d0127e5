"""``python bench.py --gpus N`` must launch its own ranks (the driver calls it exactly like that
when it is not already under torchrun).  Rehearsed here on CPU: same launch path
(child ``python -m torch.distributed.run``), real collectives over gloo, NumPy test double for the
kernels; the JSON line of rank 0 is relayed and the exit code is the child's.  A plain run (no ``--full``) is the
headline alone, and ``--dump-outputs`` writes what its timed loop computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*extra, full_json):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    # (the complete record goes to the test's own directory: the default path is where a real run's record lives)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *extra, "--full-json", str(full_json)],
                          capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)


def test_bench_launches_its_own_ranks_over_gloo(tmp_path):
    p = _run("--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "gloo", "--full",
             "--workload", "er:96:0.06", full_json=tmp_path / "full.json")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1                       # rank 0's line, relayed once
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks"] == 2 and out["steps"] == 2
    assert out["metric"] == "simrank_iterations_per_sec" and out["value"] > 0
    assert out["scaling"] == "strong" and "NOT a measurement" in out["data"]
    # the one command for an 8-GPU node carries every key of the sharded runs (here: named, and marked as not run)
    assert out["headline_loop"].startswith("tests/pydriver.Solver") and out["python_driver"]["value"] == out["value"]
    c = out["sharded_c_loop"]
    assert c["ranks"] == 2 and set(c["variants"]) == {"f32_full_form", "f32_half_form", "f32_half_form_fp16_wire",
                                                      "fp16_held_full_form"}
    assert all("skipped" in v and "value" not in v for v in c["variants"].values())
    assert [v["parity_grade"] for v in c["variants"].values()] == [True, True, False, False]
    assert "skipped" in c["config5"] and "skipped" in c["config3"] and "skipped" in c["form_measured"]
    assert "skipped" in c["link_probe"]          # (the xGMI link-rate probe of a real multi-GPU run)
    assert len(lines[0]) <= 8000                 # the driver's record keeps the tail of the line: it must be all of it
    assert "exchange_ms" in out
    assert abs(json.load(open(tmp_path / "full.json"))["value"] - out["value"]) < 1e-3 * out["value"]   # the complete record


def test_bench_child_failure_is_reported(tmp_path):
    p = _run("--gpus", "2", "--backend", "gloo", "--workload", "no-such-workload", full_json=tmp_path / "full.json")
    assert p.returncode != 0


def _dump_run(tmp_path, tag, *extra):
    out_dir = tmp_path / tag
    p = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "er:96:0.06", "--dump-outputs", str(out_dir),
             *extra, full_json=tmp_path / f"{tag}_full.json")
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0]), out_dir


def _check_dump(out, out_dir, tmp_path, tag):
    from oracle import simrank_oracle as O
    from simrank_amd import synth
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert abs(out["ms_per_step"] * out["value"] - 1e3) < 1e-4 * 1e3          # (the line keeps five significant digits)
    # a plain run is the headline alone: nothing measured or checked beside it, no complete record written
    for k in ("converge", "convergence_test", "cpu_baseline", "secondary", "bipartite_pp", "config5", "fit_wall"):
        assert k not in out, k
    assert not (tmp_path / f"{tag}_full.json").exists()
    files = sorted(os.listdir(out_dir))
    assert files == ["S_rows.npy", "changed.npy"]
    assert sum(os.path.getsize(out_dir / f) for f in files) <= 64 << 20
    S, changed = np.load(out_dir / "S_rows.npy"), np.load(out_dir / "changed.npy")
    assert S.dtype == np.float32 and changed.dtype == np.float64 and changed.shape == (1,)
    # what the timed loop computed: warm-up + timed updates from the identity (all 96 rows fit: the whole of S)
    want = O.fit_simrank(synth.er_directed(96, 0.06, 96), verbose=False, iterations=4, eps=1e-30)
    assert S.shape == want["S"].shape
    np.testing.assert_allclose(S, want["S"], rtol=1e-5, atol=1e-30)
    return S, changed


def test_bench_plain_run_dumps_outputs_over_gloo(tmp_path):
    """The plain line of one process on the NumPy test double, and its outputs: the same in two runs."""
    out, d1 = _dump_run(tmp_path, "a", "--backend", "gloo")
    S1, c1 = _check_dump(out, d1, tmp_path, "a")
    out, d2 = _dump_run(tmp_path, "b", "--backend", "gloo")
    S2, c2 = _check_dump(out, d2, tmp_path, "b")
    assert np.array_equal(S1, S2) and np.array_equal(c1, c2)


def test_bench_dump_outputs_needs_one_process(tmp_path):
    p = _run("--gpus", "2", "--backend", "gloo", "--dump-outputs", str(tmp_path / "d"), full_json=tmp_path / "full.json")
    assert p.returncode != 0 and "--dump-outputs" in p.stderr


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(tmp_path):
    """The same on the GPU: the HIP loop timed, then its S and last count written."""
    out, d = _dump_run(tmp_path, "gpu")
    _check_dump(out, d, tmp_path, "gpu")
