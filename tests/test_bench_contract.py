"""Driver-contract guard: bench.py must print ONE JSON line with the
agreed fields (BASELINE.json metric, whole-job value; strong scaling —
the 8-client protocol is fixed at every GPU count)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = ["--samples-per-client", "64", "--batch-size", "32"]


def run_bench(*extra):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), *extra, *SMALL],
        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_json_contract():
    # --full: the accuracy and soak fields asserted below are computed
    # only there
    d = run_bench("--steps", "1", "--warmup", "0", "--full")
    assert d["metric"] == "fl_round_wall_clock_ms"
    assert d["unit"] == "ms/round"
    assert d["higher_is_better"] is False
    assert d["scaling"] == "strong"
    # the fixed protocol shape (VERDICT round-1 item 1): the committee
    # machinery must be inside the timed region at EVERY gpu count
    assert d["config"]["clients"] == 8
    assert d["config"]["committee"] == 4
    assert d["config"]["update_quota"] == 4
    assert d["config"]["aggregate_top_k"] == 3
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0
    assert d["value"] == d["ms_per_step"] > 0
    assert d["dtype"] in ("bf16", "fp32")
    assert d["data"] == "synthetic"
    assert d["full"] is True
    assert 0.0 <= d["test_acc"] <= 1.0
    # untimed convergence-soak fields are always present; on CPU the
    # soak is skipped (GPU femnist runs default to 1500 rounds)
    if d["dtype"] == "fp32":
        assert d["soak_rounds"] == 0 and d["soak_test_acc"] is None
    else:
        assert d["soak_rounds"] == 1500
        assert 0.0 <= d["soak_test_acc"] <= 1.0
    cfg = d["config"]
    for key in ("model", "global_batch", "parallelism", "clients",
                "committee", "update_quota", "aggregate_top_k",
                "batch_size", "partition"):
        assert key in cfg, key


def test_plain_run_is_lean_and_dumps_reproducible_outputs(tmp_path):
    """A plain run keeps the headline fields, leaves the --full extras
    null, really runs --steps timed rounds, and --dump-outputs writes
    the last timed round's results — identical from run to run."""
    dumps = []
    for name in ("a", "b"):
        d = run_bench("--gpus", "1", "--steps", "2", "--warmup", "1",
                      "--dump-outputs", str(tmp_path / name))
        assert d["metric"] == "fl_round_wall_clock_ms"
        assert d["unit"] == "ms/round"
        assert d["higher_is_better"] is False
        assert d["dtype"] in ("bf16", "fp32")
        assert d["value"] == d["ms_per_step"] > 0
        assert d["steps"] == 2 and d["warmup"] == 1
        assert d["fl_epoch"] == 3  # warmup + steps rounds, nothing else
        assert d["full"] is False
        assert d["test_acc"] is None
        assert d["soak_rounds"] == 0 and d["soak_test_acc"] is None
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["global_model.npy", "round_stats.npy",
                         "selected.npy"]
        arrs = {f: np.load(tmp_path / name / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64)
                   for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64e6
        dumps.append(arrs)
    a, b = dumps
    assert a["global_model.npy"].ndim == 1
    assert np.isfinite(a["global_model.npy"]).all()
    assert np.abs(a["global_model.npy"]).max() > 0
    # [epoch, global_loss, n_updates, n_selected, samples_trained] of
    # the last timed round: epoch 2, quota 4 admitted, top-3 selected
    assert a["round_stats.npy"][0] == 2
    assert a["round_stats.npy"][2] == 4 and a["round_stats.npy"][3] == 3
    assert a["selected.npy"].shape == (3, 2)
    # the model and the committee's choice repeat bit for bit (fixed
    # accumulation order). The reported loss is an fp32 atomicAdd sum of
    # per-row losses (csrc/hip/softmax_ce.hip) whose order is not fixed
    # on a GPU: reordering N non-negative terms moves the sum by at most
    # N * 2^-24 relative; a client here sums 64 rows, and 1e-4 still
    # bounds N up to ~1600.
    assert np.array_equal(a["global_model.npy"], b["global_model.npy"])
    assert np.array_equal(a["selected.npy"], b["selected.npy"])
    assert np.array_equal(a["round_stats.npy"][[0, 2, 3, 4]],
                          b["round_stats.npy"][[0, 2, 3, 4]])
    assert np.allclose(a["round_stats.npy"][1], b["round_stats.npy"][1],
                       rtol=1e-4, atol=0.0)


def test_soak_needs_full():
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--soak", "5"],
        capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode != 0
    assert "--full" in out.stderr
