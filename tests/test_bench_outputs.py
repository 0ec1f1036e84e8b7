"""bench.py's plain run and `--dump-outputs`: `--steps` is the number of timed steps and `ms_per_step` the time of one, the line
holds none of the secondary legs that `--full` adds, and the dump is float32 / float64 .npy files within 64 MB that come out the
same when the same command runs twice: the replayed step starts from the same state in every run, so what remains is the
rounding of the backward's atomic sums, and the timed steps' own run-to-run drift does not reach the dump.  The replayed update
must have been applied: every sampled weight moved by at most lr from its initial value, and most of them moved."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "grad_rel_err", "trajectory", "fast_mode_bf16", "with_h2d_uint8", "dp_policy_at_world_size_1", "comm",
             "cpu_baseline")


def _bench(args, timeout=600):
    return subprocess.run([sys.executable, "bench.py"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_refuses_a_step_count_it_cannot_time(bad):
    r = _bench(["--gpus", "1"] + bad, timeout=300)
    assert r.returncode != 0
    assert "--steps must be >= 1" in r.stderr, r.stderr[-2000:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    runs = []
    for i, (steps, warmup) in enumerate([(3, 1), (6, 2)]):      # the dump must not depend on the steps before it
        d = tmp_path / f"run{i}"
        r = _bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--batch", "4", "--dump-outputs", str(d)])
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == steps and line["warmup"] == warmup and line["unit"] == "clip-pairs/s" and line["higher_is_better"] is True
        assert line["metric"] and line["dtype"] and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(4 * 1e3 / line["ms_per_step"], rel=1e-2)
        assert not [k for k in FULL_ONLY if k in line], sorted(line)
        files = sorted(os.listdir(d))
        assert files == ["grad_norms.npy", "loss.npy", "params_sample.npy"], files
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
        assert arrs["params_sample"].size > 10 ** 6 and np.isfinite(arrs["params_sample"]).all() and np.isfinite(arrs["loss"]).all()
        runs.append(arrs)
    a, b = runs
    sys.path.insert(0, ROOT)
    import bench
    bench.dump_outputs(str(tmp_path / "initial"), bench.build_model("base_patch16_224", 16), 0.0)   # the weights before any step
    p0 = np.load(tmp_path / "initial" / "params_sample.npy").astype(np.float64)
    moved = np.abs(a["params_sample"].astype(np.float64) - p0)
    bound = 3e-5 + 2 * 2.0 ** -23 * np.abs(p0)          # lr, plus the fp32 rounding of the updated weight (two ulps)
    assert np.all(moved <= bound) and (moved > 0).mean() > 0.5, (np.max(moved - bound), (moved > 0).mean())
    ga, gb = a["grad_norms"], b["grad_norms"]
    assert ga.dtype == np.float64 and np.isfinite(ga).all() and (ga > 0).mean() > 0.9
    assert np.all(np.abs(ga - gb) <= 1e-3 * gb), np.max(np.abs(ga - gb) / np.maximum(gb, 1e-30))
    assert float(a["loss"][0]) == pytest.approx(float(b["loss"][0]), rel=1e-6)      # the forward's one atomic sum: the loss over rows
    # one AdamW step moves a weight by at most lr (3e-5); only an element whose gradient lies within the atomics' rounding of zero
    # can move in opposite directions in the two runs
    pa, pb = a["params_sample"].astype(np.float64), b["params_sample"].astype(np.float64)
    assert np.abs(pa - pb).max() <= 2 * 3e-5 + 1e-6
    assert np.linalg.norm(pa - pb) <= 1e-5 * np.linalg.norm(pb)
