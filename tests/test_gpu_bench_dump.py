"""bench.py --dump-outputs on the HIP path: after exactly --steps timed rounds the stream's state is written as float64 arrays, one
row per system in global order, and two runs with the same arguments write the same bits (what lets two builds be compared
output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(d, steps, extra=("--no-cpu-baseline", "--no-extras")):
    env = dict(os.environ, IDAHIP_GEN_PROCS="1")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--n", "64", "--batch", "64", "--groups", "2", "--steps", str(steps),
                          "--warmup", "1"] + list(extra) + ["--dump-outputs", d], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_is_the_stream_state_and_repeats_bit_for_bit(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    line = run_bench(a, 3)
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["newton_iters_timed"] > 0
    assert line["dump_outputs"]["systems"] == line["dump_outputs"]["total_systems"] == 64
    got = load(a)
    assert sum(x.nbytes for x in got.values()) == line["dump_outputs"]["bytes"] <= 64 * 1000 * 1000
    assert all(x.dtype == np.float64 and x.shape[0] == 64 for x in got.values())
    assert np.array_equal(got["system"], np.arange(64)) and got["yy"].shape == got["yp"].shape == (64, 64)
    assert np.isfinite(got["yy"]).all() and np.isfinite(got["yp"]).all()
    assert (got["tn"] >= 0.0).all() and (got["nni"] > 0).any()
    run_bench(b, 3)
    again = load(b)
    assert sorted(again) == sorted(got)
    for k in got:
        assert np.array_equal(again[k].view(np.uint64), got[k].view(np.uint64)), k


def test_full_run_dumps_the_same_state_and_adds_what_a_plain_run_leaves_out(tmp_path):
    """--full measures and checks everything else after the same timed steps: the kernels' own figures (on one more context with
    all of the rank's systems), the verification pass, the whole passes, the CPU baseline, the stream-share probe. The stream it
    dumps is the plain run's, bit for bit, and the plain line carries none of those figures."""
    a, b = str(tmp_path / "plain"), str(tmp_path / "full")
    plain = run_bench(a, 3, extra=())
    full = run_bench(b, 3, extra=("--full",))
    moved = ("kernel_classes_rank0", "lu_kernels_rank0", "kernel_figures_measured_on", "roofline", "lu_plus_solve", "hbm_roofline",
             "ensemble_result", "cpu_baseline", "whole_pass", "device_controller", "newton_fusion", "reference_text_paths")
    assert plain["full"] is False and not set(moved) & set(plain) and "least_pairwise_stream_share" not in plain["config"]
    assert full["full"] is True and set(moved) <= set(full) and "least_pairwise_stream_share" in full["config"]
    for line in (plain, full):
        assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert full["newton_iters_timed"] == plain["newton_iters_timed"]
    cls = full["kernel_classes_rank0"]
    assert cls["newton_iter"]["systems"] > 0 and cls["lu"]["systems"] > 0 and full["lu_kernels_rank0"]["lu_panel"]["launches"] > 0
    assert "ONE ensemble of all 64 systems" in full["kernel_figures_measured_on"]
    assert full["ensemble_result"]["systems"] == 64 and full["ensemble_result"]["sum_nni"] > 0
    assert full["whole_pass"]["value"] > 0 and len(full["whole_pass"]["passes"]) == 10
    assert full["cpu_baseline"]["value"] > 0 and full["device_controller"]["whole_pass_value_with_the_host_stepper"] > 0
    got, again = load(a), load(b)
    assert sorted(again) == sorted(got)
    for k in got:
        assert np.array_equal(again[k].view(np.uint64), got[k].view(np.uint64)), k
