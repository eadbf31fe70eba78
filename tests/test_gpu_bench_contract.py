"""GPU: `python bench.py --full` (two steps) prints exactly ONE line of JSON on stdout and that line keeps the contract:
the metric and configuration BASELINE.json names, the roofline object of the dominant kernel (algorithmic bytes per launch over its
HIP-event duration against 8 TB/s), the CPU baseline timed in the same run, the host-side legs as medians, and the rest of BASELINE's
matrix as config.secondary - every workload's results checked inside bench.py itself before it prints anything."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_the_default_bench_line_keeps_the_contract():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--full", "--cpu-sample", "2048", "--host-reps", "2"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines[:3]
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] in base["metric"] or "presentations verified/sec" in d["metric"]
    assert d["unit"] == "presentations/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "int64" and "synthetic" in d["data"]
    assert abs(d["value"] - (1 << 20) / (d["ms_per_step"] / 1e3)) < 1e-6 * d["value"]           # value = items per step / time per step
    c = d["config"]
    assert c["workload"].startswith("C3: batch verify 2^20 presentations") and "model" not in c and c["presentations_per_gpu"] == 1 << 20
    assert c["algorithmic_bytes_per_presentation"] == 2425
    ro = d["roofline"]
    assert ro["bound"] == "hbm" and ro["unit"] == "GB/s" and ro["peak"] == 8000.0 and ro["kernel"] == "k_msm_window"
    assert abs(ro["frac"] - ro["achieved"] / ro["peak"]) < 1e-12
    assert abs(ro["achieved"] - 2425 * ro["items_per_launch"] / (ro["avg_launch_ms"] / 1e3) / 1e9) < 1e-6 * ro["achieved"]
    assert ro["items_per_launch"] == 1 << 19 and 2 * ro["avg_launch_ms"] <= d["ms_per_step"]     # two launches of the dominant kernel fit in a step
    assert ro["traffic"] is None or ro["traffic"] > ro["algorithmic_bytes_per_launch"]           # (None while the committed PMC passes are of other kernel sources)
    assert sum(ro["kernels_ms_per_step"].values()) <= d["ms_per_step"] * 1.001
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["unit"] == "presentations/s" and cpu["cores"] >= 1 and cpu["value"] > 0
    assert cpu["items"] == 2048 and str(cpu["items"]) in cpu["sample"] and str(cpu["single_thread_items"]) in cpu["sample"] and cpu["single_thread_value"] > 0
    assert d["value"] > 20 * cpu["value"]
    for leg in ("host_pointer_api_spread", "wire_blob_api_spread", "group_api_spread"):
        s = c[leg]
        assert s["reps"] == 2 and s["min"] <= s["median"] <= s["max"] <= d["value"] * 1.02, (leg, s)
    assert 0.85 < c["host_pointer_api_over_value"] < 1.02
    sec = c["secondary"]
    assert "error" not in sec, sec.get("error")
    for k, unit in (("c2", "presentations/s"), ("c5", "credentials/s"), ("c5_fast", "credentials/s"), ("show", "presentations/s"), ("show_fast", "presentations/s")):
        w = sec[k]
        assert w["unit"] == unit and w["value"] > 1e6 and w["roofline"]["bound"] == "hbm" and 0 < w["roofline"]["frac"] < 0.05, (k, w)
    assert "C5: batch issue 2^20 credentials, 16 attributes" in sec["c5"]["workload"] and sec["c5"]["algorithmic_bytes_per_item"] == 1488
    assert sec["c5"]["secret_terms_in_plan"] > 0 and sec["c5_fast"]["secret_terms_in_plan"] == 0 and sec["c5_fast"]["value"] > sec["c5"]["value"]


def test_a_plain_bench_run_times_the_headline_only_and_dumps_its_outputs(tmp_path):
    """the command run for every change (`--gpus 1 --steps N --warmup W`): the headline's line, its timed steps and nothing beside them;
    --dump-outputs writes the status bytes of the last step, the same ones in two runs of the same arguments"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    got = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines[:3]
        d = json.loads(lines[0])
        assert d["metric"] == "credential presentations verified/sec" and d["unit"] == "presentations/s" and d["higher_is_better"] is True
        assert d["dtype"] == "int64" and d["steps"] == 3 and d["warmup"] == 1
        assert abs(d["value"] - (1 << 20) / (d["ms_per_step"] / 1e3)) < 1e-6 * d["value"]
        assert d["roofline"]["kernel"] == "k_msm_window" and sum(d["roofline"]["kernels_ms_per_step"].values()) <= d["ms_per_step"] * 1.001
        c = d["config"]
        assert c["full"] is False and d["cpu_baseline"] is None and c["secondary"] is None
        assert c["host_pointer_api_spread"] is None and c["wire_blob_api_spread"] is None and c["group_api_spread"] is None
        assert sorted(os.listdir(tmp_path / run)) == ["status.npy"]
        st = np.load(tmp_path / run / "status.npy")
        assert st.dtype == np.float32 and st.shape == (1 << 20,) and set(np.unique(st).tolist()) == {0.0, 1.0}
        assert int(st.sum()) == (1 << 20) // 100    # the 1 % bench.corrupt damaged, and only those
        got.append(st)
    assert np.array_equal(got[0], got[1])
