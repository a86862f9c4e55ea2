"""The driver's own command, `python bench.py --steps 20 --warmup 5`, end to end in a child
process: one JSON line with the contract's fields and the roofline tied to the library that ran;
with --full also the direct-form figure, the other walks and the CPU baseline beside it; with
--dump-outputs the state the timed walk ends in, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
            "scaling", "vs_baseline", "dtype", "data", "config", "roofline")
BESIDE = ("value_direct_form", "direct_form", "value_piecewise", "piecewise", "value_early_reject",
          "early_reject", "small_batches", "cpu_baseline")


def run_bench(*extra):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MHX_SPLIT", "MHX_TSPLIT"):
        env.pop(k, None)
    env["MHX_BENCH_CPU_THREADS"] = "4"  # (a short CPU leg: the figure itself is not asserted)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "5",
                          *extra], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in CONTRACT:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["dtype"] == "f64"
    assert d["unit"] == "chain-steps/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["config"]["chains_per_gpu"] == 4096 and d["config"]["n_points"] == 100000
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / 4096 - 1.0) < 1e-9
    r = d["roofline"]
    assert r["bound"] == "fp64_valu_issue" and r["unit"] == "G wave-instr/s" and 0.3 < r["frac"] <= 1.0 and r["instr_source_stale"] is False
    assert r["kernel_ms_per_launch"] * 1e-3 <= d["ms_per_step"] * 1e-3 * 20 * 1.001
    assert d["build"]["id"].startswith("csrc:")
    return d


def test_bench_line_at_the_drivers_arguments():
    d = run_bench("--full")
    assert "cpu_baseline" in d
    assert d["value_direct_form"] > 0 and d["direct_form"]["ratio_to_value"] > 1.0
    er = d["early_reject"]   # (a walk's iterations 6-25 accept nothing: every sweep is left early)
    assert "+early-reject" in er["kernel"] and d["value_early_reject"] > 1.5 * d["value"], er
    sb = d["small_batches"]
    for k in ("walkers_1", "walkers_64"):   # (one persistent launch per portion: well under the 16-20 us of two launches)
        assert "persistent tsplit" in sb[k]["kernel"] and 0 < sb[k]["us_per_iteration"] < 14 and not sb[k]["trapped"], sb
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and c["single_core"]["value"] > 0
    assert d["value"] > 1e3 * c["value"]


def test_plain_bench_line_and_its_outputs(tmp_path):
    """a plain run times the headline walk only, and --dump-outputs writes the state it ends in:
    the same arrays, bit for bit, from two runs of the same command"""
    dumps = []
    for i in range(2):
        out_dir = tmp_path / ("run%d" % i)
        d = run_bench("--dump-outputs", str(out_dir))
        for k in BESIDE:
            assert k not in d, k
        names = d["outputs"]["names"]
        assert set(names) >= {"theta", "logpost", "best_theta", "best_logpost", "length", "age", "lmatrix",
                              "temperature"}
        assert sorted(p.name for p in out_dir.iterdir()) == sorted(n + ".npy" for n in names)
        dumps.append({n: np.load(out_dir / (n + ".npy")) for n in names})
    a, b = dumps
    assert a["theta"].shape == (4096, 8) and a["lmatrix"].shape == (4096, 8, 8)
    assert sum(x.nbytes for x in a.values()) < 64e6
    for n in a:
        assert a[n].dtype == np.float64, n
        assert np.array_equal(a[n], b[n]), n
    assert np.isfinite(a["logpost"]).all() and np.isfinite(a["theta"]).all()
