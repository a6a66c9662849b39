"""bench.py's output contract on a small shape: one JSON line with the fields the round driver
and the judge read (metric / value / unit / n_gpus / steps / warmup / ms_per_step /
higher_is_better / scaling / vs_baseline / dtype / data / config.workload, roofline{bound,
achieved, peak, unit, frac, traffic}, cpu_baseline{value, unit, cores, kind, sample}) and
internally consistent numbers; eager and hipGraph replay; the clock / power telemetry of the run."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--genes", "3000",
                          "--permutations", "1024", "--steps", "3", "--warmup", "1", "--full"] + extra,
                         capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                  # exactly ONE JSON line
    return json.loads(lines[0])


@pytest.mark.parametrize("extra", [["--cpu-seconds", "0.5"], ["--no-graph", "--no-cpu-baseline"],
                                   ["--kernel", "dense", "--no-cpu-baseline"]])
def test_bench_json_contract(extra):
    d = _run(extra)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "kernel_ms", "setup_ms"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["data"] == "synthetic" and d["scaling"] == "weak"
    assert d["scaling_strong"] is None                      # an overridden shape: only the default line carries it
    assert "workload" in d["config"] and "model" not in d["config"]
    G, T, P = d["config"]["genes_per_gpu"], d["config"]["traits"], d["config"]["permutations"]
    assert (G, P) == (3000, 1024)
    assert abs(d["value"] - G * T * P / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert d["value_incl_setup"] < d["value"] and d["ms_per_step_median"] > 0
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms"):
        assert k in r, k
    assert r["bound"] == "valu" and r["peak"] > 70
    # overridden shape: no committed PMC profile applies -> counters refused, not invented
    assert r["frac"] is None and r["achieved"] is None and "overridden" in r["counters_refused"]
    k3 = "k_permute" if "dense" in extra else "k_permute_lists"
    # the useful part of the issue (full-adder lane-ops from the list plan) needs no counters
    if "dense" in extra:
        assert r["useful_lane_ops"] is None and r["useful_frac"] is None
    else:
        assert r["useful_lane_ops"] > 0 and 0 < r["useful_frac_unpadded"] <= r["useful_frac"] < 1
        assert r["minority_entries_per_gene"] <= r["padded_entries_per_gene"] <= 1000 + 16
        # 2 * 31/32 lane-ops per padded entry and 32 permutations
        want = r["padded_entries_per_gene"] * 2 * 31 / 32 / 32
        assert abs(r["adder_ops_per_test"] - want) < 0.02 * want
        assert r["overhead_ops_per_test"] is None and r["measured_op_peak"] == 56.1
    # this run's shader clock / socket power (side-thread samples over the timed region)
    tel = d["telemetry"]
    for k in ("source", "samples", "sclk_mhz_mean", "socket_power_w_mean", "period_ms"):
        assert k in tel, k
    # (a box that exposes neither amdsmi nor the hwmon files yields nulls, never an error)
    for k in ("sclk_mhz_mean", "socket_power_w_mean", "ops_per_clock", "ops_per_clock_frac", "telemetry_samples"):
        assert k in r, k
    if tel["samples"]:
        assert 50 < tel["sclk_mhz_mean"] < 3000 and 20 < tel["socket_power_w_mean"] < 2000
        assert r["sclk_mhz_mean"] == tel["sclk_mhz_mean"]
    assert r["ops_per_clock"] is None                       # needs the counters: refused on an overridden shape
    assert len(d["kernel_source_sha256"]) == 64
    sus = d["sustained"]                                    # the box under ~2 s of sustained load, after the region
    if tel["source"] is None:                               # no sensor at all: nulls, and no sustained window
        assert sus is None and tel["samples"] == 0
    else:
        assert sus["steps"] > 0 and 1.5 < sus["seconds"] < 12 and sus["ms_per_step"] > 0
        if sus["samples"]:
            assert 50 < sus["sclk_mhz_mean"] < 3000 and 20 < sus["socket_power_w_mean"] < 2500
    # K1 / K2 carry their own roofline entries, timed by themselves
    k1, k2 = d["roofline_k1"], d["roofline_k2"]
    for k in ("kernel", "bound", "bytes", "kernel_ms", "gbs", "hbm_frac", "valu_frac", "hbm_floor_ms", "valu_floor_ms",
              "frac_of_bound", "traffic", "passes_over_matrix", "vectors"):
        assert k in k1, k
    N, W64 = d["config"]["isolates"], -(-d["config"]["isolates"] // 64)
    assert k1["kernel"] == "k_counts" and k1["bound"] in ("hbm", "valu") and k1["passes_over_matrix"] == 1
    assert k1["bytes"] == 8 * W64 * G + 16 * W64 * T + 16 * G * T          # B1
    assert 0 < k1["hbm_frac"] < 1 and 0 < k1["frac_of_bound"] <= 1.05 and k1["vectors"] >= T + 1
    assert abs(k1["kernel_ms"] - d["kernel_ms_isolated"]["k_counts"]) < 1e-12
    # ... and K1 as an HBM stream (round 5): a working set the Infinity Cache cannot hold, in rotation
    cold = k1["cold"]
    assert cold["hbm_peak_gbs"] == 8000.0 and cold["measured_copy_peak_gbs"] > 500
    assert [run["traits"] for run in cold["runs"]] == [1, 2, 4, 8, 16, 32, 50]
    assert [run["passes_over_matrix"] for run in cold["runs"]] == [1, 1, 1, 1, 1, 1, 2]
    assert cold["runs"][0]["bound"] == "hbm" and cold["runs"][-1]["bound"] == "valu" and "T = " in cold["crossover"]
    for run in cold["runs"]:
        assert run["bytes"] == 8 * 157 * 125_000 + 16 * 157 * run["traits"] + 16 * 125_000 * run["traits"]
        assert 0 < run["hbm_frac"] < 1 and run["launches"] == 24 and run["cold_ms_median"] >= run["warm_ms_median"] * 0.8
        assert 0 < run["frac_of_bound"] <= 1.05
        assert abs(run["gbs"] - run["bytes"] / run["cold_ms_median"] / 1e6) < 1e-6 * run["gbs"]
    assert "cache-resident" in k1["note"]
    # the label generator timed by itself (inside a step it shares the chip with k_fisher)
    if "dense" not in extra:
        assert 0 < d["kernel_ms_isolated"]["k_perm_generate_tiles"] < 1.0
    assert k2["kernel"] == "k_fisher" and k2["tables"] == G * T and k2["bytes"] == 32 * G * T
    assert k2["tables_per_s"] > 1e6 and 0 < k2["hbm_frac"] < 1
    assert r["kernel"] == k3 and d["kernel_ms"][k3] > 0
    assert sum(d["kernel_ms"].values()) < 3 * d["ms_per_step"]
    # 3000 x 10 x 1024 = 3e7 tests per step: launch-bound, so the step is replayed as a hipGraph by
    # default (AssociationEngine.auto_graph_eligible) unless --no-graph asks for eager launches
    assert d["config"]["hip_graph"] == ("--no-graph" not in extra)
    assert d["config"]["hip_graph_auto"] == ("--no-graph" not in extra)
    if "--no-cpu-baseline" not in extra:
        for name in ("cpu_baseline", "cpu_baseline_port"):
            c = d[name]
            for k in ("value", "unit", "cores", "kind", "sample"):
                assert k in c, (name, k)
        assert d["cpu_baseline"]["kind"] == "scipy-restatement" and d["cpu_baseline"]["matches_gpu"] is True
        assert d["cpu_baseline_port"]["kind"] == "port"
        assert d["cpu_baseline"]["value"] < d["cpu_baseline_port"]["value"] < d["value"]


def test_bench_headline_line_explains_itself():
    """The default command line (cfg3, the BASELINE headline shape; fewer steps): the roofline
    object carries the shader clock and socket power of THIS run and lane-ops per clock, so a
    reader can tell a slow box from a slow kernel, next to K1 / K2's
    own roofline entries (item 4)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "20", "--warmup", "3",
                          "--no-cpu-baseline", "--full"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    r, tel = d["roofline"], d["telemetry"]
    assert "cfg3" in d["config"]["workload"] and d["config"]["permutations"] == 10_000
    # the strong curve's entries ride along (at one GPU: the denominators) -- cfg3 is the line itself,
    # cfg4 (200 000 variants x 5000 isolates, one trait) is timed the same way
    ss = d["scaling_strong"]
    assert ss["cfg3"]["n_gpus"] == 1 and abs(ss["cfg3"]["value"] - d["value"]) < 1e-6 * d["value"]
    c4 = ss["cfg4"]
    for k in ("workload", "n_gpus", "value", "unit", "ms_per_step", "steps", "warmup", "genes_per_gpu",
              "gene_partition", "gene_order", "hip_graph", "kernel_ms", "exchange_exposed_ms", "rccl_ranks", "per_rank"):
        assert k in c4, k
    assert c4["n_gpus"] == 1 and c4["genes_per_gpu"] == [200_000] and c4["per_rank"] is None
    assert abs(c4["value"] - 200_000 * 10_000 / (c4["ms_per_step"] * 1e-3)) < 1e-6 * c4["value"]
    assert c4["value"] > 1e11 and c4["kernel_ms"]["k_permute_lists"] > 0
    # short forms inside the objects the driver's record keeps whole
    assert d["config"]["scaling_strong"]["cfg4"]["value"] == c4["value"]
    assert d["config"]["scaling_strong"]["cfg3"]["n_gpus"] == 1
    assert (d["roofline"]["sustained"] is None) == (d["sustained"] is None)
    if d["sustained"] is not None:
        assert d["roofline"]["sustained"]["value"] == d["sustained"]["value"]
    if tel["source"] is None:
        pytest.skip("this box exposes no clock / power source (amdsmi, hwmon): nothing to check")
    assert tel["samples"] >= 10                              # >= 10 samples inside the timed region
    assert 50 < tel["sclk_mhz_mean"] <= 3000 and 20 < tel["socket_power_w_mean"] < 2500
    sus = d["sustained"]
    assert sus["samples"] >= 20 and 50 < sus["sclk_mhz_mean"] <= 3000 and 20 < sus["socket_power_w_mean"] < 2500
    assert abs(sus["ms_per_step"] / d["ms_per_step"] - 1) < 0.25         # the same step, back to back
    if r["frac"] is not None:                                # counters of this kernel version are on file
        assert sus["ops_per_clock_frac"] > 0
        assert 0 < r["ops_per_clock"] < 32768 and abs(r["ops_per_clock_frac"] - r["ops_per_clock"] / 32768) < 1e-12
        # frac is taken against 2.4 GHz, ops_per_clock against the clock the box granted
        assert abs(r["frac"] * 2400.0 / tel["sclk_mhz_mean"] - r["ops_per_clock_frac"]) < 1e-9


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times the steps and prints the headline only; --dump-outputs writes what the
    last timed step returned, and two runs with the same arguments write the same arrays."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dumps = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--genes", "3000", "--permutations",
                              "1024", "--steps", "4", "--warmup", "1", "--dump-outputs", str(tmp_path / run)],
                             capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        assert d["steps"] == 4 and d["higher_is_better"] is True and d["unit"] == "tests/s"
        G, T, P = d["config"]["genes_per_gpu"], d["config"]["traits"], d["config"]["permutations"]
        assert abs(d["value"] - G * T * P / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
        for k in ("roofline", "kernel_ms", "telemetry", "sustained", "cpu_baseline", "roofline_k1"):
            assert k not in d, k
        assert d["scaling_strong"] is None
        dumps.append({f[:-4]: np.load(tmp_path / run / f) for f in os.listdir(tmp_path / run)})
    a, b = dumps
    names = ["counts", "crit", "margins", "odds", "p", "r"]
    assert sorted(k for k in a if not k.endswith("_nonfinite")) == names
    assert a["counts"].shape == (T, G, 4) and a["p"].shape == a["r"].shape == (T, G)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in a.values())
    # non-finite entries (odds of a table with an empty cell) are coded beside their array, not lost
    for k in a:
        if k.endswith("_nonfinite"):
            base = k[:-len("_nonfinite")]
            assert base in names and a[k].shape == a[base].shape and set(np.unique(a[k])) <= {0, 1, 2, 3}
            assert (a[base][a[k] != 0] == 0).all()
    # every table of a trait holds its valid isolates (margins: positives, valid); r counts of P permutations
    assert np.array_equal(a["counts"].sum(axis=2), np.broadcast_to(a["margins"][:, 1:2], (T, G)))
    assert a["r"].min() >= 0 and a["r"].max() <= P
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
