"""The line bench.py prints, end to end on the GPU (a short run): exactly one JSON line on stdout with the contract's fields,
`roofline` with measured traffic, `cpu_baseline` with both legs (--full); a plain run's line and the outputs it dumps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


LINE_LIMIT = 6000      # bench.py's LINE_LIMIT: the driver keeps the last 8 KB of stdout (round 5's 25 KB line was lost)


def _bench(*args, env=None, detail=False, tmp=None):
    """Runs bench.py; returns the parsed stdout line (and, with detail=True, the full record it wrote beside it)."""
    import tempfile
    dpath = os.path.join(tmp or tempfile.mkdtemp(prefix="vbx_bench_"), "bench_detail.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--detail", dpath], capture_output=True, text=True,
                       timeout=900, env=None if env is None else dict(os.environ, **env))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    assert len(p.stdout) < LINE_LIMIT, len(p.stdout)
    line = json.loads(lines[0])
    if not detail:
        return line
    with open(dpath) as f:
        return line, json.load(f)


def test_default_workload_line():
    d, full = _bench("--full", "--hours", "0.25", "--steps", "2", "--warmup", "1", "--cpu-seconds", "4", detail=True)
    assert d["value"] == pytest.approx(full["value"], rel=1e-5) and d["roofline"]["frac"] == pytest.approx(full["roofline"]["frac"], rel=1e-5)
    assert set(d["sub_benchmarks"]) == {s["name"] for s in full["sub_benchmarks"]}
    assert all(not (isinstance(v, dict) and "error" in v) for v in d["sub_benchmarks"].values()), d["sub_benchmarks"]
    assert d["sub_benchmarks"]["config2"] == pytest.approx(next(s for s in full["sub_benchmarks"] if s["name"] == "config2")["value"], rel=1e-5)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "frames/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and d["config"]["frame_len"] == 1200 and d["config"]["hop"] == 480
    assert d["value"] > 1e6
    r = d["roofline"]
    assert r["bound"] in ("hbm", "fp64_valu") and r["kernel"] == "analyze" and 0.0 < r["frac"] < 1.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5 * r["frac"]      # (the line carries six significant digits)
    assert r["traffic"] is not None and r["traffic"] > 0.9 * 4064 * d["config"]["frames_per_gpu"]     # at least the algorithmic bytes
    # round 6: the traffic is MEASURED IN THE RUN (two rocprofv3 --pmc child passes), agrees with the committed evidence file's
    # figure within 5 %, and stays below 1.3x the algorithmic bytes
    assert r["traffic_source"].startswith("measured in this run") and "live_traffic_error" not in d, (r["traffic_source"], d.get("live_traffic_error"))
    live, committed = full["roofline"]["traffic_source"]["bytes_per_frame"], full["roofline"]["traffic_committed_evidence"]["bytes_per_frame"]
    assert abs(live - committed) <= 0.05 * committed and 4064 <= live <= 1.3 * 4064, (live, committed)
    # ... and so are the vector ALU's busy share and the kernel's vector instructions per frame (an SQ child pass)
    assert full["roofline"]["issue_frac_source"].startswith("live") and 9000 < r["valu_insts_per_frame"] < 13000
    assert abs(r["issue_frac"] - full["roofline"]["issue_frac_committed_evidence"]) < 0.05
    # the headline fraction is the EXECUTED one (FFTs + evaluated sinc terms); the comparison with the reference's O(N^2) sums has its own key
    assert r["frac"] < 0.5 and r["reference_sums_at_peak_ratio"] > r["frac"] and 0.3 < r["issue_frac"] <= 1.0
    assert full["roofline"]["reference_sums_at_peak"]["ratio"] == pytest.approx(r["reference_sums_at_peak_ratio"], rel=1e-5)
    assert d["config"]["rccl_comms_per_rank"] == 0 and d["config"]["torch_nccl_process_groups"] == 0
    # sub-benchmarks: BASELINE configs 2, 3, 4 driver-timed in the default run, each with its own roofline; config 2 is the
    # HBM-bound one and carries its measured traffic (= the algorithmic 4304 B/frame)
    sub = {s["name"]: s for s in full["sub_benchmarks"]}
    assert {"config2", "config3_kmax1", "config3_kmax8", "config4", "pipeline_shapes", "speech_44k", "config5_100h_1gpu"} <= set(sub)
    # round 5: BASELINE config 5 WHOLE on this GPU (36 M frames, 138 GB resident) and the pipeline on real 44.1 kHz speech
    c5 = sub["config5_100h_1gpu"]
    assert "skipped" in c5 or (c5["frames"] == 36_000_000 and c5["value"] > 1e6 and c5["frames_with_nonzero_status"] == 0)
    for row in sub["speech_44k"]["shapes"]:
        assert row["speech"]["value"] > 1e6 and row["synthetic"]["value"] > 1e6 and row["speech"]["frames_with_nonzero_status"] == 0
        assert 0.0 <= row["speech"]["burg_direct"] <= 1.0 and row["speech"]["roots_direct"] >= 0.0
        assert row["speech"]["dominant_kernel"] == "analyze"        # the critical stream's kernel, not a co-resident one's event time
    assert all(r["dominant_kernel"] in ("analyze", "pitch") for r in sub["pipeline_shapes"]["shapes"])
    # round 6: the fast paths' hand-over shares per shape -- on the synthetic signal the one-pass Burg hands <= 2 % of the frames of
    # ANY shape to the direct recursion, and a fraction of a per cent of the Levinson rows are redone exactly
    for r in sub["pipeline_shapes"]["shapes"]:
        assert 0.0 <= r["burg_direct"] <= 0.02 and 0.0 <= r["roots_direct"] <= 0.02 and -1e-4 <= r["lpc_exact"] <= 0.02, r      # (-1 / F: the call wrote no probed LPC rows)
    c2 = sub["config2"]["roofline"]
    assert c2["bound"] == "hbm" and c2["kernel"] == "autocorr_lpc" and 0.4 < c2["frac"] < 1.0
    assert c2["traffic"] is not None and abs(c2["traffic"] / sub["config2"]["frames"] - 4304) < 0.05 * 4304
    assert sub["config3_kmax1"]["value"] > sub["config3_kmax8"]["value"] > 1e6 and sub["config4"]["whole_config"]["fp64_frac"] > 0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["value"] > 0 and c["cores"] >= 1 and c["one_core"]["cores"] == 1 and c["sample"]


def test_plain_run_times_the_headline_only_and_dumps_the_same_outputs_twice(tmp_path):
    """Without --full the line carries the headline and the roofline of its own timed steps, nothing measured elsewhere; the
    outputs of the last timed step (one record and the three statuses per frame) are the same, bit for bit, in two runs."""
    import numpy as np
    dumps = []
    for run in ("a", "b"):
        d = _bench("--hours", "0.25", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / run))
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"] == "f64" and d["unit"] == "frames/s"
        assert d["value"] == pytest.approx(d["config"]["frames_per_gpu"] / (d["ms_per_step"] * 1e-3), rel=1e-4)
        for k in ("cpu_baseline", "sub_benchmarks", "cross_rank_check", "parity", "live_traffic_error"):
            assert k not in d, k
        assert d["roofline"]["kernel"] == "analyze" and d["roofline"]["traffic_source"].startswith("committed")
        dumps.append({n: np.load(tmp_path / run / f"{n}.npy") for n in ("records", "status")})
    F = d["config"]["frames_per_gpu"]
    rec, st = dumps[0]["records"], dumps[0]["status"]
    assert rec.dtype == st.dtype == np.float64 and rec.shape == (F, d["config"]["record_bytes"] // 8) and st.shape == (F, 3)
    assert np.all(st == 0)
    for n in ("records", "status"):
        assert dumps[0][n].tobytes() == dumps[1][n].tobytes(), n


def test_config_workloads_pick_the_measured_dominant_kernel():
    d, full = _bench("--workload", "config4", "--frames", "200000", "--steps", "3", "--warmup", "1", "--no-cpu", detail=True)
    assert d["metric"].startswith("frames/sec (config4") and d["roofline"]["kernel"] in d["kernels_ms"]
    assert d["roofline"]["kernel"] == max(d["kernels_ms"], key=lambda k: d["kernels_ms"][k])
    assert "whole_config" in d and d["whole_config"]["fp64_frac"] > 0 and "kernels_ms_per_step" in full["whole_config"]
    d = _bench("--workload", "config3", "--frame-len", "2048", "--hop", "1024", "--hours", "0.25", "--steps", "2", "--warmup", "1", "--no-cpu")
    assert "2048-sample frames" in d["metric"] and d["config"]["frame_len"] == 2048 and d["roofline"]["kernel"] == "pitch"


def test_speech_mode_line():
    """bench.py --signal speech: the pipeline on the tiled 44.1 kHz fixture under its own metric name, with the fast paths'
    fallback shares and the refinement's work counters beside the synthetic signal at the same shapes."""
    d, full = _bench("--full", "--signal", "speech", "--hours", "0.1", "--steps", "1", "--warmup", "1", "--no-cpu", detail=True)
    assert "real 44.1 kHz speech" in d["metric"] and d["data"].startswith("real speech") and d["value"] > 1e6
    assert d["speech"]["1103/441"]["speech"] == pytest.approx(d["value"], rel=1e-5)
    rows = full["speech"]["shapes"]
    assert [(r["frame_len"], r["hop"]) for r in rows] == [(1103, 441), (1024, 512)]
    for r in rows:
        assert r["speech"]["sinc_evals_per_frame"] > 5 and r["synthetic"]["sinc_evals_per_frame"] > 5
        assert 0.2 < r["speech_over_synthetic"] < 2.0 and r["speech"]["burg_direct"] > r["synthetic"]["burg_direct"]


def test_cross_rank_check_rehearsal_on_one_gpu():
    """At N > 1 rank 0 re-analyses the frames around every shard cut on its own GPU and compares them, bit for bit, with the rows
    the ranks produced and the gather delivered (`cross_rank_check` in the bench line).  VBX_BENCH_SELFCHECK=1 runs the same code
    at N = 1 against an interior "cut": the check itself is exercised on every one-GPU box."""
    d = _bench("--full", "--hours", "0.5", "--steps", "2", "--warmup", "1", "--no-cpu", "--no-sub", env={"VBX_BENCH_SELFCHECK": "1"})
    c = d["cross_rank_check"]
    assert "error" not in c, c
    assert c["rows_compared"] >= 7000 and c["rows_different"] == 0 and c["verdict"] == "bit-identical", c
    assert "cross_rank_check" not in _bench("--full", "--hours", "0.25", "--steps", "1", "--warmup", "1", "--no-cpu", "--no-sub")


def test_two_ranks_without_a_second_gpu_fail_loudly_and_never_fall_back():
    """`--gpus 2` with both ranks forced onto GPU 0: RCCL refuses the duplicate device, so the library's communicator does not
    come up -- the bench must then FAIL on every rank (gloo-reduced flag), quickly, with the reason; it must not print a line
    measured over some other transport (round 2 fell back to torch.distributed P2P inside the timed region)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env["VBX_BENCH_ONE_GPU"] = "1"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--hours", "0.25", "--steps", "1", "--warmup", "0", "--no-cpu"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0
    assert not [l for l in p.stdout.splitlines() if l.startswith('{"metric"')], p.stdout[-500:]
    assert "no fallback transport" in p.stderr and "ncclCommInitRank" in p.stderr, p.stderr[-1500:]
