"""bench.py's ONE stdout line (the driver parses the last line of stdout; round 5's 25 KB line came back `parsed: null`):
final_line() must keep every contract key, stay under its byte cap whatever the tree holds, and round-trip as strict JSON."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _tree():
    """a full result tree as a real run produced it (round 5's, kept under profiles/), with this round's additions"""
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_n1.json")))
    full["ms_per_step_min_median_max"] = [0.051, 0.0533, 0.0611]
    full["latency_batch_of_one"] = {k: {"p50_us": 61.25, "p99_us": 140.123456, "planned_p50_us": 80.0, "planned_p99_us": 190.0, "same_as_batch": True}
                                    for k in ("term", "and3", "or10")}
    full["latency_batch_of_one"]["note"] = "x" * 500
    full["config"]["timed_regions"] = "5 regions of 20 steps"
    return full


def test_line_has_the_contract_keys_and_fits():
    full = _tree()
    assert len(json.dumps(full)) > 20_000   # the tree itself is what the driver could not parse
    text = bench.final_line(full)
    assert "\n" not in text and len(text.encode()) < bench.LINE_MAX_BYTES <= 8192
    line = json.loads(text)
    for key in bench.LINE_REQUIRED + ("cpu_baseline", "parity"):
        assert key in line, key
    assert line["metric"] == full["metric"] and line["n_gpus"] == 1 and line["higher_is_better"] is True and line["scaling"] == "weak"
    assert line["config"]["workload"] == full["config"]["workload"] and "model" not in line["config"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in line["roofline"], key
    assert line["roofline"]["bound"] == "hbm" and 0 < line["roofline"]["frac"] <= 1 and line["roofline"]["peak"] == 8000.0
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in line["cpu_baseline"], key
    assert line["cpu_baseline"]["kind"] in ("port", "reference")
    assert abs(line["value"] - full["value"]) <= 1e-4 * full["value"]
    # the north-star's other targets travel as scalars
    for key in ("and3_queries_per_sec", "and3_roofline_frac", "block_decode_frac", "big_and3_roofline_frac", "or10_queries_per_sec"):
        assert isinstance(line[key], (int, float)), key
    assert line["latency_us_p50_p99"]["term"] == [61.25, 140.12]
    assert all(not isinstance(v, dict) or k in ("config", "roofline", "cpu_baseline", "parity", "latency_us_p50_p99", "latency_planned_us_p50_p99")
               for k, v in line.items())


def test_line_sheds_hoisted_scalars_before_it_grows_past_the_cap():
    full = _tree()
    full["config"]["workload"] = "w" * 100
    full["cpu_baseline"]["sample"] = "s" * 5000      # clipped
    full["roofline"]["bytes_are"] = "b" * 5000       # clipped
    text = bench.final_line(full)
    assert len(text.encode()) < bench.LINE_MAX_BYTES
    line = json.loads(text)
    assert len(line["cpu_baseline"]["sample"]) <= 240 and len(line["roofline"]["bytes_are"]) <= 200
    # a tree that would not fit even so: hoisted names (here: made absurdly long values impossible, so shrink the cap instead)
    old = bench.LINE_MAX_BYTES
    try:
        bench.LINE_MAX_BYTES = 2600
        small = json.loads(bench.final_line(full))
        assert small.get("truncated") is True
        for key in bench.LINE_REQUIRED:
            assert key in small
    finally:
        bench.LINE_MAX_BYTES = old


def test_line_refuses_a_tree_without_the_contract_keys():
    full = _tree()
    del full["roofline"]
    with pytest.raises(AssertionError):
        bench.final_line(full)
    full = _tree()
    full["value"] = float("nan")
    with pytest.raises(ValueError):
        bench.final_line(full)


def test_plain_line_needs_no_roofline_and_keeps_the_contract_keys():
    """a run without --full has no kernel event pass, so no roofline: its line must still carry every other contract key"""
    full = _tree()
    for key in ("roofline", "cpu_baseline", "parity", "configs", "streams", "latency_batch_of_one", "sharded_overhead"):
        full.pop(key, None)
    line = json.loads(bench.final_line(full, required=bench.LINE_REQUIRED_PLAIN))
    assert "roofline" not in line and "cpu_baseline" not in line
    for key in bench.LINE_REQUIRED_PLAIN:
        assert key in line, key
    assert line["metric"] == full["metric"] and line["higher_is_better"] is True and abs(line["value"] - full["value"]) <= 1e-4 * full["value"]
    with pytest.raises(AssertionError):
        bench.final_line(full)   # the --full requirements still ask for the roofline
    full["ms_per_step"] = None
    with pytest.raises(AssertionError):
        bench.final_line(full, required=bench.LINE_REQUIRED_PLAIN)


def test_jsonable_drops_private_keys_and_numpy_types():
    import numpy as np
    tree = {"a": np.float32(1.5), "b": np.arange(3), "_rows": np.zeros(4), "c": {"_x": 1, "y": float("inf")}, 7: (np.int64(2),)}
    assert bench._jsonable(tree) == {"a": 1.5, "b": [0, 1, 2], "c": {"y": None}, "7": [2]}


def test_dump_outputs_writes_what_the_caller_received(tmp_path):
    import numpy as np
    rng = np.random.default_rng(1)
    hits = np.zeros((6, 4), dtype=[("doc", "<i4"), ("score", "<f4")])
    hits["doc"] = rng.integers(0, 2**31 - 1, hits.shape)
    hits["score"] = rng.random(hits.shape, dtype=np.float32)
    hits[5, 2:] = (-1, 0.0)                                   # unused slots as the kernels leave them
    totals = np.array([7, 2**40 + 1, 0, 3, 9, 2], np.int64)
    shapes = bench.dump_outputs(str(tmp_path / "d"), hits.view(np.int64), totals)
    assert shapes == {"doc": (6, 4), "score": (6, 4), "total_hits": (6,), "query": (6,)}
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in shapes}
    assert got["doc"].dtype == np.float64 and (got["doc"].astype(np.int64) == hits["doc"]).all()
    assert got["score"].dtype == np.float32 and (got["score"].view(np.int32) == hits["score"].view(np.int32)).all()
    assert got["total_hits"].dtype == np.float64 and (got["total_hits"].astype(np.int64) == totals).all()
    assert (got["query"] == np.arange(6)).all()


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1000)
    hits = np.zeros((100, 10), dtype=[("doc", "<i4"), ("score", "<f4")])
    hits["doc"] = np.arange(1000).reshape(100, 10)
    totals = np.arange(100, dtype=np.int64)
    a = bench.dump_outputs(str(tmp_path / "a"), hits, totals)
    bench.dump_outputs(str(tmp_path / "b"), hits, totals)
    assert a["doc"] == (7, 10) and sum(os.path.getsize(str(tmp_path / "a" / (n + ".npy"))) - 128 for n in a) <= 1000
    q = np.load(str(tmp_path / "a" / "query.npy"))
    assert (np.diff(q) > 0).all() and (q == np.load(str(tmp_path / "b" / "query.npy"))).all()
    assert (np.load(str(tmp_path / "a" / "doc.npy")) == hits["doc"][q.astype(np.int64)]).all()


def test_steps_below_one_is_refused():
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_configs_without_full_is_refused():
    """a plain run measures the headline alone: asking it for configs is an error, not a silent no-op"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--configs", "and3"], capture_output=True, text=True)
    assert p.returncode == 2 and "--full" in p.stderr
