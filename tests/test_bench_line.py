"""The line bench.py prints must stay parseable by the driver (VERDICT r05
items 1 and 7): BENCH_r05.parsed was null because the one JSON line had
grown to 21.5 KB and the driver reads only the tail of stdout.  The line now
carries the contract keys, the headline roofline and CPU baseline, every
verification flag and one compact entry per leg; the full record goes to a
detail file the line names.  CPU only: the full records here are committed
bench output (profiles/) and the N > 1 dry run's record, which the real
run's own helpers fill (bench.dry_run_record)."""
import json
import os
import subprocess
import sys

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R05_FULL = os.path.join(ROOT, "profiles", "r05zq", "bench_default.log")   # round 5's 21.5-KB line


def _full_r05():
    for line in open(R05_FULL):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError("no JSON line in " + R05_FULL)


def _size(d):
    return len(json.dumps(d, separators=(",", ":"), allow_nan=False))


def test_round5_line_compacts_under_6kb():
    full = _full_r05()
    assert len(json.dumps(full)) > 20000          # the record that was unparseable
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    assert _size(line) <= bench.LINE_MAX_BYTES
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config",
              "roofline", "cpu_baseline", "verified_vs_oracle", "configs", "detail_file"):
        assert k in line, k
    assert line["value"] == full["value"] and line["ms_per_step"] == full["ms_per_step"]
    rf = line["roofline"]
    assert set(rf) >= {"bound", "achieved", "peak", "unit", "frac", "traffic", "source"}
    assert rf["frac"] == full["roofline"]["frac"]
    assert set(line["cpu_baseline"]) >= {"value", "cores", "kind"}
    for key in ("config3", "config4", "config5"):
        leg = line["configs"][key]
        assert leg["ms_per_step"] == full["configs"][key]["ms_per_step"]
        assert leg["frac"] == full["configs"][key]["roofline"]["frac"]
        assert "ff" in leg and leg["ff"]["ms_per_step"] == full["configs"][key]["frame_filling_camera"]["ms_per_step"]


def test_n1_line_with_every_round6_field_under_6kb():
    """The N = 1 line with the drop-in frame, per-leg verifications and the
    longest strings the fields allow."""
    full = _full_r05()
    full["single_context"] = {"ms_per_step": 0.2345, "steps": 200, "value": 130000.0, "kernel_ms": 0.23,
                              "verified_vs_oracle": True, "basis": "x" * 500}
    full["cpu_baseline"]["sample"] = "y" * 2000
    for leg in full["configs"].values():
        for cam in (leg, leg["frame_filling_camera"]):
            cam["verified_vs_exhaustive"] = True
            cam["verified_vs_exhaustive_basis"] = "z" * 400
            cam["profile_parallelism_matches"] = True
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    assert _size(line) <= bench.LINE_MAX_BYTES
    assert line["single_context"]["verified_vs_oracle"] is True
    assert all(v["verified"] is True and v["ff"]["verified"] is True for v in line["configs"].values())


@pytest.mark.parametrize("world", [2, 8])
def test_n_gpu_record_compacts_under_6kb(world):
    full = bench.dry_run_record(world, list(range(world)), "external", "nccl")
    line = bench.compact_line(full)
    assert _size(line) <= bench.LINE_MAX_BYTES
    assert line["config"]["rccl_comm_ranks"] == world
    g = line["group_leg"]
    assert g["peer_store_check"] == "matched" and g["exchange0"]["verified"] is True
    assert g["exchange1"]["verified"] is True
    for key in ("config4", "config5"):
        assert line["configs"][key]["verified"] is True and line["configs"][key]["n_gpus"] == world
    err = line["configs"]["config_failed"]["error"]
    assert err.startswith("rank 7:") and len(err) <= 300


def test_line_is_strict_json():
    full = bench.dry_run_record(2, [0, 1], "external", "nccl")
    full["value"] = float("nan")
    full["roofline"]["frac"] = float("inf")
    line = bench.compact_line(full)
    assert line["value"] is None and line["roofline"]["frac"] is None
    json.dumps(line, allow_nan=False)


def test_oversized_line_is_refused():
    full = bench.dry_run_record(2, [0, 1], "external", "nccl")
    full["metric"] = "m" * (bench.LINE_MAX_BYTES + 1)
    with pytest.raises(ValueError):
        bench.compact_line(full)


def test_two_rank_dry_run_prints_one_compact_last_line(tmp_path):
    """`bench.py --gpus 2 --dry-run` (gloo, spawned ranks): the last stdout
    line parses, is <= 6 KB and carries the N > 1 keys; the full record lands
    in the detail file."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["PT_BENCH_DETAIL"] = str(tmp_path / "detail.json")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], cwd=ROOT,
                         env=env, capture_output=True, text=True, timeout=180)
    assert res.returncode == 0, res.stderr[-3000:]
    last = res.stdout.strip().splitlines()[-1]
    assert len(last) <= bench.LINE_MAX_BYTES
    line = json.loads(last)
    assert line["n_gpus"] == 2 and line["config"]["rccl_comm_ranks"] == 2
    assert {"peer_store_check", "exchange0", "exchange1"} <= set(line["group_leg"])
    assert line["detail_file"] == str(tmp_path / "detail.json")
    detail = json.load(open(line["detail_file"]))
    assert detail["group_leg"]["peer_store_check"]["state"] == "matched"


def test_dump_outputs_writes_the_whole_frame_as_float32(tmp_path):
    """--dump-outputs: a frame within the size limit lands whole, bit for
    bit, as float32 [H, W, 4]."""
    import numpy as np
    W, H = 37, 23
    frame = np.random.default_rng(1).random(W * H * 4, dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "out"), frame, W, H)
    got = np.load(tmp_path / "out" / "accum.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 4)
    assert np.array_equal(got.reshape(-1).view(np.uint32), frame.view(np.uint32))


def test_dump_outputs_samples_a_large_frame_the_same_way_every_time(tmp_path, monkeypatch):
    """A frame above the limit is written as a seeded sample of its pixels:
    within the limit, the same pixels on every call, each a pixel of the
    frame (its first float carries the pixel's index here)."""
    import numpy as np
    W, H = 64, 48
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16 * 500)
    frame = np.zeros((H * W, 4), np.float32)
    frame[:, 0] = np.arange(H * W)
    frame[:, 1:] = np.random.default_rng(2).random((H * W, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), frame.reshape(-1), W, H)
    a, b = np.load(tmp_path / "a" / "accum.npy"), np.load(tmp_path / "b" / "accum.npy")
    assert a.dtype == np.float32 and a.shape == (500, 4) and a.nbytes <= 16 * 500
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    idx = a[:, 0].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and np.array_equal(a.view(np.uint32), frame[idx].view(np.uint32))
