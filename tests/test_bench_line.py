"""The ONE stdout line of bench.py must stay parseable by the driver (round 3 printed 31 KB and the driver's 8 KB tail
held no complete object): compact_line() of a canned full result -- round 3's own committed run -- is < 4 KB,
round-trips through json and keeps every key the contract names."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

CONTRACT = ["metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config", "roofline", "cpu_baseline"]


def _canned():
    return json.loads((ROOT / "profiles" / "r03_bench.json").read_text())


def test_compact_line_is_small_and_complete():
    full = _canned()
    assert len(json.dumps(full)) > 20000  # the canned run really is the oversized one
    line = bench.compact_line(full, "gpurun_out/bench_detail.json")
    assert "\n" not in line and len(line) < bench.LINE_LIMIT == 4096
    out = json.loads(line)
    for k in CONTRACT:
        assert k in out, k
    assert out["value"] == float(f"{full['value']:.6g}") and out["unit"] == "stereo frames/s"
    assert "workload" in out["config"] and "model" not in out["config"]
    rf = out["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "stage", "pipeline", "stages_exclusive_ms"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4
    assert rf["valu_issue"]["pipeline_frac"] > 0
    cb = out["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert "variants" not in cb and cb["kind"] in ("port", "reference")
    assert out["parity_check"]["ok"] is True
    assert [s_["key"] for s_ in out["secondary"]] == ["tum", "euroc", "euroc_stereo"]
    for s_ in out["secondary"]:
        assert set(s_) <= {"key", "value", "unit", "ms_per_step", "vs_cpu_baseline", "pipeline_frac", "parity_ok", "scaling", "plans"}
    assert out["detail"] == "gpurun_out/bench_detail.json"
    assert "latency" not in out and "e2e" not in out and "matching_work" not in out


def test_compact_line_sheds_before_it_overflows():
    full = _canned()
    full["secondary"] = full["secondary"] * 12  # a pathological run: the line must still fit
    line = bench.compact_line(full, None)
    assert len(line) < bench.LINE_LIMIT
    out = json.loads(line)
    for k in CONTRACT:
        assert k in out, k


def test_emit_writes_the_detail_file_and_prints_the_line_last(tmp_path, capsys):
    import argparse
    full = _canned()
    args = argparse.Namespace(no_detail=False, detail_out=str(tmp_path / "d.json"), full_line=False)
    bench.emit(full, args)
    last = capsys.readouterr().out.strip().splitlines()[-1]
    assert len(last) < 4096 and json.loads(last)["detail"].endswith("d.json")
    kept = json.loads((tmp_path / "d.json").read_text())
    assert kept["latency"]["rows"] and kept["secondary"][0]["roofline"]["stages"]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_step(tmp_path):
    """A plain run times exactly --steps steps of the headline and reports their ms_per_step; --dump-outputs writes the
    last step's keypoints / descriptors / stereo matches of a fixed sample of pairs, equal to the CPU oracle's."""
    import os
    import subprocess
    import numpy as np
    import oracle_lib as orc
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "20",
                        "--render-procs", "1", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "stereo frames/s" and out["higher_is_better"] is True
    assert out["ms_per_step"] > 0 and abs(out["value"] - 20 * 1e3 / out["ms_per_step"]) < 1e-3 * out["value"]
    assert "secondary" not in out and "cpu_baseline" not in out and "roofline" not in out
    d = {f.stem[len("kitti_"):]: np.load(f) for f in tmp_path.glob("kitti_*.npy")}
    assert set(d) == {"keypoint_counts", "keypoints", "descriptors", "stereo_match_counts", "mvuRight", "mvDepth"}
    assert all(a.dtype == np.float32 for a in d.values())
    units = np.sort(np.random.default_rng(0).choice(20, size=bench.DUMP_UNITS, replace=False))
    frames = bench.render_inputs(["kitti"], {"kitti": 20}, 0, 1)["kitti"]
    wl = bench.WORKLOADS["kitti"]
    o = orc.Oracle(wl["nfeatures"], 1.2, 8, wl["ini"], wl["mn"])
    kps, descs, pyrs = zip(*(o.extract(frames[i], want_pyramid=True) for u in units for i in (2 * u, 2 * u + 1)))
    assert np.array_equal(d["keypoint_counts"], [len(k) for k in kps])
    ref_kp = np.concatenate([np.stack([k[f].astype(np.float32) for f in k.dtype.names], axis=1) for k in kps])
    assert np.array_equal(d["keypoints"], ref_kp) and np.array_equal(d["descriptors"], np.concatenate(descs))
    mbf = np.float32(wl["bf"])
    st = [o.stereo(wl["w"], wl["h"], kps[j], descs[j], kps[j + 1], descs[j + 1], pyrs[j], pyrs[j + 1], float(mbf),
                   float(np.float32(mbf / np.float32(wl["fx"])))) for j in range(0, len(kps), 2)]
    assert np.array_equal(d["mvuRight"], np.concatenate([u for u, _ in st]))
    assert np.array_equal(d["mvDepth"], np.concatenate([dep for _, dep in st]))
    assert np.array_equal(d["stereo_match_counts"], [(u >= 0).sum() for u, _ in st])
