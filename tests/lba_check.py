"""Shared by the CPU-program test and the GPU tests of the bundle adjustment: building and running tests/cpp/lba_cpu.cpp, the
scene and result files, the comparison of two runs and the tolerance rule."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def build_cpu_program(out_dir):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the CPU program with"
    exe = Path(out_dir) / "lba_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I",
                    str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "lba_cpu.cpp"), "-o", str(exe)], check=True)
    return exe


def write_scene(path, sc, kind="local", stop_before=None):
    T = np.asarray(sc["Tcw"], np.float32).reshape(-1, 16)
    n_local, n_edges, n_points = int(sc["n_local"]), len(sc["edge_pose"]), len(sc["xw"])
    fixed = sc.get("local_is_fixed")
    glob = kind != "local"
    hd = [n_local, len(T) - n_local, n_points, n_edges, int(fixed is not None), int(glob), kind[1] if glob else 0,
          int(kind[2]) if glob else 1, -1 if stop_before is None else int(stop_before)]
    with open(path, "wb") as f:
        f.write(struct.pack("9i", *hd))
        f.write(T.tobytes())
        f.write((np.zeros(n_local, np.uint8) if fixed is None else np.asarray(fixed, np.uint8)).tobytes())
        for k, dt in (("cam", np.float32), ("xw", np.float32), ("edge_pose", np.int32), ("edge_point", np.int32), ("u", np.float32),
                      ("v", np.float32), ("u_right", np.float32), ("inv_sigma2", np.float32)):
            f.write(np.ascontiguousarray(sc[k], dtype=dt).tobytes())


def read_result(path, sc):
    n_local, nE, nP = int(sc["n_local"]), len(sc["edge_pose"]), len(sc["xw"])
    raw = Path(path).read_bytes()
    o = 0

    def take(dt, n):
        nonlocal o
        a = np.frombuffer(raw, dt, n, o)
        o += a.nbytes
        return a
    out = dict(Tcw=take(np.float64, 16 * n_local).reshape(-1, 4, 4), xw=take(np.float64, 3 * nP).reshape(-1, 3), erase=take(np.uint8, nE),
               level1=take(np.uint8, nE), edge_chi2=take(np.float64, nE))
    ints = take(np.int32, 8)
    out.update(rounds=int(ints[0]), stopped=int(ints[1]), iterations=ints[2:4].tolist(), trials=ints[4:6].tolist(),
               termination=ints[6:8].tolist(), lam=take(np.float64, 2).tolist(), chi2=take(np.float64, 2).tolist())
    assert o == len(raw)
    return out


def run_cpu(exe, tmp, sc, kind="local", stop_before=None):
    write_scene(tmp / "scene.bin", sc, kind, stop_before)
    r = subprocess.run([str(exe), str(tmp / "scene.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_result(tmp / "out.bin", sc)


def deviation(a, b):
    """largest difference of the continuous results of two runs -> (poses and points, absolute; edge_chi2, lambda and the
    rounds' chi2 relative to max(|value|, 1): a chi2 is a statistic with thresholds near 6, below 1 it is compared absolutely)"""
    d_abs = max(float(np.abs(a["Tcw"] - b["Tcw"]).max()), float(np.abs(a["xw"] - b["xw"]).max()))
    rel = [np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)) / np.maximum(np.abs(np.asarray(b[k], np.float64)), 1.0)
           for k in ("edge_chi2", "lam", "chi2")]
    return d_abs, float(max(r.max(initial=0.0) for r in rel))


ULP32 = 2.0 ** -23
MARGIN = 16  # the project's standing margin


def tolerance(sc, s_ref, s_cpu):
    """max(16 x max(s_ref, s_cpu), 4 float32 ulps) -> (absolute for poses and points, relative for the chi2 group); the ulps
    are those of the largest coordinate of the scene (the caller stores the results as floats)"""
    big = max(float(np.abs(sc["Tcw"]).max()), float(np.abs(sc["xw"]).max()), 1.0)
    return max(MARGIN * max(s_ref[0], s_cpu[0]), 4 * ULP32 * big), max(MARGIN * max(s_ref[1], s_cpu[1]), 4 * ULP32)


DISCRETE = ("rounds", "stopped", "iterations", "trials", "termination")


def assert_discrete_equal(got, want, id_):
    for k in DISCRETE:
        assert got[k] == want[k], (id_, k, got[k], want[k])
    assert np.array_equal(got["erase"], want["erase"]), id_
    assert np.array_equal(got["level1"], want["level1"]), id_


TOLERANCE_FILE = ROOT / "profiles" / "lba_tolerance.txt"


def recorded():
    """the key=value tokens of profiles/lba_tolerance.txt: <scene>.<s_ref|s_schur|s_cpu>_<abs|rel>"""
    return {k: float(v) for k, v in (t.split("=") for t in TOLERANCE_FILE.read_text().split() if "=" in t and not t.startswith("="))}


def agrees(measured, written):
    """a recorded deviation names the measured one: the same order of magnitude (rounding noise depends on the linear algebra
    library behind numpy), or both below 1e-12"""
    return (measured < 1e-12 and written < 1e-12) or written / 16 <= measured <= written * 16
