"""Shared by the CPU-program test and the GPU tests of the essential-graph optimisation: building and running
tests/cpp/essgraph_cpu.cpp, the scene and result files, the comparison of two runs and the tolerance rule."""
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
    exe = Path(out_dir) / "essgraph_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I",
                    str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "essgraph_cpu.cpp"), "-o", str(exe)], check=True)
    return exe


def write_scene(path, sc):
    n, nE = len(sc["sim3"]), len(sc["edge_i"])
    with open(path, "wb") as f:
        f.write(struct.pack("4i", n, nE, int(sc["fix_scale"]), int(sc["n_iterations"])))
        for k, dt in (("sim3", np.float64), ("sim3_meas", np.float64), ("is_fixed", np.uint8), ("edge_i", np.int32), ("edge_j", np.int32),
                      ("edge_kind", np.uint8)):
            f.write(np.ascontiguousarray(sc[k], dtype=dt).tobytes())


def read_result(path, sc):
    n, nE = len(sc["sim3"]), len(sc["edge_i"])
    raw = Path(path).read_bytes()
    o = 0

    def take(dt, k):
        nonlocal o
        a = np.frombuffer(raw, dt, k, o)
        o += a.nbytes
        return a
    out = dict(sim3_out=take(np.float64, 8 * n).reshape(-1, 8), Tiw=take(np.float32, 16 * n).reshape(-1, 4, 4), edge_chi2=take(np.float64, nE))
    ints = take(np.int32, 8)
    dbl = take(np.float64, 3)
    out.update(iterations=int(ints[0]), trials=int(ints[1]), termination=int(ints[2]), host_syncs=int(ints[3]), n_free=int(ints[4]),
               blocks_A=int(ints[5]), blocks_L=int(ints[6]), solve_failures=int(ints[7]), lam=float(dbl[0]), chi2_initial=float(dbl[1]),
               chi2=float(dbl[2]))
    assert o == len(raw)
    return out


def run_cpu(exe, tmp, sc):
    write_scene(tmp / "scene.bin", sc)
    r = subprocess.run([str(exe), "opt", str(tmp / "scene.bin"), str(tmp / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_result(tmp / "out.bin", sc)


def solve_cpu(exe, tmp, colptr, rowidx, blocks, rhs):
    """tests/cpp/essgraph_cpu.cpp solve -> (x, ok, blocks_L)"""
    n = len(colptr) - 1
    with open(tmp / "system.bin", "wb") as f:
        f.write(struct.pack("2i", n, len(rowidx)))
        f.write(np.ascontiguousarray(colptr, np.int32).tobytes())
        f.write(np.ascontiguousarray(rowidx, np.int32).tobytes())
        f.write(np.ascontiguousarray(blocks, np.float64).tobytes())
        f.write(np.ascontiguousarray(rhs, np.float64).tobytes())
    r = subprocess.run([str(exe), "solve", str(tmp / "system.bin"), str(tmp / "x.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    raw = (tmp / "x.bin").read_bytes()
    x = np.frombuffer(raw, np.float64, 7 * n)
    ok, nl = np.frombuffer(raw, np.int32, 2, 8 * 7 * n)
    return x, int(ok), int(nl)


def from_device(result):
    """what optimizer.optimize_essential_graph returns, as the dictionary the other two carry"""
    sim3_out, Tiw, st, chi2 = result
    out = dict(st)
    out.update(sim3_out=sim3_out, Tiw=Tiw, edge_chi2=chi2)
    return out


def call_device(opt, sc, **kw):
    return from_device(opt.optimize_essential_graph(sc["sim3"], sc["edge_i"], sc["edge_j"], sim3_meas=sc["sim3_meas"], is_fixed=sc["is_fixed"],
                                                    edge_kind=sc["edge_kind"], fix_scale=sc["fix_scale"],
                                                    n_iterations=kw.get("n_iterations", sc["n_iterations"])))


def deviation(a, b):
    """largest difference of the continuous results of two runs -> (sim3_out, absolute; edge_chi2, lambda, chi2_initial and
    chi2 relative to max(|value|, 1), as DESIGN 4.Q reads a chi2)"""
    d_abs = float(np.abs(np.asarray(a["sim3_out"]) - np.asarray(b["sim3_out"])).max())
    rel = [np.abs(np.asarray(a[k], np.float64) - np.asarray(b[k], np.float64)) / np.maximum(np.abs(np.asarray(b[k], np.float64)), 1.0)
           for k in ("edge_chi2", "lam", "chi2_initial", "chi2")]
    return d_abs, float(max(np.max(r, initial=0.0) for r in rel))


ULP32 = 2.0 ** -23
MARGIN = 16  # the project's standing margin


def tolerance(sc, s_ref, s_cpu):
    """max(16 x max(s_ref, s_cpu), 4 float32 ulps of the scene's largest coordinate) -> (absolute for sim3_out, relative for
    the chi2 group)"""
    big = max(float(np.abs(sc["sim3"]).max()), float(np.abs(sc["sim3_meas"]).max()), 1.0)
    return max(MARGIN * max(s_ref[0], s_cpu[0]), 4 * ULP32 * big), max(MARGIN * max(s_ref[1], s_cpu[1]), 4 * ULP32)


DISCRETE = ("iterations", "trials", "termination", "n_free", "blocks_A", "blocks_L", "solve_failures", "host_syncs")


def assert_discrete_equal(got, want, id_):
    for k in DISCRETE:
        assert got[k] == want[k], (id_, k, got[k], want[k])


TOLERANCE_FILE = ROOT / "profiles" / "essential_graph_tolerance.txt"


def recorded():
    """the key=value tokens of profiles/essential_graph_tolerance.txt"""
    return {k: float(v) for k, v in (t.split("=") for t in TOLERANCE_FILE.read_text().split() if "=" in t and not t.startswith("="))}


def agrees(measured, written):
    """a recorded deviation names the measured one: the same order of magnitude (rounding noise depends on the linear algebra
    library behind numpy), or both below 1e-12"""
    return (measured < 1e-12 and written < 1e-12) or written / 16 <= measured <= written * 16
