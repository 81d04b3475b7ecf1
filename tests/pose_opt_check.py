"""What the tests of orbfe_pose_optimization* share: the scene file tests/cpp/poseopt_cpu.cpp reads, the recorded tolerances
(profiles/pose_opt_tolerance.txt), the engineered scenes beyond pose_opt_ref.gpu_scenes() and THE pass condition of a result
against the restatement (tests/pose_opt_ref.py):

* outlier[], the return value and stats.rounds identical;
* every Tcw_out entry within max(16 x s_pose, 4 float32 ulps of the entry);
* every classification chi2 within 16 x s_chi2, relative -- s_pose / s_chi2 being the reference's own reordering noise
  (measured by tests/test_pose_opt_ref.py).  The device's tree sum is a third summation order and its sin / cos / sqrt differ
  from libm in the last place, hence the margin of 16."""
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np

import pose_opt_ref as pr

ROOT = Path(__file__).resolve().parent.parent
TOLERANCE_FILE = ROOT / "profiles" / "pose_opt_tolerance.txt"


def tolerance():
    rec = dict(line.split("=") for line in TOLERANCE_FILE.read_text().split() if "=" in line)
    return float(rec["s_pose"]), float(rec["s_chi2"])


def check_against(ref, got, label):
    """THE pass condition of got = (n_inliers, Tcw_out, outlier, stats, edge_chi2) against a result of pose_opt_ref.run()."""
    ni, T, flags, st, chi2 = got
    s_pose, s_chi2 = tolerance()
    print(f"{label}: ref rounds {ref['rounds']} iterations {ref['iterations']} trials {ref['trials']} | got rounds {st['rounds']} "
          f"iterations {st['iterations']} trials {st['trials']}")
    assert st["rounds"] == ref["rounds"]
    assert ni == ref["n_inliers"]
    if ref["outlier"] is None:
        return
    assert np.array_equal(flags, ref["outlier"])
    want = ref["Tcw"].astype(np.float64)
    tol = np.maximum(16 * s_pose, 4 * np.spacing(np.abs(ref["Tcw"])).astype(np.float64))
    dev = np.abs(T.astype(np.float64) - want)
    print(f"{label}: pose deviation max {dev.max():.3e} (allowed {tol.min():.3e} ..)")
    assert (dev <= tol).all(), (dev.max(), st, ref["iterations"], ref["trials"])
    c = ref["edge_chi2"][-1]
    nz = c != 0
    rel = np.abs(chi2[nz] - c[nz]) / np.abs(c[nz])
    print(f"{label}: edge_chi2 relative deviation max {rel.max() if len(rel) else 0:.3e} (allowed {16 * s_chi2:.3e})")
    assert (rel <= 16 * s_chi2).all(), (rel.max(), st, ref["iterations"], ref["trials"])


def check_same_run(cpu, gpu, label):
    """The device against tests/cpp/poseopt_cpu.cpp -- the same header in the same summation order: every discrete field
    identical, every float within the pass condition above.  (A round's lambda is printed only: it is the start value times
    factors of rho = (cur - trial chi2) / scale, a difference that cancels near convergence, so no bound on it follows from
    s_chi2.)"""
    assert gpu[0] == cpu[0] and gpu[3]["rounds"] == cpu[3]["rounds"], label
    assert gpu[3]["iterations"] == cpu[3]["iterations"] and gpu[3]["trials"] == cpu[3]["trials"], (label, gpu[3], cpu[3])
    assert np.array_equal(gpu[2], cpu[2]), label
    s_pose, s_chi2 = tolerance()
    tol = np.maximum(16 * s_pose, 4 * np.spacing(np.abs(cpu[1])).astype(np.float64))
    dev = np.abs(gpu[1].astype(np.float64) - cpu[1].astype(np.float64))
    rel = np.abs(gpu[4] - cpu[4])[cpu[4] != 0] / np.abs(cpu[4][cpu[4] != 0])
    lam = np.abs(np.array(gpu[3]["lam"]) - np.array(cpu[3]["lam"]))
    print(f"{label}: pose deviation {dev.max():.3e}, edge_chi2 relative deviation {rel.max(initial=0.0):.3e}, lambda {lam.max(initial=0.0):.3e}")
    assert (dev <= tol).all(), (label, dev.max())
    assert np.array_equal(gpu[4][cpu[4] == 0], cpu[4][cpu[4] == 0]) and (rel <= 16 * s_chi2).all(), (label, rel.max(initial=0.0))
    a, b = np.array(gpu[3]["chi2"]), np.array(cpu[3]["chi2"])  # a round's robust chi2: a sum of edge chi2, the same bound
    assert (np.abs(a - b) <= 16 * s_chi2 * np.abs(b)).all(), (label, a, b)


def equal_points_scene(seed, n):
    """Every edge observes the same point, and with no information: the scene whose first solve meets a pivot that is not
    positive.  H is a sum of squares and lambda starts at 1e-5 max |H_jj|, so H + lambda I is positive definite unless that
    maximum is 0 -- equal points alone leave a rank-3 H and every pivot positive (and an ill-posed problem: with unit
    information the reference's own two summation orders differ by 4e-6 in the pose).  With inv_sigma2 = 0, H = 0 and
    lambda = 0: the first pivot is 0, every one of the ten trials of an iteration fails (update 0, chi2 DBL_MAX, rho = -inf,
    lambda stays 0) and the round ends on the trial limit with the start pose."""
    sc = pr.scene(seed, n, 0.5, 0.0)
    sc["xw"] = np.repeat(sc["xw"][:1], n, axis=0)
    sc["inv_sigma2"] = np.zeros(n, np.float32)
    return sc


# (id, seed, n, stereo fraction, outlier fraction): the sizes around one round (n < 10), around a lane's second edge (256) and
# a mono / stereo mix; seeds: the first whose scene keeps out of the guard bands (tests/test_pose_opt_math_cpu.py re-checks)
EXTRA = (("x-n2", 0, 2, 0.5, 0.2), ("x-n3", 0, 3, 0.5, 0.2), ("x-n9", 0, 9, 0.5, 0.2), ("x-n10", 0, 10, 0.5, 0.2),
         ("x-n255", 0, 255, 0.5, 0.2), ("x-n256", 0, 256, 0.5, 0.2), ("x-n257", 0, 257, 0.5, 0.2), ("x-mix-n40", 0, 40, 0.3, 0.1))


def extra_scenes():
    """(id, scene) of the engineered cases the CPU program runs beyond pose_opt_ref.gpu_scenes()."""
    out = [(id_, pr.scene(100 + seed, n, sf, of)) for id_, seed, n, sf, of in EXTRA]
    out.append(("x-all-outliers-n40", pr.scene(100, 40, 0.5, 0.0, all_outliers=True)))  # round two starts on an empty active set
    out.append(("x-equal-points-n24", equal_points_scene(0, 24)))
    return out


def build_program(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else (shutil.which("clang++") or shutil.which("g++"))
    assert cxx, "no compiler to build the program with"
    exe = tmp_path / "poseopt_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-I",
                    str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "poseopt_cpu.cpp"), "-o", str(exe)],
                   check=True)
    return exe


def write_scenes(path, scenes):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(scenes)))
        for sc in scenes:
            f.write(struct.pack("<i", len(sc["u"])))
            for key in ("K5", "Tcw", "xw", "u", "v", "u_right", "inv_sigma2"):
                f.write(np.ascontiguousarray(sc[key], np.float32).tobytes())


def read_results(path, scenes):
    """-> per scene the tuple pose_optimization() returns: (n_inliers, Tcw_out, outlier, stats, edge_chi2); the flags the
    program starts from are 7."""
    out = []
    buf = Path(path).read_bytes()
    at = 0
    for sc in scenes:
        n = len(sc["u"])
        T = np.frombuffer(buf, np.float32, 16, at).reshape(4, 4)
        i = np.frombuffer(buf, np.int32, 10, at + 64)
        d = np.frombuffer(buf, np.float64, 8, at + 104)
        at += 168
        flags = np.frombuffer(buf, np.uint8, n, at)
        chi2 = np.frombuffer(buf[at + n:at + 9 * n], np.float64)
        at += 9 * n
        r = int(i[1])
        st = dict(rounds=r, iterations=[int(k) for k in i[2:6]][:r], trials=[int(k) for k in i[6:10]][:r], lam=list(d[:4])[:r],
                  chi2=list(d[4:8])[:r])
        out.append((int(i[0]), T.copy(), flags.copy(), st, chi2.copy()))
    assert at == len(buf)
    return out


def run_program(exe, tmp_path, scenes):
    write_scenes(tmp_path / "scenes.bin", scenes)
    r = subprocess.run([str(exe), str(tmp_path / "scenes.bin"), str(tmp_path / "results.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_results(tmp_path / "results.bin", scenes)
