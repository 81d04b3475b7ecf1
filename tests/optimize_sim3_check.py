"""What the tests of orbfe_optimize_sim3* share: the scene file tests/cpp/optsim3_cpu.cpp reads, the recorded tolerances
(profiles/optimize_sim3_tolerance.txt) and THE pass condition of a result against the restatement
(tests/optimize_sim3_ref.py, analytic Jacobian, forward sums):

* bad[], n_in, rounds, n_bad, iterations and trials identical;
* every sim3_out entry within max(16 x max(s_sim3, s_cpu), 4 float32 ulps of the entry) -- the 16 and the float32 floor are
  those of the pose optimisation: the device's reduction is a third summation order, its sin / cos / exp differ
  from libm in the last place, and every consumer rounds S12 to float;
* every classification chi2 within 16 x s_chi2, relative."""
import struct
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
TOLERANCE_FILE = ROOT / "profiles" / "optimize_sim3_tolerance.txt"


def recorded():
    return {k: float(v) for k, v in (line.split("=") for line in TOLERANCE_FILE.read_text().split() if "=" in line)}


def write_scenes(path, scenes):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(scenes)))
        for sc in scenes:
            n = len(sc["x3dc1"])
            f.write(struct.pack("<iif", n, int(sc["fix_scale"]), float(sc["th2"])))
            for key in ("cam1", "cam2", "sim3_in", "x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
                f.write(np.ascontiguousarray(sc[key], np.float32).tobytes())


def read_results(path, scenes):
    """-> per scene the tuple optimize_sim3() returns: (n_in, sim3_out, bad, stats, chi2_12, chi2_21)."""
    out = []
    buf = Path(path).read_bytes()
    at = 0
    for sc in scenes:
        n = len(sc["x3dc1"])
        d = np.frombuffer(buf, np.float64, 12, at)
        i = np.frombuffer(buf, np.int32, 7, at + 96)
        at += 96 + 28
        bad = np.frombuffer(buf, np.uint8, n, at)
        c12 = np.frombuffer(buf[at + n:at + n + 8 * n], np.float64)
        c21 = np.frombuffer(buf[at + 9 * n:at + 17 * n], np.float64)
        at += 17 * n
        r = int(i[2])
        st = dict(rounds=r, n_bad=int(i[1]), iterations=[int(i[3]), int(i[4])][:r], trials=[int(i[5]), int(i[6])][:r],
                  lam=list(d[8:10])[:r], chi2=list(d[10:12])[:r])
        out.append((int(i[0]), d[:8].copy(), bad.copy(), st, c12.copy(), c21.copy()))
    assert at == len(buf)
    return out


def deviations(ref, got):
    """(largest |difference| of a sim3_out entry, largest relative difference of a classification chi2) after asserting that
    everything discrete is identical.  No pair is left out: a chi2 the reference holds as 0 must come back as 0."""
    n_in, sim3, bad, st, c12, c21 = got
    assert n_in == ref["n_in"] and st["rounds"] == ref["rounds"] and st["n_bad"] == ref["n_bad"], (n_in, st, ref["n_in"])
    assert st["iterations"] == ref["iterations"] and st["trials"] == ref["trials"], (st, ref["iterations"], ref["trials"])
    assert np.array_equal(bad, ref["bad"])
    d_sim3 = float(np.abs(np.asarray(sim3) - ref["sim3"]).max())
    d_chi2 = 0.0
    if ref["rounds"] > 0:
        for a, b in ((c12, ref["chi2_12"]), (c21, ref["chi2_21"])):
            assert np.array_equal(a[b == 0], b[b == 0])
            d_chi2 = max(d_chi2, float((np.abs(a - b)[b != 0] / np.abs(b[b != 0])).max(initial=0.0)))
    return d_sim3, d_chi2


def check(ref, got, rec=None):
    """THE pass condition; returns the deviations."""
    rec = rec or recorded()
    d_sim3, d_chi2 = deviations(ref, got)
    tol = np.maximum(16 * max(rec["s_sim3"], rec["s_cpu"]), 4 * np.spacing(np.abs(ref["sim3"]).astype(np.float32)).astype(np.float64))
    assert (np.abs(np.asarray(got[1]) - ref["sim3"]) <= tol).all(), (np.abs(np.asarray(got[1]) - ref["sim3"]), tol)
    assert d_chi2 <= 16 * rec["s_chi2"], (d_chi2, rec["s_chi2"])
    return d_sim3, d_chi2
