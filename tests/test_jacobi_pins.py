"""CPU: the seven eigen / SVD routines of the solver math (tri_null_vector, sim3_top_eigenvector, init_null_vector with
InitHostLanes, init_rank2, recon_svd3, pnp_ls6 for m = 3, 4, 5, pnp_eig12) bit for bit against the outputs pinned in
tests/golden/jacobi_pins.txt, which were taken before the routines were moved onto csrc/jacobi_math.h.  No tolerance: the
routines use only + - * /, sqrt and fabs under -ffp-contract=off.  A case whose name begins with one_nan has a NaN in its input: there
only which outputs are NaN is compared (the payload may differ), and that the program ends."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "jacobi_pins.txt"
ROUTINES = {"tri", "sim3", "null9", "rank2", "svd3", "ls6", "eig12"}


def is_nan(word):
    b = int(word, 16)
    return (b >> 52) & 0x7FF == 0x7FF and b & ((1 << 52) - 1) != 0


def read_fixture():
    cases, outs = [], []
    for line in FIXTURE.read_text().splitlines():
        f = line.split()
        if f and f[0] == "case":
            cases.append((f[1], f[2]))
        elif f and f[0] == "out":
            outs.append(f[1:])
    assert len(cases) == len(outs) and cases
    return cases, outs


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    tmp = tmp_path_factory.mktemp("jacobi")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "jacobi_pins.cpp"), "-o", str(tmp / "jacobi_pins")],
                   check=True)
    subprocess.run([str(tmp / "jacobi_pins"), str(FIXTURE), str(tmp / "out.txt")], check=True, timeout=60)  # it ends, NaN or not
    return [line.split()[1:] for line in (tmp / "out.txt").read_text().splitlines()]


def test_the_fixture_has_every_routine_and_a_nan_case_for_each():
    cases, _ = read_fixture()
    assert {r for r, _ in cases} == ROUTINES
    assert {r for r, name in cases if name.startswith("one_nan")} == ROUTINES
    assert {name for r, name in cases if r == "ls6" and name.startswith("random")} == {"random_m3", "random_m4", "random_m5"}


def test_every_output_bit_equals_the_pinned_one(computed):
    cases, pinned = read_fixture()
    assert len(computed) == len(pinned)
    bad = []
    for (routine, name), want, got in zip(cases, pinned, computed):
        assert len(got) == len(want), (routine, name)
        if name.startswith("one_nan"):
            same = [is_nan(w) for w in want] == [is_nan(g) for g in got]
        else:
            same = want == got
        if not same:
            bad.append((routine, name, [i for i, (w, g) in enumerate(zip(want, got)) if w != g]))
    assert not bad, f"outputs that differ from tests/golden/jacobi_pins.txt (routine, case, value indices): {bad}"
