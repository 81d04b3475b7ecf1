"""CPU: the host layers of the three RANSAC solvers (sim3_host.h, pnp_host.h, initializer_host.h) text for text against the
answers pinned in tests/golden/ransac_host_pins.txt, which were taken before their shared parts were moved onto
csrc/ransac_host.h: every refusal of sim3_check, pnp_check_common + pnp_check_sets and init_check with the text it returns,
calls with two faults (which one is named), the accepted edge cases, the layouts (word_off, every record field, the owner of
every item) and the selections without replacement for S = 3, 4 and 8."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
FIXTURE = ROOT / "tests" / "golden" / "ransac_host_pins.txt"
FUNCTIONS = {f"{s}_{f}" for s in ("sim3", "pnp", "init") for f in ("check", "layout")} | {"draws3", "draws4", "draws8"}


def read_fixture():
    cases, outs = [], []
    for line in FIXTURE.read_text().splitlines():
        f = line.split()
        if f and f[0] == "case":
            cases.append((f[1], f[2]))
        elif f and f[0] == "out":
            outs.append(line)
    assert len(cases) == len(outs) and cases
    return cases, outs


@pytest.fixture(scope="module")
def computed(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    tmp = tmp_path_factory.mktemp("ransac_host")
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "ransac_host_pins.cpp"), "-o", str(tmp / "ransac_host_pins")],
                   check=True)
    subprocess.run([str(tmp / "ransac_host_pins"), str(FIXTURE), str(tmp / "out.txt")], check=True, timeout=60)
    return (tmp / "out.txt").read_text().splitlines()


def test_the_fixture_has_every_function_and_every_kind_of_case():
    cases, outs = read_fixture()
    assert {f for f, _ in cases} == FUNCTIONS
    for solver in ("sim3", "pnp", "init"):
        names = {name for f, name in cases if f == f"{solver}_check"}
        answers = {out for (f, _), out in zip(cases, outs) if f == f"{solver}_check"}
        assert sum(name.startswith("two_") for name in names) >= 4
        assert {"fine_k0", "fine_owner_without_sets", "fine_n32", "fine_n33", "fine_n64"} <= names
        assert "out more than 2^31 - 1 mask words" in answers and "out fine" in answers
    for S in (3, 4, 8):
        names = {name for f, name in cases if f == f"draws{S}"}
        assert {f"fine_n{S}"} <= {name for f, name in cases if f.endswith("_check")}
        assert {"all_zero", "all_last", "same_draw_twice", f"random_n{S}", f"random_n{S + 1}", "random_n50"} <= names
        assert {f"refuse_negative_at_{i}" for i in range(S)} | {f"after_refuse_size_at_{i}" for i in range(S)} <= names


def test_every_answer_equals_the_pinned_one(computed):
    cases, pinned = read_fixture()
    assert len(computed) == len(pinned)
    bad = [(f, name, want[:120], got[:120]) for (f, name), want, got in zip(cases, pinned, computed) if want != got]
    assert not bad, f"answers that differ from tests/golden/ransac_host_pins.txt (function, case, pinned, computed): {bad}"
