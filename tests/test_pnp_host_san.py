"""CPU: the host side of orbfe_pnp_* (csrc/pnp_host.h, csrc/pnp_math.h, include/orbfe_pnp_replay.hpp) as a stand-alone program
under the address and undefined-behaviour sanitizers (tests/cpp/pnp_host_san.cpp): every ORBFE_ERR_INVALID case, the layout,
the record scan, the compaction, and the replay of iterate() on hand-made count sequences, every array exactly as long as the
call says."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pnp_ref as pr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("pnpsan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "pnp_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "pnp_host_san.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_pnp_host_code_is_clean_under_asan_and_ubsan(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_library_sets_from_draws_equal_the_list_pop_on_random_draws(exe):
    rng = np.random.default_rng(1)
    for n, H in ((50, 200), (4, 40), (5, 40), (1000, 100)):
        d = np.stack([rng.integers(0, n - i, H) for i in range(4)], axis=1)
        r = subprocess.run([str(exe), "draws", str(n), str(H)], input=" ".join(str(int(v)) for v in d.reshape(-1)),
                           capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        assert np.array_equal(np.array(r.stdout.split(), np.int32).reshape(H, 4), pr.sets_from_draws(n, d)), n
    bad = subprocess.run([str(exe), "draws", "7", "1"], input="0 0 0 4", capture_output=True, text=True)
    assert bad.stdout.strip() == "refused"  # the fourth draw indexes a list of 4


def test_replay_ransac_parameters_equal_the_restatement_on_a_grid(exe):
    cases = [(n, p, mi, mx, e) for n in list(range(0, 130)) + [500, 5000, 10 ** 6] for p in (0.99,) for mi in (4, 8, 10, 50)
             for mx in (1, 10, 300) for e in (0.1, 0.4, 0.5, 0.9, 1.0)]
    r = subprocess.run([str(exe), "params"], input="\n".join(f"{n} {p} {mi} {mx} {e}" for n, p, mi, mx, e in cases),
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    got = np.array(r.stdout.split(), np.int64).reshape(-1, 2).tolist()
    want = [list(pr.set_ransac_parameters(n, p, mi, mx, 4, e)[:2]) for n, p, mi, mx, e in cases]
    assert got == want
