"""CPU: the host side of orbfe_initializer_ransac* (csrc/initializer_host.h, csrc/initializer_math.h,
include/orbfe_initializer_replay.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/cpp/initializer_host_san.cpp): every array exactly as long as the call says."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_ref as ir

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("initsan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "initializer_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "initializer_host_san.cpp"),
                    "-o", str(exe)], check=True)
    return exe


def test_initializer_host_code_is_clean_under_asan_and_ubsan(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_library_sets_from_draws_equal_the_pop_back_loop_on_random_draws(exe):
    """the library's own selection (csrc/initializer_host.h) against the literal list-pop of tests/initializer_ref.py"""
    rng = np.random.default_rng(1)
    for n, H in ((8, 40), (9, 40), (50, 200), (1000, 100)):
        d = np.stack([rng.integers(0, n - j, H) for j in range(8)], axis=1)
        d[0] = [n - 1 - j for j in range(8)]  # always the current last element
        r = subprocess.run([str(exe), "sets", str(n), str(H)], input=" ".join(str(int(v)) for v in d.reshape(-1)),
                           capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        assert np.array_equal(np.array(r.stdout.split(), np.int32).reshape(H, 8), ir.sets_from_draws(n, d)), n
    bad = subprocess.run([str(exe), "sets", "10", "1"], input="0 0 0 0 0 0 0 3", capture_output=True, text=True)
    assert bad.stdout.strip() == "refused"  # the 8th draw indexes past n - 7 = 3 entries


def test_library_normalize_equals_the_restatement(exe):
    rng = np.random.default_rng(2)
    for n in (1, 2, 333, 2000):
        xy = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1).astype(np.float32)
        r = subprocess.run([str(exe), "normalize", str(n)], input=" ".join(f"{float(v):.9g}" for v in xy.reshape(-1)),
                           capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr
        got, want = np.array(r.stdout.split(), np.float64), ir.normalize(xy)
        assert np.array_equal(got, want) or np.allclose(got, want, rtol=1e-14, atol=0), (n, got, want)
    assert subprocess.run([str(exe), "normalize", "0"], input="", capture_output=True, text=True).stdout.strip() == "refused"
