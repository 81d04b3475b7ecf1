"""CPU: the host side of orbfe_initializer_reconstruct* (csrc/initializer_host.h, csrc/initializer_reconstruct_math.h,
include/orbfe_initializer_replay.hpp) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/cpp/initializer_reconstruct_host_san.cpp): every array exactly as long as the call says."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp_path = tmp_path_factory.mktemp("reconsan")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "initializer_reconstruct_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "initializer_reconstruct_host_san.cpp"), "-o", str(exe)], check=True)
    return exe


def test_reconstruct_host_code_is_clean_under_asan_and_ubsan(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
