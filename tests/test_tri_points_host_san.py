"""CPU: the host side of triangulated-point creation (csrc/tripoints_host.h) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/cpp/tripoints_host_san.cpp): the definition on the engineered inputs of
tests/tri_points_ref.py on exactly-sized buffers, the capacity rule and every refused input."""
import os
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_tripoints_host_code_is_clean_under_asan_and_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "tripoints_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "tripoints_host_san.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
