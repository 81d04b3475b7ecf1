"""CPU: the argument checks of the last-frame / key-frame searches on the resident map points that need no device
(csrc/mappoints_host.h: track_check_operands) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/cpp/track_host_san.cpp): every array exactly as long as the call says.  And the four entry points refuse the same
operands through the library before they touch a device."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_track_host_checks_are_right_and_clean_under_asan_and_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "track_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "track_host_san.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_the_library_refuses_bad_operands_without_a_device():
    """The checks run before the table is made ready: they answer ORBFE_ERR_INVALID on a machine without a GPU too."""
    from orb_slam2_annotate_amd import _lib
    from orb_slam2_annotate_amd._lib import ERR_INVALID, ptr
    L = _lib.load()
    mp = C.c_void_p()
    assert L.orbfe_mappoints_create(0, 128, C.byref(mp)) == 0
    try:
        n = 4
        pose = (_lib.CameraPoseC * 65)()
        for p in pose:
            p.n_levels = 8
        slot = np.array([0, 1, 2, 127], np.int32)
        octave = np.array([0, 7, 3, 1], np.int32)
        angle = np.zeros(n, np.float32)
        sf = np.ones(8, np.float32)
        th = np.full(65, 10.0, np.float32)
        od = np.full(65, 100, np.int32)
        cnt = np.zeros(65, np.int32)
        nm = C.c_int32(0)
        view = _lib.FrameViewC(n=0, min_x=0, max_x=10, min_y=0, max_y=10)
        outs = [None] * 6

        def project_last(n_, slot_, oct_, pose_=pose, levels=8, mode=0):
            return L.orbfe_project_last_frame(mp, n_, ptr(slot_), None, ptr(oct_), pose_, ptr(sf), levels, 7.0, mode, *outs)

        def search_last(n_, slot_, oct_, pose_=pose, levels=8, mode=0):
            return L.orbfe_search_last_frame_mappoints(mp, n_, ptr(slot_), None, ptr(oct_), ptr(angle), pose_, C.byref(view), ptr(sf), levels,
                                                       None, mode, 7.0, 1, None, C.byref(nm), None)

        for call in (project_last, search_last):
            assert call(n, np.array([0, 1, 2, 128], np.int32), octave) == ERR_INVALID
            assert call(n, np.array([0, -1, 2, 3], np.int32), octave) == ERR_INVALID  # -1 stays invalid
            assert call(n, None, octave) == ERR_INVALID
            assert call(n, slot, None) == ERR_INVALID
            assert call(n, slot, np.array([0, 8, 3, 1], np.int32)) == ERR_INVALID
            assert call(n, slot, np.array([0, -1, 3, 1], np.int32)) == ERR_INVALID
            assert call(n, slot, octave, pose_=None) == ERR_INVALID
            assert call(n, slot, octave, levels=5) == ERR_INVALID  # the pose predicts 8 levels, an octave is 7
            assert call(n, slot, octave, mode=3) == ERR_INVALID
            assert call(-1, slot, octave) == ERR_INVALID
            assert call(0, None, None) == 0  # nothing to do: fine, nothing touched
        assert L.orbfe_project_last_frame(None, n, ptr(slot), None, ptr(octave), pose, ptr(sf), 8, 7.0, 0, *outs) == ERR_INVALID

        def project_kf(K_, off_, slot_, pose_=pose):
            return L.orbfe_project_keyframe(mp, K_, ptr(off_), ptr(slot_), None, pose_, *outs)

        def search_kf(K_, off_, slot_, pose_=pose, levels=8):
            return L.orbfe_search_keyframe_mappoints_multi(mp, C.byref(view), ptr(sf), levels, K_, ptr(off_), ptr(slot_), None, ptr(angle),
                                                           pose_, None, ptr(th), ptr(od), 1, None, ptr(cnt))

        off = np.array([0, 3, 3, 4], np.int32)
        for call in (project_kf, search_kf):
            assert call(65, np.zeros(66, np.int32), slot) == ERR_INVALID
            assert b"64 jobs" in L.orbfe_last_error()
            assert call(-1, off, slot) == ERR_INVALID
            assert call(3, None, slot) == ERR_INVALID
            assert call(3, np.array([1, 3, 3, 4], np.int32), slot) == ERR_INVALID
            assert call(3, np.array([0, 3, 2, 4], np.int32), slot) == ERR_INVALID
            assert b"descend" in L.orbfe_last_error()
            assert call(3, off, np.array([0, 1, 2, 128], np.int32)) == ERR_INVALID
            assert call(3, off, np.array([0, 1, 2, -1], np.int32)) == ERR_INVALID
            assert call(3, off, None) == ERR_INVALID
            assert call(3, off, slot, pose_=None) == ERR_INVALID
            assert call(0, None, None) == 0 and call(3, np.zeros(4, np.int32), None) == 0  # nothing to do
        assert search_kf(3, off, slot, levels=5) == ERR_INVALID  # the poses predict 8 levels
        assert L.orbfe_project_keyframe(None, 3, ptr(off), ptr(slot), None, pose, *outs) == ERR_INVALID
    finally:
        L.orbfe_mappoints_destroy(mp)
