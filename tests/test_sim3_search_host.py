"""CPU: the argument checks of ComputeSim3's two searches on the resident map points that need no device
(csrc/mappoints_host.h: sim3_check_legs, sim3_check_search) as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/cpp/sim3_search_host_san.cpp): every array exactly as long as the call says.  And the three entry points
refuse the same operands through the library before they touch a device."""
import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


def test_sim3_search_host_checks_are_right_and_clean_under_asan_and_ubsan(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++")
    assert cxx, "no hipcc / clang++ to build the sanitizer program with"
    exe = tmp_path / "sim3_search_host_san"
    flags = ["-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
    subprocess.run([cxx, *flags, "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "sim3_search_host_san.cpp"), "-o", str(exe)], check=True)
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
        legs = (_lib.Sim3LegC * 129)()
        for leg in legs:
            leg.n_levels = 8
        bad_legs = (_lib.Sim3LegC * 3)()
        for leg in bad_legs:
            leg.n_levels = 8
        bad_legs[1].n_levels = 65
        slot = np.array([0, -1, 2, 127], np.int32)
        off = np.array([0, 3, 3, 4], np.int32)
        sf = np.ones(8, np.float32)
        outs = [None] * 5

        def project(n_, off_, slot_, legs_=legs):
            return L.orbfe_project_sim3(mp, n_, ptr(off_), ptr(slot_), None, legs_, *outs)

        assert project(129, np.zeros(130, np.int32), slot) == ERR_INVALID
        assert b"128 legs" in L.orbfe_last_error()
        assert project(-1, off, slot) == ERR_INVALID
        assert project(3, None, slot) == ERR_INVALID
        assert project(3, np.array([1, 3, 3, 4], np.int32), slot) == ERR_INVALID
        assert project(3, np.array([0, 3, 2, 4], np.int32), slot) == ERR_INVALID
        assert b"descend" in L.orbfe_last_error()
        assert project(3, off, np.array([0, 1, 2, 128], np.int32)) == ERR_INVALID
        assert project(3, off, np.array([0, 1, 2, -2], np.int32)) == ERR_INVALID  # below -1
        assert project(3, off, None) == ERR_INVALID
        assert project(3, off, slot, legs_=None) == ERR_INVALID
        assert project(3, off, slot, legs_=bad_legs) == ERR_INVALID
        assert project(0, None, None) == 0 and project(3, np.zeros(4, np.int32), None) == 0  # nothing to do
        assert L.orbfe_project_sim3(None, 3, ptr(off), ptr(slot), None, legs, *outs) == ERR_INVALID

        # the multi search: KF1 with 4 keypoints, K = 2 candidates of 2 and 1 keypoints (host views without arrays would be bad
        # views, so the views carry real arrays)
        def view(n):
            a = dict(x=np.full(n, 5, np.float32), y=np.full(n, 5, np.float32), octave=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8))
            v = _lib.FrameViewC(n=n, x=a["x"].ctypes.data, y=a["y"].ctypes.data, octave=a["octave"].ctypes.data, desc=a["desc"].ctypes.data,
                                min_x=0, max_x=10, min_y=0, max_y=10)
            return v, a

        (v1, k1), (v2a, k2a), (v2b, k2b) = view(4), view(2), view(1)
        views = (C.POINTER(_lib.FrameViewC) * 2)(C.pointer(v2a), C.pointer(v2b))
        off2 = np.array([0, 2, 3], np.int32)
        slot2 = np.array([1, -1, 2], np.int32)
        match = np.zeros(8, np.int32)
        cnt = np.zeros(2, np.int32)

        def multi(K_=2, slot1_=slot, off2_=off2, slot2_=slot2, l12=legs, l21=legs, matched=None, levels=8, mp_=mp, views_=views,
                  sf1=sf, match_=match, cnt_=cnt):
            return L.orbfe_search_by_sim3_mappoints_multi(mp_, None, C.byref(v1), ptr(slot1_), K_, views_, ptr(off2_), ptr(slot2_), l12, l21,
                                                          ptr(matched), None, None, ptr(sf1), ptr(sf), levels, 7.5, ptr(match_), ptr(cnt_))

        assert multi(K_=65) == ERR_INVALID
        assert b"64 candidates" in L.orbfe_last_error()
        assert multi(K_=-1) == ERR_INVALID
        assert multi(slot1_=np.array([0, -2, 2, 127], np.int32)) == ERR_INVALID
        assert multi(slot1_=np.array([0, 1, 2, 128], np.int32)) == ERR_INVALID
        assert multi(slot1_=None) == ERR_INVALID
        assert multi(off2_=None) == ERR_INVALID
        assert multi(off2_=np.array([1, 2, 3], np.int32)) == ERR_INVALID
        assert multi(off2_=np.array([0, 2, 1], np.int32)) == ERR_INVALID
        assert multi(off2_=np.array([0, 1, 3], np.int32)) == ERR_INVALID  # not KF2->n entries per candidate
        assert multi(slot2_=None) == ERR_INVALID
        assert multi(slot2_=np.array([1, -1, 128], np.int32)) == ERR_INVALID
        assert multi(l12=None) == ERR_INVALID and multi(l21=None) == ERR_INVALID
        assert multi(l21=bad_legs) == ERR_INVALID
        assert multi(matched=np.array([-1, 0, 5, -1, -1, -1, -1, 128], np.int32)) == ERR_INVALID
        assert multi(matched=np.array([-1, 0, 5, -1, -1, -1, -1, -2], np.int32)) == ERR_INVALID
        assert multi(levels=0) == ERR_INVALID and multi(levels=65) == ERR_INVALID
        assert multi(levels=5) == ERR_INVALID  # the legs predict 8 levels
        assert multi(mp_=None) == ERR_INVALID
        assert multi(views_=None) == ERR_INVALID and multi(sf1=None) == ERR_INVALID
        assert multi(match_=None) == ERR_INVALID and multi(cnt_=None) == ERR_INVALID
        assert multi(K_=0) == 0  # nothing to do

        # the projection form
        pose = _lib.CameraPoseC()
        pose.n_levels = 8
        nm = C.c_int32(0)
        pslot = np.array([0, 1, 2, 127], np.int32)
        m4 = np.zeros(4, np.int32)

        def proj(n_=4, slot_=pslot, pose_=C.byref(pose), levels=8, mp_=mp, sf_=sf, match_=m4, nm_=C.byref(nm)):
            return L.orbfe_search_by_projection_sim3_mappoints(mp_, n_, ptr(slot_), None, pose_, C.byref(v1), ptr(sf_), levels, None, 10.0,
                                                               ptr(match_), nm_, None)

        assert proj(slot_=np.array([0, -1, 2, 3], np.int32)) == ERR_INVALID  # vpPoints holds no NULL
        assert proj(slot_=np.array([0, 1, 2, 128], np.int32)) == ERR_INVALID
        assert proj(slot_=None) == ERR_INVALID and proj(n_=-1) == ERR_INVALID
        assert proj(pose_=None) == ERR_INVALID
        assert proj(levels=5) == ERR_INVALID and proj(levels=0) == ERR_INVALID
        assert proj(mp_=None) == ERR_INVALID and proj(sf_=None) == ERR_INVALID
        assert proj(match_=None) == ERR_INVALID and proj(nm_=None) == ERR_INVALID
        m4[:] = 9
        assert proj(n_=0, slot_=None) == 0 and (m4 == -1).all()  # empty input: fine, outputs cleared
        del k1, k2a, k2b
    finally:
        L.orbfe_mappoints_destroy(mp)
