"""The kernel forms behind the result-neutral run-time switches, each against the CPU oracle.

About a dozen switches of liborbfe.so are read ONCE per process into `static` variables (csrc/*.hip: `getenv("ORBFE_...")`,
`occupancy_pad_bytes("...")`) and select another kernel, template instance or grid shape than the default launch: the
latency form of DistributeOctTree with 256 threads, the persistent-grid loops, the 128 / 256-keypoint `k_orient_desc`, the
128 x 32 blur tiles, ...  README promises that none of them changes a result.  A setting cannot change inside a process
that has already read it, so every entry of VARIANTS runs in a fresh process of its own:

    python tests/kernel_variants.py NAME      # exit 0: every frame bit-identical to the oracle; 1: first mismatch printed

Each VARIANTS entry names the environment it sets and the workload that makes the switch's code run; its docstring gives
the arithmetic that shows the code is reached.  What decides the form (csrc/): a launch of <= 8 frames per sub-batch stream
is the LATENCY form (k_octree_reg1024 / k_octree_reg, k_orient_desc<16>, the per-level blur as its own launch), more than 8
the THROUGHPUT form (k_octree, k_orient_desc<64 | 128 | 256>, the blur fused with the next resize).
tests/test_gpu_kernel_variants.py runs every entry; tests/test_kernel_variant_table.py keeps the table in step with the
switches csrc/ reads.
"""
from __future__ import annotations

import os
import sys
import time
from dataclasses import dataclass
from pathlib import Path
from typing import Callable

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

VGA = (640, 480)
KITTI = (1241, 376)
# Keypoint slots per frame = sum over the levels of (quota + 3).  1100 features on 8 levels: 1100 + 24 = 1124, not a
# multiple of 64, 128 or 256, so the last k_orient_desc workgroup of every frame is a partial one (1000 features would give
# 1024 slots, a multiple of every workgroup size).
P_BATCH = (1100, 1.2, 8, 20, 7)
P_KITTI = (2000, 1.2, 8, 20, 7)  # 2024 slots
P_VGA = (1000, 1.2, 8, 20, 7)
P_ONE_LEVEL = (700, 1.2, 1, 20, 7)  # nlevels = 1: one octree item per frame, 703 slots


class Mismatch(AssertionError):
    pass


def _fail(case, frame, field, index, detail=""):
    raise Mismatch(f"case={case} frame={frame} field={field} index={index} {detail}".rstrip())


def _first_diff(a, b):
    d = np.flatnonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))
    return int(d[0]) if d.size else -1


def compare_frame(case, frame, kps_ref, desc_ref, kps, desc):
    """Every cv::KeyPoint field bit for bit (float fields as their 32-bit patterns) and the 32 descriptor bytes of every
    keypoint; raises Mismatch at the first difference.  Returns the keypoint count."""
    if len(kps) != len(kps_ref):
        _fail(case, frame, "count", min(len(kps), len(kps_ref)), f"gpu {len(kps)} vs oracle {len(kps_ref)}")
    for name in kps_ref.dtype.names:
        i = _first_diff(np.ascontiguousarray(kps_ref[name]).view(np.uint32), np.ascontiguousarray(kps[name]).view(np.uint32))
        if i >= 0:
            _fail(case, frame, name, i, f"gpu {kps[name][i]!r} vs oracle {kps_ref[name][i]!r}")
    i = _first_diff(desc_ref, desc)
    if i >= 0:
        _fail(case, frame, "descriptor", i // 32, f"byte {i % 32}")
    return len(kps)


def compare_image(case, frame, field, ref, got):
    if ref.shape != got.shape:
        _fail(case, frame, field, -1, f"shape gpu {got.shape} vs oracle {ref.shape}")
    i = _first_diff(ref, got)
    if i >= 0:
        _fail(case, frame, field, i, f"(row {i // ref.shape[1]}, col {i % ref.shape[1]}) gpu {got.reshape(-1)[i]} vs "
                                     f"oracle {ref.reshape(-1)[i]}")


# ---------------------------------------------------------------------------------------------------------------------
# workloads
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Run:
    """What a variant does to every extractor it makes (the per-handle setter its switch needs) and what it checked."""
    setup: Callable | None = None
    blur_spec: int = 0
    frames: int = 0
    keypoints: int = 0

    def extractor(self, params, streams=1):
        import orb_slam2_annotate_amd as amd
        e = amd.ORBextractor(*params)
        e.set_streams(streams)
        if self.blur_spec:
            e.set_blur_spec(self.blur_spec)
        if self.setup:
            self.setup(e)
        return e

    def oracle(self, params):
        import oracle_lib as orc
        return orc.Oracle(*params, blur_spec=self.blur_spec)


def slot_count(e, W, H):
    """Keypoint slots per frame of the handle's pipeline for W x H (OrientDescArgs.kpSlotsPerFrame)."""
    from orb_slam2_annotate_amd import _lib
    return int(_lib.load().orbfe_extractor_max_keypoints_for(e._h, int(W), int(H)))


def check_single(run: Run, case, img, params):
    """One frame through orbfe_extract (a 1-frame launch: the latency forms): pyramid, grid candidates in emission order,
    blurred levels, keypoints and descriptors, as tests/test_gpu_extractor.py::_check_frame checks them."""
    import oracle_lib as orc
    H, W = img.shape
    o, e = run.oracle(params), run.extractor(params)
    kps_ref, desc_ref, pyr = o.extract(img, want_pyramid=True)
    kps, desc = e(img)
    levels = o.split_pyramid(pyr, W, H)
    for l, ref in enumerate(levels):
        compare_image(case, 0, f"pyramid[{l}]", ref, e.pyramid_level(l))
    for l, ref in enumerate(levels):
        xr, yr, rr = orc.grid_candidates(o, ref)
        xg, yg, rg = e.debug_candidates(l)
        if len(xr) != len(xg):
            _fail(case, 0, f"candidates[{l}].count", min(len(xr), len(xg)), f"gpu {len(xg)} vs oracle {len(xr)}")
        for name, a, b in (("x", xr, xg), ("y", yr, yg), ("response", rr, rg)):
            i = _first_diff(a.view(np.uint32), b.view(np.uint32))
            if i >= 0:
                _fail(case, 0, f"candidates[{l}].{name}", i)
    for l, ref in enumerate(levels):
        compare_image(case, 0, f"blurred[{l}]", orc.gaussian_blur7(ref, run.blur_spec), e.debug_blurred_level(l))
    run.frames += 1
    run.keypoints += compare_frame(case, 0, kps_ref, desc_ref, kps, desc)
    return len(kps)


def check_batch(run: Run, case, frames, params, streams=1, blurred=False):
    """A batch through orbfe_extract_batch on `streams` sub-batch streams.  Each stream's consecutive frames go through one
    launch per stage, so the form follows the sub-batch size -- ceil(B / streams), made even for an even B -- not B.
    blurred: every frame's blurred levels too."""
    import oracle_lib as orc
    frames = np.ascontiguousarray(frames)
    B, H, W = frames.shape
    o, e = run.oracle(params), run.extractor(params, streams)
    res = e.extract_batch(frames)
    for f in range(B):
        out = o.extract(frames[f], want_pyramid=blurred)
        if blurred:
            for l, ref in enumerate(o.split_pyramid(out[2], W, H)):
                compare_image(case, f, f"blurred[{l}]", orc.gaussian_blur7(ref, run.blur_spec), e.debug_blurred_level(l, f))
        run.keypoints += compare_frame(case, f, out[0], out[1], *res[f])
        run.frames += 1
    return e


def mixed_frames(seed, n, W=640, H=480):
    """A sequence with the edges the kernels meet in a batch: a constant frame (no keypoint, every octree item empty),
    two noise frames (every FAST cell of every level full) and a checkerboard (response ties everywhere)."""
    from orb_slam2_annotate_amd import synth
    fr = np.stack(synth.render_sequence(seed, n, W, H))
    fr[3] = synth.adversarial("constant", W, H)
    fr[7] = synth.adversarial("noise", W, H, seed=seed)
    fr[n - 2] = synth.adversarial("noise", W, H, seed=seed + 1)
    fr[n // 2] = synth.adversarial("checker", W, H, seed=seed)
    return fr


def latency_cases(run: Run):
    """Single frames and batches of <= 8 frames per stream."""
    from orb_slam2_annotate_amd import synth
    check_single(run, "kitti_1241x376_2000", synth.render_stereo(4)[0], P_KITTI)
    check_single(run, "vga_640x480_1000", synth.render_frame(1), P_VGA)
    check_single(run, "noise_min7", synth.adversarial("noise", 640, 480, seed=3), P_VGA)
    # 813 x 77: round((813 - 32) / (77 - 32)) = round(17.4) = 17 octree roots on level 0
    check_single(run, "wide_813x77_17_roots", synth.render_frame(11, 813, 77), (100, 1.1, 3, 30, 10))
    # 96 x 80: level 2 is 67 x 56, a detection rectangle of 35 x 24 px -- less than one 30-px cell row, no FAST grid on
    # levels 2..7 (empty octree items next to full ones in the same launch)
    check_single(run, "tiny_96x80", synth.render_frame(12, 96, 80), P_VGA)
    n = check_single(run, "constant", synth.adversarial("constant", 640, 480), P_VGA)
    if n != 0:
        _fail("constant", 0, "count", 0, f"{n} keypoints on a constant frame")
    seq = np.stack(synth.render_sequence(5, 8, 640, 480))
    check_batch(run, "batch3_2streams", seq[:3], P_VGA, streams=2)
    check_batch(run, "batch8", seq, P_VGA, streams=1)  # the last latency-form size


def throughput_cases(run: Run):
    """Batches of more than 8 frames per stream, with slot counts that are not a multiple of any k_orient_desc
    workgroup size (the child checks that against the library's own figure)."""
    from orb_slam2_annotate_amd import synth
    kitti = np.stack(synth.render_sequence(6, 9, *KITTI))
    e = check_batch(run, "batch9_kitti", kitti, P_KITTI)  # the first throughput size
    mixed = mixed_frames(7, 40)
    e2 = check_batch(run, "mixed40_1stream", mixed, P_BATCH, streams=1)
    for case, ext, (W, H) in (("batch9_kitti", e, KITTI), ("mixed40_1stream", e2, VGA)):
        s = slot_count(ext, W, H)
        if s % 128 == 0:
            _fail(case, -1, "workload", s, f"{s} slots per frame is a multiple of 128")
    # 8 streams: ceil(72 / 8) = 9 frames per sub-batch, rounded up to 10 (an even batch never splits a stereo pair), so one
    # call runs seven 10-frame throughput sub-batches and one 2-frame latency sub-batch side by side
    check_batch(run, "mixed72_8streams", mixed_frames(8, 72), P_BATCH, streams=8)
    check_batch(run, "one_level_533x400", np.stack(synth.render_sequence(9, 12, 533, 400)), P_ONE_LEVEL)


def blur_cases(run: Run):
    """Every blur arithmetic x both pass orders through launch_blur7_levels: the standalone blur, single frames (the
    per-level blur launch of a <= 8-frame call) and a 12-frame batch with the pyramid-blur fusion off."""
    import orb_slam2_annotate_amd as amd
    import oracle_lib as orc
    from orb_slam2_annotate_amd import synth
    try:
        for order in (1, 0):
            amd.set_blur_pass_order(order)
            for spec in (0, 1, 2):
                sub = Run(blur_spec=spec)
                tag = f"order{order}_spec{spec}"
                for (w, h) in (KITTI, (533, 400), (70, 67)):
                    for kind, img in (("noise", synth.adversarial("noise", w, h, seed=w)), ("scene", synth.render_frame(w, w, h))):
                        compare_image(f"gaussian_blur7_{w}x{h}_{kind}_{tag}", 0, "blurred",
                                      orc.gaussian_blur7(img, spec), amd.gaussian_blur7(img, spec=spec))
                check_single(sub, f"kitti_{tag}", synth.render_stereo(4 + spec)[0], P_KITTI)
                check_single(sub, f"533x400_{tag}", synth.render_frame(20 + spec, 533, 400), P_VGA)
                check_single(sub, f"70x67_{tag}", synth.render_frame(30 + spec, 70, 67), (300, 1.2, 3, 20, 7))
                sub.setup = lambda e: e.set_pyramid_blur(False)
                check_batch(sub, f"batch12_unfused_{tag}", mixed_frames(40 + spec, 12, 533, 400), P_VGA, blurred=True)
                run.frames += sub.frames
                run.keypoints += sub.keypoints
    finally:
        amd.set_blur_pass_order(1)


def pad_cases(run: Run):
    """One latency case (the resize and the per-level blur launches carry the padding) and throughput cases (the octree
    and orientation launches carry it)."""
    from orb_slam2_annotate_amd import synth
    check_single(run, "kitti_1241x376_2000", synth.render_stereo(4)[0], P_KITTI)
    check_batch(run, "batch9_kitti", np.stack(synth.render_sequence(6, 9, *KITTI)), P_KITTI)
    check_batch(run, "mixed40_1stream", mixed_frames(7, 40), P_BATCH, streams=1)


def _random_keypoints(rng, n, spread):
    x = rng.uniform(-spread, 640 + spread, n).astype(np.float32)
    y = rng.uniform(-spread, 480 + spread, n).astype(np.float32)
    octv = rng.integers(0, 8, n).astype(np.int32)
    ang = rng.uniform(0, 360, n).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return x, y, octv, ang, desc


def grid_cases(run: Run):
    """GetFeaturesInArea on host-array and resident frames (n = 1, 1000, 2300, bounds off the image) and one
    SearchByProjection per frame kind, against oracle_lib.Frame, as tests/test_gpu_projection.py runs them."""
    import orb_slam2_annotate_amd as amd
    import oracle_lib as orc
    image = (0.0, 640.0, 0.0, 480.0)
    for resident in (False, True):
        kind = "resident" if resident else "host_arrays"
        for seed, n, bounds in ((2, 1, image), (0, 1000, image), (1, 2300, (-12.5, 655.25, -8.0, 490.5))):
            case = f"features_in_area_{kind}_n{n}"
            rng = np.random.default_rng(seed)
            x, y, octv, ang, desc = _random_keypoints(rng, n, 5.0)
            F = amd.FrameView(x, y, octv, desc, bounds, angle=ang)
            if resident:
                F = F.upload()
            Fo = orc.Frame(x, y, octv, desc, bounds, angle=ang)
            nq = 400
            qx = rng.uniform(-30, 700, nq).astype(np.float32)
            qy = rng.uniform(-30, 520, nq).astype(np.float32)
            r = rng.choice(np.array([0.5, 3.0, 15.0, 64.0, 900.0], np.float32), nq)
            lv = np.array([(-1, -1), (0, -1), (2, -1), (0, 3), (1, 2), (3, 1)], np.int32)[rng.integers(0, 6, nq)]
            got = F.GetFeaturesInArea(qx, qy, r, lv[:, 0], lv[:, 1], capacity=16)
            for q in range(nq):
                want = Fo.features_in_area(qx[q], qy[q], r[q], lv[q, 0], lv[q, 1])
                if got[q].tolist() != want.tolist():
                    _fail(case, 0, "indices", q, f"gpu {got[q].tolist()[:8]} vs oracle {want.tolist()[:8]}")
            run.frames += 1
        # SearchByProjection(Frame&, vector<MapPoint*>&, th) looks its windows up in the same grid
        case = f"search_by_projection_{kind}"
        rng = np.random.default_rng(10)
        nf, n_mp = 1500, 2500
        x, y, octv, ang, desc = _random_keypoints(rng, nf, 0.0)
        F = amd.FrameView(x, y, octv, desc, image, angle=ang)
        if resident:
            F = F.upload()
        Fo = orc.Frame(x, y, octv, desc, image, angle=ang)
        src = rng.integers(0, nf, n_mp)
        px = (x[src] + rng.normal(0, 1.5, n_mp)).astype(np.float32)
        py = (y[src] + rng.normal(0, 1.5, n_mp)).astype(np.float32)
        flip = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8) & rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
        md = desc[src] ^ flip
        sf = (1.2 ** np.arange(8)).astype(np.float32)
        level = np.clip(octv[src] + rng.integers(0, 2, n_mp), 0, 7).astype(np.int32)
        in_view = (rng.random(n_mp) < 0.85).astype(np.uint8)
        view_cos = rng.uniform(0.99, 1.0, n_mp).astype(np.float32)
        blocked = (rng.random(nf) < 0.1).astype(np.uint8)
        obs = (rng.random(n_mp) < 0.9).astype(np.uint8)
        n_ref, ref = orc.search_by_projection_mappoints(Fo, sf, blocked, in_view, level, view_cos, px, py, None, md, obs,
                                                        1.0, 0.8)
        n_got, got = amd.ORBmatcher(0.8, True).SearchByProjection(F, sf, in_view, level, view_cos, px, py, md, th=1.0,
                                                                  blocked=blocked, mp_obs_positive=obs)
        if n_got != n_ref:
            _fail(case, 0, "nmatches", -1, f"gpu {n_got} vs oracle {n_ref}")
        i = _first_diff(ref, got)
        if i >= 0:
            _fail(case, 0, "match", i)
        if n_ref < 300:
            _fail(case, 0, "workload", -1, f"only {n_ref} matches")
        run.frames += 1


# ---------------------------------------------------------------------------------------------------------------------
# the table: one entry per switch value
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Variant:
    name: str
    env: dict
    workload: Callable  # (Run) -> None; raises Mismatch
    setup: Callable | None = None  # per-handle setter the switch needs
    doc: str = ""


VARIANTS: dict[str, Variant] = {}


def variant(name, env, setup=None):
    """Registers the decorated workload under `name`; its docstring is the reason the switch's code is reached."""
    def deco(fn):
        VARIANTS[name] = Variant(name, dict(env), fn, setup, (fn.__doc__ or "").strip())
        return fn
    return deco


def octree_item_cases(run: Run, count=300):
    """`count` small candidate sets of tests/octree_edges.py as the frames of ONE k_octree launch (form 1 of
    orbfe_debug_octree_device), each frame against the oracle's DistributeOctTree in the reference's list order."""
    import octree_edges as oe
    import oracle_lib as orc
    from orb_slam2_annotate_amd.extractor import debug_octree_device
    items = oe.small_items(count)
    minX, _, minY, _ = oe.AREA
    got = debug_octree_device(items, *oe.AREA, oe.NEIGHBOUR_N, form=1)
    answers = {}
    for f, ((xs, ys, rs), res) in enumerate(zip(items, got)):
        key = (xs.tobytes(), ys.tobytes(), rs.tobytes())
        if key not in answers:
            answers[key] = orc.distribute_octtree(xs, ys, rs, *oe.AREA, oe.NEIGHBOUR_N)
        idx = answers[key]
        if res["count"] != len(idx):
            _fail("octree_items", f, "count", min(res["count"], len(idx)), f"gpu {res['count']} vs oracle {len(idx)}")
        o = np.argsort(res["rank"][:len(idx)], kind="stable")
        for name, a, b in (("x", xs[idx] + minX, res["x"][:len(idx)][o]), ("y", ys[idx] + minY, res["y"][:len(idx)][o]),
                           ("response", rs[idx], res["resp"][:len(idx)][o])):
            i = _first_diff(np.asarray(a, np.int64), np.asarray(b, np.int64))
            if i >= 0:
                _fail("octree_items", f, name, i, f"gpu {b[i]} vs oracle {a[i]}")
        run.frames += 1
        run.keypoints += len(idx)


@variant("octree_t256", {"ORBFE_OCTREE_T": "256"})
def _octree_t256(run):
    """launch_octree: a launch of <= 8 frames is the latency form, and with 256 threads it is k_octree_reg
    (dim3(levels, frames)) instead of k_octree_reg1024.  octree_gathers() is false unless the latency form has 1024
    threads, so every latency case also runs the separate k_gather_candidates launch.  Level 0 of the 1241 x 376 /
    2000-feature frame lists ~5000 candidates > 256 x kRegCand (16) = 4096: k_octree_reg takes its global-memory branch
    there and its register branch on the smaller levels."""
    latency_cases(run)


@variant("octree_gather0", {"ORBFE_OCTREE_GATHER": "0"})
def _octree_gather0(run):
    """octree_gathers() is false: the <= 8-frame launches run k_gather_candidates and then k_octree_reg1024 with
    gCells = NULL, which reads the gathered candidates instead of compacting its own level."""
    latency_cases(run)


@variant("octree_grid1", {"ORBFE_OCTREE_GRID": "1"})
def _octree_grid1(run):
    """k_octree's persistent loop: 1 workgroup per CU = a grid of 256.  mixed40_1stream launches 40 frames x 8 levels =
    320 (frame, level) items > 256 workgroups, so workgroups 0..63 take a second item (it = blockIdx.x + 256).  The other
    throughput launches (9 x 8 = 72 items, 10 x 8 per sub-batch of the 8-stream call, 12 x 1) stay below the grid:
    one item each.  octree_item_cases adds ONE launch of form 1 (k_octree) over 300 small candidate sets = 300 one-level
    (frame, level) items > 256: workgroups 0..43 take a second item, each next to other sets than in the launch above."""
    throughput_cases(run)
    octree_item_cases(run)


@variant("orient_kpb128", {"ORBFE_ORIENT_KPB": "128"})
def _orient_kpb128(run):
    """k_orient_desc<128, ...> for every launch of > 8 frames.  Slots per frame: 2024 (KITTI) = 15 x 128 + 104, 1124
    (VGA / 1100 features) = 8 x 128 + 100, 703 (one level) = 5 x 128 + 63: the last workgroup of every frame is partial."""
    throughput_cases(run)


@variant("orient_kpb256", {"ORBFE_ORIENT_KPB": "256"})
def _orient_kpb256(run):
    """k_orient_desc<256, ...> for every launch of > 8 frames.  Slots per frame 2024 = 7 x 256 + 232, 1124 = 4 x 256 +
    100, 703 = 2 x 256 + 191: the last workgroup of every frame is partial."""
    throughput_cases(run)


@variant("orient_grid1", {"ORBFE_ORIENT_GRID": "1"})
def _orient_grid1(run):
    """k_orient_desc's persistent loop with the grid forced to 1 workgroup per CU = 256 (a one-stream launch has no cap
    without the switch): mixed40_1stream has ceil(1124 / 64) = 18 items per frame x 40 frames = 720 > 256, so a workgroup
    walks up to ceil(90 / 32) = 3 items of its XCD's chunk; batch9_kitti has 32 x 9 = 288 > 256."""
    throughput_cases(run)


@variant("orient_interleave0", {"ORBFE_ORIENT_INTERLEAVE": "0"})
def _orient_interleave0(run):
    """k_orient_desc with consecutive keypoint slots per wave (4 in the latency form, 16 in the throughput form) instead
    of slots w, w + 4, w + 8, ...: both forms, so the latency and the throughput cases."""
    latency_cases(run)
    throughput_cases(run)


@variant("desc_tiles_grid1", {"ORBFE_DESC_TILES_GRID": "1"}, setup=lambda e: e.set_desc_tiles(True))
def _desc_tiles_grid1(run):
    """k_orient_desc_tiles (set_desc_tiles(True) on every handle) with its persistent grid at 1 workgroup per CU = 256:
    level 0 of a VGA frame alone has 5 x 4 tiles of 128 x 128, so the 40-frame launch has > 800 tile items > 256 and
    every workgroup loops; the single frames and small batches run the same kernel one item per workgroup."""
    latency_cases(run)
    throughput_cases(run)


@variant("blur_tile128x32", {"ORBFE_BLUR_TILE": "1"})
def _blur_tile(run):
    """launch_blur7_levels -> launch_blur_tiles<128, 32>, i.e. k_blur7<spec, 128, 32, false, hfirst> for spec 0 / 1 / 2
    and both pass orders: the standalone blur always, an extraction whenever the blur is its own launch -- a call of <= 8
    frames (the pyramid-blur fusion only runs above 8) or set_pyramid_blur(False).  1241 = 9 x 128 + 89, 376 = 11 x 32 + 24,
    533 = 4 x 128 + 21, 400 = 12 x 32 + 16, 70 < 128, 67 = 2 x 32 + 3: partial tiles on both axes."""
    blur_cases(run)


@variant("pad_4kb", {"ORBFE_PAD_RESIZE": "4", "ORBFE_PAD_BLUR": "4", "ORBFE_PAD_OCTREE": "4", "ORBFE_PAD_ORIENT": "4"})
def _pad(run):
    """4 KB of dynamic LDS on each of the four launches that take it: the single frame runs k_resize_flat (RESIZE) and the
    per-level blur (BLUR); the 9- and 40-frame launches run k_octree (OCTREE, throughput form only) and k_orient_desc<64>
    (ORIENT, throughput form only)."""
    pad_cases(run)


def grid_edge_cases(run: Run):
    """The engineered grid and window cases of tests/window_edges.py (key points on half cells, on the bounds, at -0.0f;
    windows on cell boundaries, clamped, outside the grid; |dx| == r) in the sparse, crowded-cell and n > 8192 frame forms,
    on host-array and resident frames."""
    import orb_slam2_annotate_amd as amd
    import window_edges as we
    for c in we.area_cases():
        ref = we.run_oracle(c)[0]
        for form in ("sparse", "crowded", "large"):
            for resident in (False, True):
                got = we.run_gpu(amd, we.padded_case(c, form), resident)
                if got != ref:
                    q = next(i for i, (g, r) in enumerate(zip(got[0], ref[0])) if g != r)
                    _fail(f"{c.name}_{form}_{'resident' if resident else 'host_arrays'}", 0, "indices", q,
                          f"gpu {got[0][q][:8]} vs oracle {ref[0][q][:8]}")
                run.frames += 1


@variant("grid_sort1", {"ORBFE_GRID_SORT": "1"})
def _grid_sort(run):
    """launch_grid_build: k_grid_build (the bitonic sort) for every frame instead of k_grid_build_count, which otherwise
    runs for every n <= 8192 -- all of n = 1, 1000, 2300 and the 1500-keypoint projection frame, and the grid-edge frames
    of tests/window_edges.py (21 key points; 91 with a crowded cell)."""
    grid_cases(run)
    grid_edge_cases(run)


def run_variant(name: str) -> int:
    """The variant's workload in THIS process; its switches must be in the environment before the library first reads
    them (main() sets them)."""
    v = VARIANTS[name]
    run = Run(setup=v.setup)
    t0 = time.time()
    try:
        v.workload(run)
    except Mismatch as m:
        print(f"MISMATCH variant={name} {m}", flush=True)
        return 1
    print(f"parity ok: variant={name} {run.frames} frames / queries, {run.keypoints} keypoints bit-identical to the "
          f"oracle ({time.time() - t0:.1f} s)", flush=True)
    return 0


def child_env(name: str, base=None) -> dict:
    env = dict(os.environ if base is None else base)
    env.update(VARIANTS[name].env)
    return env


def main(argv) -> int:
    if len(argv) != 2 or argv[1] not in VARIANTS:
        print(f"usage: {argv[0]} NAME  (NAME in {', '.join(VARIANTS)})", file=sys.stderr)
        return 2
    os.environ.update(VARIANTS[argv[1]].env)  # before liborbfe.so is loaded: it reads every switch after this point
    return run_variant(argv[1])


if __name__ == "__main__":
    sys.exit(main(sys.argv))
