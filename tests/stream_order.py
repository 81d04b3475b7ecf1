"""The ordering between liborbfe.so's streams, one deterministic case per cross-stream wait.

The library runs on several kinds of stream: an extractor handle's stream 0, its sub-batch / lane streams extra[], the
H2D / D2H copy streams of the pipelined host path, and one matcher stream per calling thread.  Correct results depend on
the hipStreamWaitEvent / hipEventSynchronize calls between them, but the kernels that race are microseconds long, so a
missing wait seldom shows.  Each case here holds the upstream stream back with the library's test hook
(orbfe_debug_stall_*: a one-wave kernel that waits on the clock and writes nothing), so the racing work would overtake it
for a fifth of a second if the wait were missing:

    python tests/stream_order.py NAME      # exit 0 and "order ok": every output equal to the oracle; 1: first mismatch

Every case that races two streams first proves that its window is open: it stalls the upstream stream, enqueues a marker
(a zero-length stall) on the racing stream, and requires the marker to finish while the stall is still running
(staging_reuse races the host against a stream: it checks that the host runs ahead of the held stream;
stale_output_block is not a race and holds nothing back).  Two streams bound to one hardware
queue may not overtake each other, so the children run with GPU_MAX_HW_QUEUES=16 (child_env).  If the marker does not
finish first the case fails with "window closed" -- it never passes without the window.  The case then runs the real calls
behind the same stall and compares every output with the CPU oracle (extractor outputs, stereo matches) or with a twin
uploaded from host arrays (resident frames).  Every buffer involved is primed with a complete earlier result of the same
geometry and capacity, so a missing wait makes a kernel read another complete, valid result, never uninitialised or freed
memory.

CASES maps each case to the wait sites it pins; NOT_CASED lists the sites no case pins, with the reason.  A site key is
"file:function:call(arguments)" with the arguments whitespace-normalised and hipStreamWaitEvent's flags dropped
(tests/test_stream_order_table.py keeps both lists in step with csrc/).  tests/test_gpu_stream_order.py runs every case.
"""
from __future__ import annotations

import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path
from typing import Callable

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

STALL_US = 200_000       # how long the upstream stream is held back
GPU_MAX_HW_QUEUES = "16"  # the project's own value: every stream of a case on a hardware queue of its own
P_VGA = (1000, 1.2, 8, 20, 7)
P_STEREO = (800, 1.2, 8, 20, 7)


class Mismatch(AssertionError):
    pass


class WindowClosed(AssertionError):
    pass


@dataclass
class Case:
    run: Callable[[], None]
    pins: list = field(default_factory=list)  # site keys (see the module docstring)
    bug: str = ""                             # the ordering bug the case was written for, if any


def child_env(name: str | None = None) -> dict:
    env = dict(os.environ)
    env["GPU_MAX_HW_QUEUES"] = GPU_MAX_HW_QUEUES
    return env


# ---- helpers ----------------------------------------------------------------------------------------------------------
def _amd():
    import orb_slam2_annotate_amd as amd
    return amd


def _wait(pred, timeout_s):
    t_end = time.monotonic() + timeout_s
    while not pred():
        if time.monotonic() > t_end:
            return False
        time.sleep(0.0002)
    return True


def prove_window(case, stall, marker, upstream_idle, racing_idle):
    """stall(usec) holds the upstream stream back, marker(0) enqueues a zero-length stall on the racing stream: the marker
    must complete while the stall is still running, or the case cannot show anything."""
    stall(STALL_US)
    marker(0)
    if not _wait(racing_idle, 0.8 * STALL_US / 1e6):
        raise WindowClosed(f"case={case}: window closed (the marker on the racing stream did not finish while the "
                           "upstream stream was stalled)")
    if upstream_idle():
        raise WindowClosed(f"case={case}: window closed (the stall ended before the marker was seen)")
    if not _wait(upstream_idle, 10.0):
        raise WindowClosed(f"case={case}: the stall did not end")


def prove_host_ahead(case, stall, upstream_idle):
    """For a race between the host and a stream: the call after the stall returns while the stream is still busy."""
    stall(STALL_US)
    if upstream_idle():
        raise WindowClosed(f"case={case}: window closed (the stream was idle right after the stall was enqueued)")
    if not _wait(upstream_idle, 10.0):
        raise WindowClosed(f"case={case}: the stall did not end")


def _first_diff(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return -2
    d = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
    return int(d[0]) if d.size else -1


def expect_equal(case, what, ref, got):
    i = _first_diff(ref, got)
    if i == -2:
        raise Mismatch(f"case={case} {what}: shape {np.asarray(got).shape} vs {np.asarray(ref).shape}")
    if i >= 0:
        raise Mismatch(f"case={case} {what}: first difference at flat index {i}: "
                       f"{np.asarray(got).reshape(-1)[i]!r} vs {np.asarray(ref).reshape(-1)[i]!r}")


def expect_records(case, what, kr, dr, kps, desc):
    from kernel_variants import compare_frame
    try:
        compare_frame(case, what, kr, dr, kps, desc)
    except AssertionError as m:
        raise Mismatch(str(m)) from None


_ORACLES = {}


def oracle(params, img, want_pyramid=False):
    import oracle_lib as orc
    key = (params, img.tobytes(), want_pyramid)
    if key not in _ORACLES:
        _ORACLES[key] = orc.Oracle(*params).extract(img, want_pyramid=want_pyramid)
    return _ORACLES[key]


def nodes_of(n, seed):
    """A synthetic FeatureVector assignment: feature i -> one of 40 sparse node ids."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 40, n).astype(np.uint32) * 7 + 3)


def view_of(kps, desc, w=640, h=480):
    amd = _amd()
    return amd.FrameView(kps["x"], kps["y"], kps["octave"], desc, (0.0, float(w), 0.0, float(h)), angle=kps["angle"])


class Probe:
    """What a resident frame answers, against its twin uploaded from host arrays: SearchByBoW with the twin as the key frame
    (descriptors, angles, index list) and GetFeaturesInArea on 64 windows (positions, octaves, grid)."""

    def __init__(self, seed=5, w=640, h=480):
        amd = _amd()
        self.rng = np.random.default_rng(seed)
        self.qx = self.rng.uniform(0, w, 64).astype(np.float32)
        self.qy = self.rng.uniform(0, h, 64).astype(np.float32)
        self.qr = self.rng.uniform(5, 60, 64).astype(np.float32)
        self.m = amd.ORBmatcher(0.8, True)

    def _ask(self, twin, has, R):
        n, match = self.m.SearchByBoWResident(twin, has, R)
        area = [a.tolist() for a in R.GetFeaturesInArea(self.qx, self.qy, self.qr)]
        return n, np.asarray(match).copy(), area

    def expect(self, case, what, twin, R):
        has = (self.rng.random(twin.N) < 0.8).astype(np.uint8)
        n0, m0, a0 = self._ask(twin, has, twin)
        n1, m1, a1 = self._ask(twin, has, R)
        if n0 < 20:
            raise Mismatch(f"case={case} {what}: the probe matches only {n0} features (too few to tell frames apart)")
        expect_equal(case, f"{what} SearchByBoW matches", m0, m1)
        if a0 != a1:
            k = next(i for i in range(len(a0)) if a0[i] != a1[i])
            raise Mismatch(f"case={case} {what}: GetFeaturesInArea window {k}: {a1[k][:8]} vs {a0[k][:8]}")


def _frames(seed, n, w=640, h=480):
    from orb_slam2_annotate_amd import synth
    return [synth.render_frame(seed + i, w, h) for i in range(n)]


# ---- cases ------------------------------------------------------------------------------------------------------------
def frame_build_vs_next_extract():
    """orbfe_frame_from_extractor(A) builds a resident frame from the handle's output block on this thread's matcher
    stream (held back), then the next call rewrites the block with B's records on the extractor's streams.  The build
    must still see A.  Forms: orbfe_extract (the host waits in sync_all), orbfe_extract_stereo_frame on one stream (the
    wait on stream 0) and with the lane schedule on two streams (the wait on P)."""
    amd = _amd()
    from orb_slam2_annotate_amd import synth
    from orb_slam2_annotate_amd.matcher import ResidentFrame, debug_stall_thread_stream, debug_thread_stream_idle
    case = "frame_build_vs_next_extract"
    probe = Probe()
    A, B = _frames(40, 2)
    e = amd.ORBextractor(*P_VGA)
    kB, dB = e(B)                              # primes the output block
    kA, dA = e(A)
    fvA = amd.FeatureVector.from_node_of_feature(nodes_of(len(kA), 41))
    twin = view_of(kA, dA).upload(fvA)
    ResidentFrame(view_of(kA, dA), fvA, extractor=e, frame=0).close()  # primes slab pool + staging
    prove_window(case, debug_stall_thread_stream, lambda u: e.debug_stall_stream(0, u), debug_thread_stream_idle,
                 lambda: e.debug_stream_idle(0))
    debug_stall_thread_stream(STALL_US)
    R = ResidentFrame(view_of(kA, dA), fvA, extractor=e, frame=0)
    kB2, dB2 = e(B)
    expect_records(case, "extract(B) after the build", kB, dB, kB2, dB2)
    probe.expect(case, "orbfe_extract form", twin, R)
    R.close()

    pairA = synth.render_stereo(42, 640, 480, n_shapes=250, max_disp=40)
    pairB = synth.render_stereo(43, 640, 480, n_shapes=250, max_disp=40)
    for lanes in (False, True):
        form = "stereo_frame lanes" if lanes else "stereo_frame"
        e = amd.ORBextractor(*P_VGA)
        if lanes:
            e.set_streams(2)
            e.set_schedule(True)
        e.extract_stereo_frame(*pairB, 400.0, 1.0)
        kA, dA = e.extract_stereo_frame(*pairA, 400.0, 1.0)[:2]
        fvA = amd.FeatureVector.from_node_of_feature(nodes_of(len(kA), 44))
        twin = view_of(kA, dA).upload(fvA)
        ResidentFrame(view_of(kA, dA), fvA, extractor=e, frame=0).close()
        racing = 1 if lanes else 0
        prove_window(case, debug_stall_thread_stream, lambda u: e.debug_stall_stream(racing, u), debug_thread_stream_idle,
                     lambda: e.debug_stream_idle(racing))
        debug_stall_thread_stream(STALL_US)
        R = ResidentFrame(view_of(kA, dA), fvA, extractor=e, frame=0)
        e.extract_stereo_frame(*pairB, 400.0, 1.0)
        probe.expect(case, form, twin, R)
        R.close()


def set_featvec_cross_thread():
    """A frame is uploaded without a FeatureVector on a worker thread (its stream held back: the upload's one copy of the
    slab head, index region included, is still queued), then the main thread attaches the FeatureVector and searches.  The
    index copy must land after the upload's copy, not before it (Tracking builds the Frame, LocalMapping runs
    KeyFrame::ComputeBoW).  The worker's staging buffer is primed with another frame's index list of the same length."""
    amd = _amd()
    from orb_slam2_annotate_amd.matcher import debug_stall_thread_stream, debug_thread_stream_idle
    case = "set_featvec_cross_thread"
    probe = Probe()
    X, B = _frames(50, 2)
    e = amd.ORBextractor(*P_VGA)
    kB, dB = e(B)
    kX, dX = kB, dB.copy()
    fvB = amd.FeatureVector.from_node_of_feature(nodes_of(len(kB), 51))
    fvX = amd.FeatureVector.from_node_of_feature(nodes_of(len(kB), 52))  # same length, other indices
    twin = view_of(kB, dB).upload(fvB)
    with ThreadPoolExecutor(1) as worker:
        worker.submit(lambda: view_of(kX, dX).upload(fvX).close()).result()  # the worker's staging holds X's index list
        debug_thread_stream_idle()  # (the main thread's stream exists)
        prove_window(case, lambda u: worker.submit(debug_stall_thread_stream, u).result(), debug_stall_thread_stream,
                     lambda: worker.submit(debug_thread_stream_idle).result(), debug_thread_stream_idle)

        def build():
            debug_stall_thread_stream(STALL_US)
            return view_of(kB, dB).upload(None)
        R = worker.submit(build).result()
        R.set_featvec(fvB)
        probe.expect(case, "SearchByBoWResident after set_featvec", twin, R)
        R.close()


def stale_output_block():
    """After orbfe_extract, a pipelined host batch or a rectified device batch writes the caller's arrays, not the handle's
    output block: orbfe_frame_from_extractor must then refuse (ORBFE_ERR_INVALID) instead of building a frame from the
    earlier call's records; a later orbfe_extract makes it work again."""
    amd = _amd()
    import torch
    from orb_slam2_annotate_amd import _lib
    from orb_slam2_annotate_amd.ingest import Rectifier
    from orb_slam2_annotate_amd.matcher import ResidentFrame
    case = "stale_output_block"
    probe = Probe()
    A, B, C_ = _frames(60, 3)
    w, h = 640, 480
    dev = torch.device("cuda", 0)
    ident_x, ident_y = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    rl, rr = Rectifier(ident_x, ident_y), Rectifier(ident_x, ident_y)
    for form in ("pipelined", "rectified"):
        e = amd.ORBextractor(*P_VGA)
        kA, dA = e(A)
        if form == "pipelined":
            out = e.extract_batch_pipelined(np.stack([B, C_, B, C_]), chunk_frames=2)
            expect_records(case, "pipelined frame 1", *oracle(P_VGA, C_), *out[1])
        else:
            cap = e.max_keypoints(w, h)
            raw = torch.from_numpy(np.stack([B, C_])).to(dev)
            rect = torch.zeros((2, h, w), dtype=torch.uint8, device=dev)
            d_kp = torch.zeros((2, cap, 7), dtype=torch.float32, device=dev)
            d_de = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
            d_n = torch.zeros((2,), dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            e.extract_stereo_rectified_batch_device(rl, rr, raw[0].data_ptr(), raw[1].data_ptr(), 1, w, h, w, w * h,
                                                    rect.data_ptr(), d_kp.data_ptr(), d_de.data_ptr(), cap, d_n.data_ptr())
            e.synchronize()
            if int(d_n[1].item()) <= 100:
                raise Mismatch(f"case={case} rectified: only {int(d_n[1].item())} keypoints in frame 1")
        try:
            ResidentFrame(view_of(kA, dA), None, extractor=e, frame=0).close()
        except amd.OrbfeError as err:
            if err.code != _lib.ERR_INVALID:
                raise
        else:
            raise Mismatch(f"case={case} {form}: frame_from_extractor built a frame from the records of the orbfe_extract "
                           "call before the batch (expected ORBFE_ERR_INVALID)")
        kC, dC = e(C_)
        fvC = amd.FeatureVector.from_node_of_feature(nodes_of(len(kC), 61))
        R = ResidentFrame(view_of(kC, dC), fvC, extractor=e, frame=0)
        probe.expect(case, f"{form}: orbfe_extract afterwards", view_of(kC, dC).upload(fvC), R)
        R.close()


def frame_synchronize():
    """orbfe_frame_from_device on caller-owned device arrays, the build held back on this thread's stream:
    orbfe_frame_synchronize returns only after the build, so the caller may then overwrite its arrays (here with another
    frame's complete records) without the frame noticing."""
    amd = _amd()
    import torch
    from orb_slam2_annotate_amd.matcher import ResidentFrame, debug_stall_thread_stream, debug_thread_stream_idle
    case = "frame_synchronize"
    probe = Probe()
    A, B = _frames(70, 2)
    w, h = 640, 480
    dev = torch.device("cuda", 0)
    e = amd.ORBextractor(*P_VGA)
    cap = e.max_keypoints(w, h)
    imgs = torch.from_numpy(np.stack([A, B])).to(dev)
    d_kp = torch.zeros((2, cap, 7), dtype=torch.float32, device=dev)
    d_de = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros((2,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.extract_batch_device(imgs.data_ptr(), 2, w, h, w, w * h, d_kp.data_ptr(), d_de.data_ptr(), cap, d_n.data_ptr())
    kA, dA = e(A)
    fvA = amd.FeatureVector.from_node_of_feature(nodes_of(len(kA), 71))
    twin = view_of(kA, dA).upload(fvA)
    keep_kp, keep_de = d_kp[0].clone(), d_de[0].clone()
    torch.cuda.synchronize()

    def torch_marker(_usec):
        d_n.add_(0)
        torch.cuda.current_stream().synchronize()
    prove_window(case, debug_stall_thread_stream, torch_marker, debug_thread_stream_idle, lambda: True)
    debug_stall_thread_stream(STALL_US)
    R = ResidentFrame(view_of(kA, dA), fvA, d_keypoints=d_kp[0].data_ptr(), d_descriptors=d_de[0].data_ptr())
    R.synchronize()
    d_kp[0].copy_(d_kp[1])                     # the caller reuses its arrays for the next frame
    d_de[0].copy_(d_de[1])
    torch.cuda.synchronize()
    probe.expect(case, "frame_from_device + synchronize", twin, R)
    R.close()
    d_kp[0].copy_(keep_kp)
    d_de[0].copy_(keep_de)
    torch.cuda.synchronize()


def frame_ready_cross_thread():
    """A frame uploaded / built from the extractor on a worker thread whose stream is held back, used by a search on the
    main thread at once: the search's stream must wait for the frame's event (frame_use)."""
    amd = _amd()
    from orb_slam2_annotate_amd.matcher import ResidentFrame, debug_stall_thread_stream, debug_thread_stream_idle
    case = "frame_ready_cross_thread"
    probe = Probe()
    A, = _frames(80, 1)
    e = amd.ORBextractor(*P_VGA)
    kA, dA = e(A)
    fvA = amd.FeatureVector.from_node_of_feature(nodes_of(len(kA), 81))
    twin = view_of(kA, dA).upload(fvA)
    perm = np.random.default_rng(82).permutation(len(kA))  # another complete frame of the same size
    fvP = amd.FeatureVector.from_node_of_feature(nodes_of(len(kA), 83))
    debug_thread_stream_idle()
    with ThreadPoolExecutor(1) as worker:
        for form in ("upload", "from_extractor"):
            make = (lambda: view_of(kA, dA).upload(fvA)) if form == "upload" else \
                (lambda: ResidentFrame(view_of(kA, dA), fvA, extractor=e, frame=0))
            # the slab pool hands the next frame of this size the slab of a released one: prime it with the permuted frame
            worker.submit(lambda: view_of(kA[perm], dA[perm]).upload(fvP).close()).result()
            prove_window(case, lambda u: worker.submit(debug_stall_thread_stream, u).result(), debug_stall_thread_stream,
                         lambda: worker.submit(debug_thread_stream_idle).result(), debug_thread_stream_idle)

            def build():
                debug_stall_thread_stream(STALL_US)
                return make()
            R = worker.submit(build).result()
            probe.expect(case, form, twin, R)
            R.close()


def staging_reuse():
    """Two uploads back to back on one thread whose stream is held back: the first one's copy out of the thread's pinned
    staging buffer is still queued when the second fills the buffer -- it must wait for that copy first."""
    amd = _amd()
    from orb_slam2_annotate_amd.matcher import debug_stall_thread_stream, debug_thread_stream_idle
    case = "staging_reuse"
    probe = Probe()
    A, B = _frames(90, 2)
    e = amd.ORBextractor(*P_VGA)
    kA, dA = e(A)
    kB, dB = e(B)
    n = min(len(kA), len(kB))                  # one slab layout for both
    kA, dA, kB, dB = kA[:n], dA[:n], kB[:n], dB[:n]
    fvA = amd.FeatureVector.from_node_of_feature(nodes_of(n, 91))
    fvB = amd.FeatureVector.from_node_of_feature(nodes_of(n, 92))
    twinA, twinB = view_of(kA, dA).upload(fvA), view_of(kB, dB).upload(fvB)
    prove_host_ahead(case, debug_stall_thread_stream, debug_thread_stream_idle)
    debug_stall_thread_stream(STALL_US)
    RA = view_of(kA, dA).upload(fvA)
    RB = view_of(kB, dB).upload(fvB)
    probe.expect(case, "first upload", twinA, RA)
    probe.expect(case, "second upload", twinB, RB)
    RA.close()
    RB.close()


# -- the extractor's own streams --
class _DeviceBatch:
    """B stereo frames (L0, R0, L1, R1, ...) as device tensors + output arrays of one capacity."""

    def __init__(self, e, pairs, w, h):
        import torch
        dev = torch.device("cuda", 0)
        self.w, self.h, self.B, self.P = w, h, 2 * len(pairs), len(pairs)
        self.imgs = np.stack([im for pr in pairs for im in pr])
        self.d_img = torch.from_numpy(self.imgs).to(dev)
        self.cap = e.max_keypoints(w, h)
        self.d_kp = torch.zeros((self.B, self.cap, 7), dtype=torch.float32, device=dev)
        self.d_de = torch.zeros((self.B, self.cap, 32), dtype=torch.uint8, device=dev)
        self.d_n = torch.zeros((self.B,), dtype=torch.int32, device=dev)
        self.d_u = torch.zeros((self.P, self.cap), dtype=torch.float32, device=dev)
        self.d_d = torch.zeros((self.P, self.cap), dtype=torch.float32, device=dev)
        self.d_ns = torch.zeros((self.P,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def extract(self, e, d_img=None):
        img = self.d_img if d_img is None else d_img
        e.extract_batch_device(img.data_ptr(), self.B, self.w, self.h, self.w, self.w * self.h, self.d_kp.data_ptr(),
                               self.d_de.data_ptr(), self.cap, self.d_n.data_ptr(), wait=False)

    def stereo(self, e, n_pairs=None):
        """n_pairs < P: the consumer form (one launch on stream 0 behind all sub-batches) also on the sub-batch schedule,
        which matches a full batch on each sub-batch's own stream instead."""
        self.np = self.P if n_pairs is None else n_pairs
        e.stereo_match_batch_device(self.np, self.d_kp.data_ptr(), self.d_de.data_ptr(), self.d_n.data_ptr(), self.cap,
                                    MBF, MB, self.d_u.data_ptr(), self.d_d.data_ptr(), self.d_ns.data_ptr())

    def expect_records(self, case, what, params, imgs):
        from orb_slam2_annotate_amd import _lib
        for f in range(self.B):
            n = int(self.d_n[f].item())
            kps = np.ascontiguousarray(self.d_kp[f, :n].cpu().numpy()).view(_lib.KP_DTYPE).reshape(-1)
            expect_records(case, f"{what} frame {f}", *oracle(params, imgs[f]), kps, self.d_de[f, :n].cpu().numpy())

    def expect_stereo(self, case, what, params, imgs):
        import oracle_lib as orc
        o = orc.Oracle(*params)
        for p in range(self.np):
            kL, dL, pL = oracle(params, imgs[2 * p], True)
            kR, dR, pR = oracle(params, imgs[2 * p + 1], True)
            u_ref, d_ref = o.stereo(self.w, self.h, kL, dL, kR, dR, pL, pR, MBF, MB)
            expect_equal(case, f"{what} pair {p} mvuRight", u_ref, self.d_u[p, :len(kL)].cpu().numpy())
            expect_equal(case, f"{what} pair {p} mvDepth", d_ref, self.d_d[p, :len(kL)].cpu().numpy())


MBF = float(np.float32(120.0))
MB = float(np.float32(np.float32(120.0) / np.float32(400.0)))
STEREO_WH = (640, 240)


def _stereo_pairs(seed, n):
    from orb_slam2_annotate_amd import synth
    w, h = STEREO_WH
    return [synth.render_stereo(seed + p, w, h, n_shapes=250, max_disp=40) for p in range(n)]


def _consumer_vs_extract(case, lanes):
    """async extract(A) on 4 streams, the batched stereo matcher on A (a consumer on stream 0, held back), async
    extract(B) into the same arrays: extract(B) must not overwrite A's pyramid / records before the matcher has read them."""
    import torch
    amd = _amd()
    pa, pb = _stereo_pairs(100, 4), _stereo_pairs(110, 4)
    e = amd.ORBextractor(*P_STEREO)
    e.set_streams(4)
    e.set_schedule(lanes)
    bt = _DeviceBatch(e, pa, *STEREO_WH)
    d_b = torch.from_numpy(np.stack([im for pr in pb for im in pr])).to(bt.d_img.device)
    imgsB = np.stack([im for pr in pb for im in pr])
    n_pairs = None if lanes else bt.P - 1
    bt.extract(e, d_b)                          # primes every buffer with B
    bt.stereo(e, n_pairs)
    bt.extract(e)
    e.synchronize()
    racing = 1                                  # the first stream extract(B) writes on besides stream 0 (lanes: P)
    prove_window(case, lambda u: e.debug_stall_stream(0, u), lambda u: e.debug_stall_stream(racing, u),
                 lambda: e.debug_stream_idle(0), lambda: e.debug_stream_idle(racing))
    e.debug_stall_stream(0, STALL_US)
    bt.stereo(e, n_pairs)                       # reads A, behind the stall
    bt.extract(e, d_b)                          # overwrites the arrays with B
    e.synchronize()
    bt.expect_records(case, "extract(B)", P_STEREO, imgsB)
    bt.expect_stereo(case, "stereo(A)", P_STEREO, bt.imgs)


def consumer_vs_extract_subbatch():
    """Sub-batch schedule: streams 1..3 of extract(B) wait for the matcher's event (evConsumerDone)."""
    _consumer_vs_extract("consumer_vs_extract_subbatch", False)


def consumer_vs_extract_lanes():
    """Lane schedule: the pyramid lane P of extract(B) waits for the matcher's event (evConsumerDone)."""
    _consumer_vs_extract("consumer_vs_extract_lanes", True)


def tail_lane_vs_next_call():
    """Lane schedule, two async calls into separate arrays: call 1's tail lane (T = stream 0, held back) still reads its
    pyramid / candidates when call 2's pyramid lane P would rewrite them -- P waits for evTail of the same slice."""
    amd = _amd()
    case = "tail_lane_vs_next_call"
    pa, pb = _stereo_pairs(120, 4), _stereo_pairs(130, 4)
    e = amd.ORBextractor(*P_STEREO)
    e.set_streams(4)
    e.set_schedule(True)
    b1, b2 = _DeviceBatch(e, pa, *STEREO_WH), _DeviceBatch(e, pb, *STEREO_WH)
    b1.extract(e, b2.d_img)                     # primes both sets of arrays with complete results
    b2.extract(e, b1.d_img)
    e.synchronize()
    prove_window(case, lambda u: e.debug_stall_stream(0, u), lambda u: e.debug_stall_stream(1, u),
                 lambda: e.debug_stream_idle(0), lambda: e.debug_stream_idle(1))
    e.debug_stall_stream(0, STALL_US)
    b1.extract(e)
    b2.extract(e)
    e.synchronize()
    b1.expect_records(case, "call 1", P_STEREO, b1.imgs)
    b2.expect_records(case, "call 2", P_STEREO, b2.imgs)


def subbatch_join_vs_consumer():
    """Sub-batch schedule: extract(A) with one of its streams held back, then the stereo matcher on stream 0 -- it must
    join every sub-batch stream first (evChunkDone) instead of reading the previous call's records."""
    import torch
    amd = _amd()
    case = "subbatch_join_vs_consumer"
    pa, pb = _stereo_pairs(140, 4), _stereo_pairs(150, 4)
    e = amd.ORBextractor(*P_STEREO)
    e.set_streams(4)
    bt = _DeviceBatch(e, pa, *STEREO_WH)
    d_b = torch.from_numpy(np.stack([im for pr in pb for im in pr])).to(bt.d_img.device)
    n_pairs = bt.P - 1                          # the consumer form (stereo() docstring)
    bt.extract(e, d_b)                          # primes the arrays with B
    bt.stereo(e, n_pairs)
    e.synchronize()
    for k in (1, 2):                            # sub-batches 1 and 2 hold frames 2-5, which the 3-pair consumer reads
        prove_window(case, lambda u: e.debug_stall_stream(k, u), lambda u: e.debug_stall_stream(0, u),
                     lambda: e.debug_stream_idle(k), lambda: e.debug_stream_idle(0))
        e.debug_stall_stream(k, STALL_US)
        bt.extract(e)
        bt.stereo(e, n_pairs)
        e.synchronize()
        bt.expect_records(case, f"extract(A), stream {k} held", P_STEREO, bt.imgs)
        bt.expect_stereo(case, f"stereo(A), stream {k} held", P_STEREO, bt.imgs)
        bt.extract(e, d_b)
        bt.stereo(e, n_pairs)
        e.synchronize()


def pipelined_slots():
    """The pipelined host path (6 chunks of 2 frames, two input slabs, two output blocks), both schedules.  H2D copy stream
    held back: the kernels of each chunk wait for its upload (evIn), and the download of each chunk waits for its kernels
    (evComp on the D2H stream) instead of copying the block's previous contents.  D2H copy stream held back: the kernels of
    chunk k+2 wait for chunk k's download out of the same output block (evOutDone), so they are held back too, and the
    upload of chunk k+4 into the same input slab must wait for them (evComp on the H2D stream)."""
    amd = _amd()
    case = "pipelined_slots"
    from orb_slam2_annotate_amd import _lib
    B = 12
    frames = np.stack(_frames(160, B))
    prime = np.stack(_frames(172, B))
    for lanes in (False, True):
        e = amd.ORBextractor(*P_VGA)
        e.set_streams(2)
        e.set_schedule(lanes)
        img, kps, desc, n = e.pinned_buffers(B, 480, 640)
        np.copyto(img, prime)
        e.extract_pinned(chunk_frames=2)        # primes slabs, output blocks and the copy streams
        np.copyto(img, frames)
        for held, racing in ((_lib.DEBUG_STREAM_H2D, 0), (_lib.DEBUG_STREAM_D2H, 0)):
            what = f"{'lanes' if lanes else 'sub-batches'}, {'H2D' if held == _lib.DEBUG_STREAM_H2D else 'D2H'} held"
            prove_window(case, lambda u: e.debug_stall_stream(held, u), lambda u: e.debug_stall_stream(racing, u),
                         lambda: e.debug_stream_idle(held), lambda: e.debug_stream_idle(racing))
            e.debug_stall_stream(held, STALL_US)
            e.extract_pinned(chunk_frames=2)
            for f in range(B):
                expect_records(case, f"{what} frame {f}", *oracle(P_VGA, frames[f]), kps[f, :n[f]], desc[f, :n[f]])
            np.copyto(img, prime)               # the slabs hold another complete result before the next form
            e.extract_pinned(chunk_frames=2)
            np.copyto(img, frames)


def vocab_straddling_pair():
    """Consecutive-frame SearchByBoW per sub-batch (orbfe_bow_match_consecutive_batch_device_async behind an async
    extract on 4 streams, 2 frames each): the pair that straddles sub-batches i-1 and i runs on stream i.  (1) Stream i-1
    held back before the calls: the pair must wait for sub-batch i-1's FeatureVectors (evFv) instead of reading the
    previous call's.  (2) Stream i held back before call 1, call 2 enqueued at once into the same arrays: call 2's stream
    i-1 must wait for call 1's straddling pair (evBoundary) before it rewrites frame 2i-1.  Matches against the oracle."""
    import torch
    import oracle_lib as orc
    amd = _amd()
    from orb_slam2_annotate_amd import synth
    from orb_slam2_annotate_amd.vocabulary import synthetic_vocabulary_arrays
    case = "vocab_straddling_pair"
    B, LS, params = 8, 4, P_VGA
    arrays = synthetic_vocabulary_arrays(10, 6, 1)
    vo = orc.Vocabulary.from_arrays(arrays)
    voc = amd.ORBVocabulary()
    if not voc.createFromArrays(arrays):
        raise Mismatch(f"case={case}: vocabulary not created")
    seqs = [np.stack(synth.render_sequence(s, B, 640, 480, step=1.5)) for s in (4300, 4400, 4500)]
    e = amd.ORBextractor(*params)
    e.set_streams(4)
    cap = e.max_keypoints(640, 480)
    dev = torch.device("cuda", 0)
    d_imgs = [torch.from_numpy(s).to(dev) for s in seqs]
    d_kp = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
    d_de = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros((B,), dtype=torch.int32, device=dev)
    d_m = torch.zeros((2, B - 1, cap), dtype=torch.int32, device=dev)
    d_nm = torch.zeros((2, B - 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def call(k, out):
        e.extract_batch_device(d_imgs[k].data_ptr(), B, 640, 480, 640, 640 * 480, d_kp.data_ptr(), d_de.data_ptr(), cap,
                               d_n.data_ptr(), wait=False)
        voc.bow_match_consecutive_batch_device(B, d_kp.data_ptr(), d_de.data_ptr(), d_n.data_ptr(), cap,
                                               d_m[out].data_ptr(), d_nm[out].data_ptr(), nnratio=0.7,
                                               check_orientation=True, levelsup=LS, extractor=e)

    def expect(k, out, what):
        ref = [oracle(params, f) for f in seqs[k]]
        fvs = [orc.FeatVec(vo.transform(d, LS)[3]) for _, d in ref]
        total = 0
        for t in range(1, B):
            (k1, de1), (k2, de2) = ref[t - 1], ref[t]
            rn, rm = orc.search_by_bow(de1, np.ones(len(k1), np.uint8), k1["angle"], fvs[t - 1], de2, k2["angle"],
                                       fvs[t], 0.7, True)
            expect_equal(case, f"{what} pair ({t - 1}, {t}) match count", np.int32(rn), np.int32(d_nm[out, t - 1].item()))
            expect_equal(case, f"{what} pair ({t - 1}, {t}) matches", rm, d_m[out, t - 1, :len(k2)].cpu().numpy())
            total += rn
        if total < 100:
            raise Mismatch(f"case={case} {what}: only {total} matches over the sequence (too few to tell frames apart)")

    for i in (1, 2, 3):  # (1) the FeatureVectors of sub-batch i-1 (stream i-1 held back)
        call(2, 0)       # primes records, FeatureVectors and matches with another complete sequence
        e.synchronize()
        prove_window(case, lambda u: e.debug_stall_stream(i - 1, u), lambda u: e.debug_stall_stream(i, u),
                     lambda: e.debug_stream_idle(i - 1), lambda: e.debug_stream_idle(i))
        e.debug_stall_stream(i - 1, STALL_US)
        call(0, 0)
        e.synchronize()
        expect(0, 0, f"stream {i - 1} held")
    for i in (1, 2, 3):  # (2) call 2 vs call 1's straddling pair (stream i held back)
        call(2, 0)
        call(2, 1)
        e.synchronize()
        prove_window(case, lambda u: e.debug_stall_stream(i, u), lambda u: e.debug_stall_stream(i - 1, u),
                     lambda: e.debug_stream_idle(i), lambda: e.debug_stream_idle(i - 1))
        e.debug_stall_stream(i, STALL_US)
        call(0, 0)
        call(1, 1)
        e.synchronize()
        expect(0, 0, f"call 1, stream {i} held")
        expect(1, 1, f"call 2, stream {i} held")


def lane_stages():
    """Lane schedule inside one call: V (FAST, blur) waits for P's pyramid (evPyr), T waits for V's FAST (evFast) and blur
    (evBlur).  P or V held back before an async call; every output equal to the oracle."""
    amd = _amd()
    case = "lane_stages"
    pa = _stereo_pairs(180, 4)
    e = amd.ORBextractor(*P_STEREO)
    e.set_streams(4)
    e.set_schedule(True)
    bt = _DeviceBatch(e, pa, *STEREO_WH)
    other = bt.d_img.flip(0).contiguous()       # the same frames in another order
    for held, racing in ((1, 2), (2, 0)):
        bt.extract(e, other)                    # primes every buffer with another complete result
        e.synchronize()
        prove_window(case, lambda u: e.debug_stall_stream(held, u), lambda u: e.debug_stall_stream(racing, u),
                     lambda: e.debug_stream_idle(held), lambda: e.debug_stream_idle(racing))
        e.debug_stall_stream(held, STALL_US)
        bt.extract(e)
        e.synchronize()
        bt.expect_records(case, f"lane {'P' if held == 1 else 'V'} held", P_STEREO, bt.imgs)


# ---- the table --------------------------------------------------------------------------------------------------------
CASES = {
    "frame_build_vs_next_extract": Case(frame_build_vs_next_extract, pins=[
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(s, e->evReaderDone)",
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(sP, e->evReaderDone)",
        "extractor_handle.hip:reader_settle:hipEventSynchronize(e->evReaderDone)",
    ], bug="resident frame built from the output block vs. the next extract (write after read)"),
    "set_featvec_cross_thread": Case(set_featvec_cross_thread, pins=[],
                                     bug="orbfe_frame_set_featvec vs. the frame's own build copy (frame_use)"),
    "stale_output_block": Case(stale_output_block, pins=[],
                               bug="a stale output block served after a pipelined or rectified call"),
    "frame_synchronize": Case(frame_synchronize, pins=[
        "frames.hip:orbfe_frame_synchronize:hipEventSynchronize(f->ready)",
    ]),
    "frame_ready_cross_thread": Case(frame_ready_cross_thread, pins=[
        "frames.hip:frame_use:hipStreamWaitEvent(ar->stream, f->ready)",
    ]),
    "staging_reuse": Case(staging_reuse, pins=[
        "arena.hip:staging_reserve:hipEventSynchronize(t_staging.pending)",
    ]),
    "consumer_vs_extract_subbatch": Case(consumer_vs_extract_subbatch, pins=[
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(s, e->evConsumerDone)",
    ]),
    "consumer_vs_extract_lanes": Case(consumer_vs_extract_lanes, pins=[
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(sP, e->evConsumerDone)",
    ]),
    "tail_lane_vs_next_call": Case(tail_lane_vs_next_call, pins=[
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(sP, e->evTail[i])",
    ]),
    "subbatch_join_vs_consumer": Case(subbatch_join_vs_consumer, pins=[
        "extractor_handle.hip:orbfe_extractor_consumer_begin_:hipStreamWaitEvent(e->stream, e->evChunkDone[i])",
    ]),
    "pipelined_slots": Case(pipelined_slots, pins=[
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(s, waitFor[k])",
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(sP, waitFor[k])",
        "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(sT, waitFor[k])",
        "extractor.hip:orbfe_extract_batch_pipelined:hipStreamWaitEvent(e->sH2D, e->evComp[slot])",
        "extractor.hip:orbfe_extract_batch_pipelined:hipStreamWaitEvent(e->sD2H, e->evComp[slot])",
    ]),
    "vocab_straddling_pair": Case(vocab_straddling_pair, pins=[
        "vocabulary.hip:bow_match_consecutive:hipStreamWaitEvent(streams[i], v->evFv[i - 1])",
        "vocabulary.hip:bow_match_consecutive:hipStreamWaitEvent(streams[i - 1], v->evBoundary[i])",
    ]),
    "lane_stages": Case(lane_stages, pins=[
        "extractor_pipeline.hip:run_chunk:hipStreamWaitEvent(sV, e->evPyr[sub])",
        "extractor_pipeline.hip:run_chunk:hipStreamWaitEvent(sT, e->evFast[sub])",
        "extractor_pipeline.hip:run_chunk:hipStreamWaitEvent(sT, e->evBlur[sub])",
    ]),
}

# wait sites no case pins, each with the reason
NOT_CASED = {
    "extractor_handle.hip:resolve_slot:hipEventSynchronize(e->evB[slot][sub][st])":
        "stage-timer readout after the call's own synchronisation: orders no data",
    "extractor.hip:orbfe_extract_batch_pipelined:hipStreamWaitEvent(e->stream, e->evChunkDone[i])":
        "the call drains stream 0 and extra[] first and all sub-batches of a chunk wait on the same copy events, so no "
        "stall holds one sub-batch back against stream 0",
    "frames.hip:orbfe_frame_release:hipEventSynchronize(f->ready)":
        "teardown: a frame released before its build finished; the wait guards the slab's return to the pool",
}


def main(argv):
    if len(argv) != 2 or argv[1] not in CASES:
        print("usage: stream_order.py CASE\n  " + "\n  ".join(CASES), file=sys.stderr)
        return 2
    name = argv[1]
    try:
        CASES[name].run()
    except (Mismatch, WindowClosed) as m:
        print(f"MISMATCH {m}" if isinstance(m, Mismatch) else f"WINDOW {m}")
        return 1
    print(f"order ok: {name}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
