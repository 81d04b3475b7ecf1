"""Every result-neutral run-time switch of liborbfe.so against the CPU oracle (tests/kernel_variants.py has the table).

The switches are read once per process, so each VARIANTS entry runs in one fresh child process
(`python tests/kernel_variants.py NAME`), one after the other: never more than this process and one child have the GPU
open.  A child that ends by a signal, an abort, a segfault or the time limit may have left the device in a bad state, so
nothing more is started on the GPU after it: every later variant test is skipped, naming the variant that faulted.
`ORBFE_COPY_UNALIGNED` is read per handle at create, so it is tested in this process."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import kernel_variants as kv
import oracle_lib as orc
from orb_slam2_annotate_amd import synth

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
CHILD_TIMEOUT_S = 300
_FAULTED = []  # the variant whose child ended abnormally; nothing is started on the GPU after it


def _abnormal(rc):
    # < 0: killed by a signal (subprocess reports -signum); 134 / 139: SIGABRT / SIGSEGV as a shell reports them;
    # 124 / 137: a `timeout` wrapper's time limit / kill
    return rc < 0 or rc in (134, 139, 124, 137)


@pytest.mark.parametrize("name", list(kv.VARIANTS))
def test_variant_matches_the_oracle(name):
    if _FAULTED:
        pytest.skip(f"not started: the child of variant {_FAULTED[0]} ended abnormally, nothing more runs on the GPU")
    try:
        p = subprocess.run([sys.executable, str(HERE / "kernel_variants.py"), name], env=kv.child_env(name),
                           cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as t:
        _FAULTED.append(name)
        tail = t.stdout.decode(errors="replace") if isinstance(t.stdout, bytes) else (t.stdout or "")
        pytest.fail(f"variant {name}: no result within {CHILD_TIMEOUT_S} s\n{tail[-3000:]}")
    if _abnormal(p.returncode):
        _FAULTED.append(name)
    out = (p.stdout + p.stderr)[-4000:]
    assert p.returncode == 0, f"variant {name} ({kv.VARIANTS[name].env}) exit {p.returncode}:\n{out}"
    assert "parity ok" in p.stdout, out
    print(p.stdout.strip().splitlines()[-1])


# ---- ORBFE_COPY_UNALIGNED: read when a handle is created ------------------------------------------------------------
def _records(d_kp, d_desc, d_n, f):
    from orb_slam2_annotate_amd import KP_DTYPE
    n = int(d_n[f].item())
    kps = np.ascontiguousarray(d_kp[f, :n].cpu().numpy()).view(KP_DTYPE).reshape(-1)
    return kps, d_desc[f, :n].cpu().numpy()


def test_copy_unaligned_single_frame_odd_pitch_and_base(monkeypatch):
    """With $ORBFE_COPY_UNALIGNED=1 a level 0 whose pitch (641), base address (offset 1, 2, 3) or frame stride is not a
    multiple of 4 is first repacked into the handle's own 64-byte pitched slab (launch_copy2d) and the kernels read that.
    Host input at pitch 641 reaches it through the input slab of the caller's pitch, device input at an odd base
    directly."""
    import torch

    import orb_slam2_annotate_amd as amd
    monkeypatch.setenv("ORBFE_COPY_UNALIGNED", "1")
    params = (1000, 1.2, 8, 20, 7)
    w, h, pitch = 640, 480, 641
    img = synth.render_frame(70)
    kr, dr = orc.Oracle(*params).extract(img)
    dev = torch.device("cuda", 0)
    for off in (1, 2, 3):
        host = np.zeros(off + pitch * h, np.uint8)
        view = np.lib.stride_tricks.as_strided(host[off:], (h, w), (pitch, 1))
        view[...] = img
        e = amd.ORBextractor(*params)
        kv.compare_frame(f"host_pitch641_offset{off}", 0, kr, dr, *e(view))
        kv.compare_image(f"host_pitch641_offset{off}", 0, "pyramid[1]", orc.resize_linear(img, *e.level_size(w, h, 1)),
                         e.pyramid_level(1))
        buf = torch.zeros(off + pitch * h + 64, dtype=torch.uint8, device=dev)
        buf[off:off + pitch * h].view(h, pitch)[:, :w] = torch.from_numpy(img).to(dev)
        cap = e.max_keypoints(w, h)
        d_kp = torch.zeros((1, cap, 7), dtype=torch.float32, device=dev)
        d_desc = torch.zeros((1, cap, 32), dtype=torch.uint8, device=dev)
        d_n = torch.zeros((1,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.extract_batch_device(buf.data_ptr() + off, 1, w, h, pitch, pitch * h, d_kp.data_ptr(), d_desc.data_ptr(), cap,
                               d_n.data_ptr())
        kv.compare_frame(f"device_pitch641_offset{off}", 0, kr, dr, *_records(d_kp, d_desc, d_n, 0))


def test_copy_unaligned_batch_odd_frame_stride(monkeypatch):
    """A 10-frame batch of caller-owned device frames at pitch 640 but an odd frame stride (640 x 480 + 1): frames 1, 3, ...
    start at odd addresses, so the whole batch is repacked first.  On 1 stream (one 10-frame launch: the throughput form)
    and on 2 sub-batch streams (6 + 4 frames: the latency form)."""
    import torch

    import orb_slam2_annotate_amd as amd
    monkeypatch.setenv("ORBFE_COPY_UNALIGNED", "1")
    params = (1100, 1.2, 8, 20, 7)
    B, w, h = 10, 640, 480
    fstride = w * h + 1
    frames = np.stack(synth.render_sequence(71, B, w, h))
    frames[4] = synth.adversarial("noise", w, h, seed=71)
    o = orc.Oracle(*params)
    ref = [o.extract(frames[f]) for f in range(B)]
    dev = torch.device("cuda", 0)
    buf = torch.zeros(B * fstride + 64, dtype=torch.uint8, device=dev)
    for f in range(B):
        buf[f * fstride:f * fstride + w * h] = torch.from_numpy(frames[f].reshape(-1)).to(dev)
    for streams in (1, 2):
        e = amd.ORBextractor(*params)
        e.set_streams(streams)
        cap = e.max_keypoints(w, h)
        d_kp = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
        d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        d_n = torch.zeros((B,), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        e.extract_batch_device(buf.data_ptr(), B, w, h, w, fstride, d_kp.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr())
        for f in range(B):
            kv.compare_frame(f"batch_fstride_odd_s{streams}", f, *ref[f], *_records(d_kp, d_desc, d_n, f))
