"""The cross-stream waits of liborbfe.so, each held open by a stalled stream (tests/stream_order.py has the table).

Each CASES entry runs in one fresh child process (`python tests/stream_order.py NAME`, GPU_MAX_HW_QUEUES=16), one after
the other: never more than this process and one child have the GPU open.  A child that ends any other way than with
"order ok" or a reported finding (a signal, an abort, the time limit, an error traceback) may have left the device in a bad
state, so nothing more is started on the GPU after it: every
later case is skipped, naming the case that ended abnormally."""
import subprocess
import sys
from pathlib import Path

import pytest

import stream_order as so

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
CHILD_TIMEOUT_S = 120
_FAULTED = []  # the case whose child ended abnormally; nothing is started on the GPU after it


def _abnormal(rc, stdout):
    # normal ends: 0 ("order ok"), or 1 after the child printed its finding (a MISMATCH or WINDOW line); anything else --
    # a signal, an abort, a time limit, an error traceback such as a HIP error -- may have left the device faulted
    if rc == 0:
        return False
    return not (rc == 1 and any(ln.startswith(("MISMATCH ", "WINDOW ")) for ln in stdout.splitlines()))


@pytest.mark.parametrize("name", list(so.CASES))
def test_stream_order_case(name):
    if _FAULTED:
        pytest.skip(f"not started: the child of case {_FAULTED[0]} ended abnormally, nothing more runs on the GPU")
    try:
        p = subprocess.run([sys.executable, str(HERE / "stream_order.py"), name], env=so.child_env(name),
                           cwd=str(HERE.parent), capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
    except subprocess.TimeoutExpired as t:
        _FAULTED.append(name)
        tail = t.stdout.decode(errors="replace") if isinstance(t.stdout, bytes) else (t.stdout or "")
        pytest.fail(f"case {name}: no result within {CHILD_TIMEOUT_S} s\n{tail[-3000:]}")
    if _abnormal(p.returncode, p.stdout):
        _FAULTED.append(name)
    out = (p.stdout + p.stderr)[-4000:]
    assert p.returncode == 0, f"case {name} exit {p.returncode}:\n{out}"
    assert "order ok" in p.stdout, out
