"""CPU drift guard of the ingest and vocabulary files of csrc/: kernels and launchers in k_ingest.hip / k_vocab.hip, handles
and entry points in ingest.hip / vocabulary.hip, and the host-array calls staged through the calling thread's arena -- no
buffer of their own, no synchronous copy, no device-wide wait, no scratch on the vocabulary handle."""
import re
from pathlib import Path

from test_host_internal_header import _DEFN, _code

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
KERNEL_FILES = ("k_ingest.hip", "k_vocab.hip")
HOST_FILES = ("ingest.hip", "vocabulary.hip")
EXTERN_C_FN = re.compile(r'^extern\s+"C"\s+[^;{}]*\{', re.M)
HANDLE = re.compile(r"^struct\s+orbfe_\w+", re.M)
SYNC_WAYS = re.compile(r"\bhipDeviceSynchronize\b|\bhipMemcpy\s*\(|\bhipMemcpy2D\s*\(")
DELETED_MEMBERS = ("d_desc", "d_word", "d_node", "d_weight", "fk_keys")
_CLOSE = re.compile(r"^\}", re.M)


def code(name, root=CSRC):
    return _code((root / name).read_text())


def scope(text, start_rx):
    """The text of the function or struct that starts in column 0 where start_rx matches, up to its closing brace."""
    m = re.search(start_rx, text, re.M)
    assert m, start_rx
    return text[m.start():_CLOSE.search(text, m.start()).start()]


def function(text, name):
    starts = [m.start() for m in _DEFN.finditer(text) if m.group(2) == name]
    assert len(starts) == 1, (name, starts)
    return text[starts[0]:_CLOSE.search(text, starts[0]).start()]


def devbuf_outside_the_rectifier(root=CSRC):
    """Every `DevBuf<` of ingest.hip that is not a member of struct orbfe_rectifier: (function or '?', the line)."""
    text = code("ingest.hip", root)
    handle = re.search(r"^struct\s+orbfe_rectifier\s*\{", text, re.M)
    lo, hi = handle.start(), _CLOSE.search(text, handle.start()).start()
    spans = [(m.start(), _CLOSE.search(text, m.start()).start(), m.group(2)) for m in _DEFN.finditer(text)]
    out = []
    for m in re.finditer(r"\bDevBuf\s*<", text):
        if lo <= m.start() < hi:
            continue
        inside = [n for a, b, n in spans if a <= m.start() < b]
        out.append((inside[-1] if inside else "?", text[text.rfind("\n", 0, m.start()) + 1:text.find("\n", m.start())].strip()))
    return out


def test_the_scan_reads_the_four_files():
    assert "__global__" in code("k_ingest.hip") and "__global__" in code("k_vocab.hip")
    assert len(EXTERN_C_FN.findall(code("ingest.hip"))) == 13  # (twelve public calls and orbfe_remap_launch_)
    assert EXTERN_C_FN.search(code("vocabulary.hip"))
    assert re.search(r"\bDevBuf\s*<", scope(code("ingest.hip"), r"^struct\s+orbfe_rectifier\s*\{"))


def test_kernel_files_hold_no_entry_point_and_no_handle():
    for name in KERNEL_FILES:
        assert not EXTERN_C_FN.search(code(name)), f'{name} defines an extern "C" function: entry points belong in the host file'
        assert not HANDLE.search(code(name)), f"{name} defines a handle struct"


def test_host_files_hold_no_kernel():
    for name in HOST_FILES:
        assert "__global__" not in code(name), f"{name} holds a kernel: kernels belong in k_*.hip behind a launcher"


def test_every_kernel_of_the_issue_is_where_its_launcher_is():
    k = code("k_ingest.hip")
    for kernel in ("k_cvt_gray", "k_distinctive", "k_remap_convert", "k_remap", "k_init_rectify_map", "k_undistort_points",
                   "k_undistort_keypoints", "k_stereo_from_rgbd"):
        assert re.search(r"__global__[^;{]*\b" + kernel + r"\s*\(", k), kernel
        assert re.search(r"^void\s+launch_" + kernel[2:] + r"\s*\(", k, re.M), f"no launcher of {kernel}"
    v = code("k_vocab.hip")
    assert re.search(r"^void\s+launch_vocab_transform\s*\(", v, re.M) and re.search(r"^void\s+launch_vocab_featvec\s*\(", v, re.M)


def test_ingest_hip_has_no_synchronous_copy_and_no_device_wide_wait():
    found = sorted({m.group(0) for m in SYNC_WAYS.finditer(code("ingest.hip"))})
    assert not found, f"ingest.hip names {found}: stage through the arena and wait for one stream"


def test_ingest_hip_owns_device_memory_only_in_the_rectifier():
    assert not devbuf_outside_the_rectifier(), "a host-array call carves from the thread arena (arena_stage), it holds no DevBuf"


def test_the_host_array_calls_stage_through_the_arena():
    text = code("ingest.hip")
    for fn in ("orbfe_cvt_gray", "orbfe_distinctive_descriptors", "orbfe_rectifier_create", "orbfe_remap",
               "orbfe_init_undistort_rectify_map", "orbfe_undistort_points", "orbfe_stereo_from_rgbd"):
        body = function(text, fn)
        assert "arena_stage(" in body and "hipStreamSynchronize(ar->stream)" in body, fn
        assert not re.search(r"launch_\w+\s*\(\s*(?:0|nullptr|kDefaultStream)\b", body), f"{fn} launches on the default stream"
    assert "orbfe_undistort_points(" in function(text, "orbfe_compute_image_bounds")


def test_the_vocabulary_handle_keeps_no_scratch_of_the_stateless_calls():
    text = code("vocabulary.hip")
    body = scope(text, r"^struct\s+orbfe_vocabulary\s*\{")
    for member in DELETED_MEMBERS:
        assert not re.search(r"\b" + member + r"\b", body), f"struct orbfe_vocabulary has {member} again"
    assert "arena_stage(" in function(text, "orbfe_vocabulary_transform")
    assert "arena_stage(" in function(text, "orbfe_vocabulary_featvec_batch_device")
    assert "vocab_upload" in {m.group(2) for m in _DEFN.finditer(text)}


def test_the_guard_notices_a_buffer_of_its_own(tmp_path):
    """A scratch copy of csrc/ whose orbfe_undistort_points holds a DevBuf again, and one whose k_vocab.hip has an entry point."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp"):
            (tmp_path / p.name).write_text(p.read_text())
    assert not devbuf_outside_the_rectifier(tmp_path)
    f = tmp_path / "ingest.hip"
    text = f.read_text()
    line = "  if (n == 0) return ORBFE_OK;\n  float *din, *dout;\n"
    assert text.count(line) == 1
    f.write_text(text.replace(line, "  if (n == 0) return ORBFE_OK;\n  DevBuf<float> tmp;\n  float *din, *dout;\n"))
    assert devbuf_outside_the_rectifier(tmp_path) == [("orbfe_undistort_points", "DevBuf<float> tmp;")]
    f.write_text(text.replace("  HIPCHK(hipStreamSynchronize(kDefaultStream));\n", "  HIPCHK(hipDeviceSynchronize());\n", 1))
    assert [m.group(0) for m in SYNC_WAYS.finditer(code("ingest.hip", tmp_path))] == ["hipDeviceSynchronize"]
    k = tmp_path / "k_vocab.hip"
    k.write_text(k.read_text() + '\nextern "C" int orbfe_vocabulary_peek(void) {\n  return 0;\n}\n')
    assert EXTERN_C_FN.search(code("k_vocab.hip", tmp_path))
