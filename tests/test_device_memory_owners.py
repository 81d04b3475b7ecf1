"""CPU drift guard of who owns device and pinned memory in csrc/: the allocator calls of the HIP runtime appear in the owning
buffer of csrc/host_internal.h (DevBuf / PinBuf), in the slab pool and in the public raw allocator, and nowhere else -- host
code that needs memory holds a buffer, so no error path has a pointer of its own to free."""
import re
from pathlib import Path

from test_host_internal_header import _DEFN, _code

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
CALLS = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree)\s*\(")
# "file:scope" -> why the raw call is there; a scope is a function or struct that starts in column 0 and ends at the next
# closing brace in column 0
ALLOWED = {
    "host_internal.h:DevBuf": "DevBuf / PinBuf: the owning buffer every other site holds",
    "arena.hip:slab_get": "the slab pool hands out a kept slab or allocates one of the next size class",
    "arena.hip:slab_put": "the slab pool frees a slab it has no room to keep",
    "runtime.hip:orbfe_host_alloc": "public raw allocator of pinned host memory (include/orbfe.h)",
    "runtime.hip:orbfe_host_free": "frees what orbfe_host_alloc returned",
}
_STRUCT = re.compile(r"^(?:struct|class)\s+(\w+)[^;{}()]*\{", re.M)
_CLOSE = re.compile(r"^\}", re.M)


def raw_calls(root=CSRC):
    """(file:scope, call) of every allocator call; scope "?": outside every function and struct that starts in column 0."""
    out = []
    for path in sorted(root.iterdir()):
        if path.suffix not in (".hip", ".cpp", ".h"):
            continue
        text = _code(path.read_text())
        scopes = [(m.start(), m.group(2).split("::")[-1]) for m in _DEFN.finditer(text)]
        scopes += [(m.start(), m.group(1)) for m in _STRUCT.finditer(text)]
        spans = []
        for start, name in scopes:
            close = _CLOSE.search(text, start)
            spans.append((start, close.start() if close else len(text), name))
        for m in CALLS.finditer(text):
            inside = [name for lo, hi, name in spans if lo <= m.start() < hi]
            out.append((f"{path.name}:{inside[-1] if inside else '?'}", m.group(1)))
    return out


def strays(root=CSRC):
    return sorted({(where, call) for where, call in raw_calls(root) if where not in ALLOWED})


def test_the_scan_finds_the_owners():
    where = {w for w, _ in raw_calls()}
    assert {"arena.hip:slab_get", "arena.hip:slab_put", "runtime.hip:orbfe_host_alloc",
            "runtime.hip:orbfe_host_free"} <= where, where
    assert {c for w, c in raw_calls() if w == "host_internal.h:DevBuf"} == {"hipMalloc", "hipFree", "hipHostMalloc",
                                                                            "hipHostFree"}


def test_raw_allocator_calls_only_where_listed():
    assert not strays(), "hold a DevBuf / PinBuf (csrc/host_internal.h) or a pool slab instead of a raw pointer"


def test_every_allowed_site_exists_and_has_a_reason():
    where = {w for w, _ in raw_calls()}
    for key, reason in ALLOWED.items():
        assert reason.strip() and "\n" not in reason, key
        assert key in where, f"{key} holds no allocator call any more"


def test_one_source_file_defines_the_slab_pool():
    defining = [p.name for p in sorted(CSRC.iterdir()) if p.suffix in (".hip", ".cpp", ".h")
                and any(m.group(2).split("::")[-1] == "slab_get" for m in _DEFN.finditer(_code(p.read_text())))]
    assert defining == ["arena.hip"], defining


def test_the_guard_notices_a_hand_made_allocation(tmp_path):
    """A scratch copy of csrc/ whose vocabulary.hip allocates one array by hand again."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp"):
            (tmp_path / p.name).write_text(p.read_text())
    assert not strays(tmp_path)
    v = tmp_path / "vocabulary.hip"
    v.write_text(v.read_text().replace(
        "  HIPCHK(hipSetDevice(v->device));\n  HIPCHK(hipStreamCreateWithFlags(",
        "  HIPCHK(hipSetDevice(v->device));\n  void* extra; HIPCHK(hipMalloc(&extra, 16));\n  HIPCHK(hipStreamCreateWithFlags(", 1))
    assert strays(tmp_path) == [("vocabulary.hip:vocab_upload", "hipMalloc")]


def test_the_guard_bounds_a_function_by_its_closing_brace(tmp_path):
    """A raw call in an indented definition behind slab_put is not credited to slab_put, nor one beside DevBuf to DevBuf."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp"):
            (tmp_path / p.name).write_text(p.read_text())
    m = tmp_path / "arena.hip"
    text = m.read_text()
    at = text.index("\n}\n", text.index("\nvoid slab_put(")) + 3
    m.write_text(text[:at] + "  inline void drop(void* q) { (void)hipFree(q); }\n" + text[at:])
    h = tmp_path / "host_internal.h"
    h.write_text(h.read_text().replace("struct Slab {", "inline void drop_pinned(void* q) { (void)hipHostFree(q); }\nstruct Slab {", 1))
    assert strays(tmp_path) == [("arena.hip:?", "hipFree"), ("host_internal.h:drop_pinned", "hipHostFree")]
