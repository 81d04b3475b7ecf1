"""CPU drift guard of csrc/host_internal.h and csrc/extractor_handle.h: what one host source of csrc/ defines for another
is declared there, once, and both sides include it -- so a signature that drifts does not compile.  A prototype re-typed in
a source file would bring the silent mismatch back (the back doors are extern "C"; a re-declared orbfe:: helper with other
parameters is an overload nothing defines), and an entry nobody uses would only look like an interface."""
import re
from pathlib import Path

import pytest

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
HEADERS = ("host_internal.h", "extractor_handle.h")  # the back doors of every host file; the extractor's own files
BACK_DOOR = re.compile(r"orbfe_[a-z0-9_]+_$")  # the internal cross-file functions end in '_'
_NOT_A_TYPE = {"return", "else", "delete", "new", "throw", "goto", "case", "typedef", "using", "co_return"}
# "<type words> name(<arguments>)": arguments may nest one level of parentheses (function pointers, casts in defaults)
_SIG = r'(?:extern\s+"C"\s+)?((?:[A-Za-z_][\w:<>]*[\s\*&]+)+)([A-Za-z_][\w:]*)\s*\((?:[^;{}()]|\([^;{}()]*\))*\)'
_DECL = re.compile(r"(?:^|(?<=[;{}\n]))[ \t]*" + _SIG + r"\s*;", re.M)
_DEFN = re.compile(r"^" + _SIG + r"\s*(?:const\s*)?\{", re.M)  # a definition starts in column 0 in csrc/


def _code(text):
    """The text without comments and string literals (their content could look like a declaration)."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r'"(?:[^"\\\n]|\\.)*"', lambda m: '"C"' if m.group(0) == '"C"' else '""', text)
    return re.sub(r"//[^\n]*", "", text)


def sources(root=CSRC):
    return {p.name: _code(p.read_text()) for p in sorted(root.iterdir()) if p.suffix in (".hip", ".cpp")}


def _matches(rx, text):
    for m in rx.finditer(text):
        if not set(m.group(1).replace("*", " ").replace("&", " ").split()) & _NOT_A_TYPE:
            yield m.group(2).split("::")[-1]


def defined(srcs):
    """name -> the source files that define a function of that name."""
    out = {}
    for name, text in srcs.items():
        for fn in set(_matches(_DEFN, text)):
            out.setdefault(fn, set()).add(name)
    return out


def stray_prototypes(root=CSRC):
    """(file, function) of every body-less declaration in a source file of a back-door function, or of a function that
    another source file defines."""
    srcs = sources(root)
    defs = defined(srcs)
    out = []
    for name, text in srcs.items():
        for fn in _matches(_DECL, text):
            if BACK_DOOR.match(fn) or (defs.get(fn, set()) - {name} and name not in defs.get(fn, set())):
                out.append((name, fn))
    return sorted(set(out))


def header_names(header, root=CSRC):
    return sorted(set(_matches(_DECL, _code((root / header).read_text()))))


def test_the_scan_reads_the_header_and_the_sources():
    names = header_names("host_internal.h")
    assert {"fail", "orbfe_extractor_consumer_begin_", "orbfe_remap_launch_", "orbfe_stereo_views_"} <= set(names), names
    names = header_names("extractor_handle.h")
    assert {"run_pipeline", "begin_call", "sync_all", "fetch_outputs"} <= set(names), names
    assert not {"stage_on", "stage_open", "stage_close", "StageTimer"} & set(names), names  # defined in the header itself
    defs = defined(sources())
    assert defs["orbfe_extract"] == {"extractor.hip"} and defs["orbfe_search_by_bow"] == {"matcher.hip"}
    assert defs["launch_search_by_bow"] == {"k_match.hip"} and defs["run_pipeline"] == {"extractor_pipeline.hip"}


def test_no_source_file_declares_another_files_function():
    assert not stray_prototypes(), "prototypes belong in a header (csrc/host_internal.h for the host back doors)"


@pytest.mark.parametrize("header", HEADERS)
def test_every_header_entry_is_defined_once_and_used_elsewhere(header):
    srcs = sources()
    defs = defined(srcs)
    names = header_names(header)
    assert names, f"the scan finds no declaration in csrc/{header}"
    for fn in names:
        where = defs.get(fn, set())
        assert len(where) == 1, f"{fn} (csrc/{header}) is defined in {sorted(where) or 'no source file'}"
        users = [n for n, t in srcs.items() if n not in where and re.search(r"\b" + fn + r"\s*\(", t)]
        assert users, f"{fn} (csrc/{header}) is used by no other source file: delete it, or make it static"


@pytest.mark.parametrize("header", HEADERS)
def test_every_user_and_definer_includes_the_header(header):
    srcs = sources()
    for fn in header_names(header):
        for n, t in srcs.items():
            if re.search(r"\b" + fn + r"\s*\(", t):
                assert f'#include "{header}"' in (CSRC / n).read_text(), f"{n} uses {fn} without including {header}"


def test_only_the_extractors_own_files_see_the_handle():
    """struct orbfe_extractor has one definition, and the matcher side keeps to the back doors of host_internal.h."""
    own = {"extractor_handle.hip", "extractor_pipeline.hip", "extractor.hip", "stereo_batch.hip", "extractor_debug.hip"}
    texts = {p.name: p.read_text() for p in CSRC.iterdir() if p.suffix in (".hip", ".h", ".cpp")}
    assert [n for n, t in texts.items() if "struct orbfe_extractor {" in t] == ["extractor_handle.h"]
    assert {n for n, t in texts.items() if '#include "extractor_handle.h"' in t} == own


def test_the_guard_notices_a_hand_copied_prototype(tmp_path):
    """A scratch copy of csrc/ whose vocabulary.hip declares one of the extractor's back doors itself again."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp"):
            (tmp_path / p.name).write_text(p.read_text())
    assert not stray_prototypes(tmp_path)
    v = tmp_path / "vocabulary.hip"
    v.write_text(v.read_text().replace(
        "static int bow_match_consecutive(",
        'extern "C" int orbfe_extractor_consumer_end_(orbfe_extractor* e);\nstatic int bow_match_consecutive(', 1))
    assert stray_prototypes(tmp_path) == [("vocabulary.hip", "orbfe_extractor_consumer_end_")]
    # ... and a public function of another file, declared at block scope
    m = tmp_path / "matcher.hip"
    m.write_text(m.read_text().replace("  GridFrame g{};", "  extern int orbfe_device_count(void);\n  GridFrame g{};", 1))
    assert ("matcher.hip", "orbfe_device_count") in stray_prototypes(tmp_path)
    # ... and a helper of extractor_handle.h, re-declared by one of the extractor's own files
    s = tmp_path / "stereo_batch.hip"
    s.write_text(s.read_text().replace(
        "using namespace orbfe;\n",
        "using namespace orbfe;\nnamespace orbfe {\nint run_pipeline(orbfe_extractor* e, LevelView level0, int nFrames, "
        "orbfe_keypoint* d_kp, uint8_t* d_desc, int capacity, int32_t* d_nOut);\n}\n", 1))
    assert ("stereo_batch.hip", "run_pipeline") in stray_prototypes(tmp_path)
