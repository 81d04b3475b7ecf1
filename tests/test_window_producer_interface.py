"""CPU drift guard of csrc/window_call.h: the window-search machinery (csrc/matcher.hip) reaches a prologue on the resident
map points through the Producer interface alone.  A kernel argument block, the table's device record or a prologue launch
named in matcher.hip, or a second producer member in WindowJob, would bring the per-producer branches back."""
import re
from pathlib import Path

from test_host_internal_header import _code

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
# what belongs to the producers (csrc/mappoints_search.hip) and the kernels
PRODUCER_ONLY = re.compile(r"\b(ProjectArgs|FuseArgs|TrackArgs|Sim3Args|MapPointsDevice|launch_project_\w*)\b")


def named_in_matcher(root=CSRC):
    return sorted({m.group(1) for m in PRODUCER_ONLY.finditer(_code((root / "matcher.hip").read_text()))})


def producer_members(root=CSRC):
    """the members of struct WindowJob whose type is a producer"""
    body = re.search(r"^struct WindowJob \{(.*?)^\};", _code((root / "window_call.h").read_text()), re.S | re.M).group(1)
    return re.findall(r"\b\w*Producer\s*\*\s*(\w+)", body)


def test_the_scan_reads_the_producers_and_the_machinery():
    search = _code((CSRC / "mappoints_search.hip").read_text())
    assert {"ProjectArgs", "FuseArgs", "TrackArgs", "Sim3Args", "MapPointsDevice", "launch_project_frustum", "launch_project_fuse",
            "launch_project_track", "launch_project_sim3"} <= {m.group(1) for m in PRODUCER_ONLY.finditer(search)}
    matcher = _code((CSRC / "matcher.hip").read_text())
    assert "window_search_multi" in matcher and '#include "window_call.h"' in (CSRC / "matcher.hip").read_text()
    assert len(re.findall(r"struct \w+ final : Producer", search)) == 4


def test_matcher_names_no_producer_type_and_no_prologue_launch():
    assert not named_in_matcher(), "reach a prologue through Producer (csrc/window_call.h)"


def test_a_window_job_has_one_producer_member():
    assert producer_members() == ["producer"]


def test_the_guard_notices_a_prologue_launch_in_matcher(tmp_path):
    """A scratch copy of csrc/ whose matcher.hip launches a prologue itself again, and one whose WindowJob names a second
    producer."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h"):
            (tmp_path / p.name).write_text(p.read_text())
    assert not named_in_matcher(tmp_path) and producer_members(tmp_path) == ["producer"]
    m = tmp_path / "matcher.hip"
    text = m.read_text()
    assert text.count("  if (P) TRY(P->launch(ar->stream));") == 1
    m.write_text(text.replace("  if (P) TRY(P->launch(ar->stream));", "  launch_project_fuse(ar->stream, fuseArgs);", 1))
    assert named_in_matcher(tmp_path) == ["launch_project_fuse"]
    h = tmp_path / "window_call.h"
    h.write_text(h.read_text().replace("  Producer* producer = nullptr;\n", "  Producer* producer = nullptr;\n  struct FuseProducer* fuse = nullptr;\n", 1))
    assert producer_members(tmp_path) == ["producer", "fuse"]
