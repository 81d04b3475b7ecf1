"""CPU drift guard of csrc/arena.h, csrc/frame.h and csrc/mappoints.hip: the thread arena, the resident frames and the
map-point table are each owned by one file and reached through one interface.  A host file that begins the arena by a
hand-written size, names the thread-local state, or looks into a table handle would bring the second way back."""
import re
from pathlib import Path

from test_host_internal_header import _DEFN, _code

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
ARENA = {"arena.h", "arena.hip"}
# what only the arena's own files may name: the begin behind arena_stage / arena_stream, the hand sum's helper and the
# pinned mirror (a call reads it through mirror_of() and writes it through up() / up_pack() / up_fill() / put()); what
# only arena.hip may name: the thread-local state
ARENA_ONLY = re.compile(r"\b(arena_begin|arena_begin_owned|pad)\s*\(|\bhmirror\b")
STATE_ONLY = re.compile(r"\b(t_arenas|t_staging)\b")
# the scheme the graph and the database had before they owned an arena: a workspace and a pinned block on the handle, sized
# by hand sums and cut by offset tables
HANDLE_BLOCKS = re.compile(r"\b(obs_ensure_work|obs_al)\b|\b(?:g|db|held)\s*->\s*(?:work|pin)\b")
TABLE_ONLY = re.compile(r"\bmappoints_ready\b|\bmp\s*->\s*(?:slab|m|d)\b")


def files(root=CSRC):
    return {p.name: _code(p.read_text()) for p in sorted(root.iterdir()) if p.suffix in (".hip", ".cpp", ".h", ".inc")}


def named_outside(rx, owners, root=CSRC):
    """(file, name) of every match of rx in a file of csrc/ that is not one of `owners`."""
    return sorted({(n, m.group(0).split("(")[0].strip()) for n, t in files(root).items() if n not in owners
                   for m in rx.finditer(t)})


def defining(fn, root=CSRC):
    return [n for n, t in files(root).items() if any(m.group(2).split("::")[-1] == fn for m in _DEFN.finditer(t))]


def test_the_scan_reads_the_owners():
    f = files()
    assert ARENA_ONLY.search(f["arena.hip"]) and ARENA_ONLY.search(f["arena.h"])  # arena_begin: defined / behind arena_stage
    assert {m.group(1) for m in STATE_ONLY.finditer(f["arena.hip"])} == {"t_arenas", "t_staging"}
    assert TABLE_ONLY.search(f["mappoints.hip"])
    for way in ("arena_stage", "arena_stream"):
        users = [n for n, t in f.items() if n not in ARENA and re.search(r"\b" + way + r"\s*\(", t)]
        assert users, f"{way} (csrc/arena.h) is used by no other file"


def test_the_caller_laid_block_is_gone():
    assert not [p.name for p in sorted(CSRC.iterdir()) if p.is_file() and "arena_scratch" in p.read_text(errors="replace")]


def test_only_the_arena_begins_the_arena_and_nothing_sums_by_hand():
    assert not named_outside(ARENA_ONLY, ARENA), "carve inside arena_stage(), or take arena_stream(); reach the mirror through up*() / mirror_of()"


def test_no_handle_keeps_a_workspace_and_a_pinned_block_of_its_own():
    f = files()
    assert not named_outside(HANDLE_BLOCKS, set()), "stage through the handle's arena: arena_stage(&g->arena, g->device, stage)"
    for handle, owner in (("orbfe_obsgraph", "obsgraph_handle.h"), ("orbfe_kfdb", "kfdb.hip")):
        body = re.search(r"^struct\s+" + handle + r"\s*\{(.*?)^\};", f[owner], re.M | re.S).group(1)
        assert re.search(r"\bArena\s+arena\s*;", body), f"{handle} owns no arena"
        assert not re.search(r"\b(work|pin)\s*;", body), f"{handle} has a work / pin member again"
    for owner in ("obsgraph.hip", "kfpoints.hip", "obsdesc.hip", "loopcorrect.hip", "kfdb.hip"):
        assert re.search(r"\barena_stage\s*\(", f[owner]), f"{owner} stages nothing through the arena"


def test_the_thread_local_state_is_named_only_in_arena_hip():
    assert not named_outside(STATE_ONLY, {"arena.hip"})


def test_the_raw_pointer_back_door_is_gone():
    assert not [n for n, t in files().items() if "orbfe_thread_scratch_" in t]


def test_one_file_defines_each_pool_and_the_frame_ordering():
    assert defining("slab_get") == ["arena.hip"]
    assert defining("event_get") == ["arena.hip"]
    assert defining("frame_use") == ["frames.hip"]


def test_the_table_handle_is_private_to_mappoints_hip():
    owners = [n for n, t in files().items() if re.search(r"^struct\s+orbfe_mappoints\s*\{", t, re.M)]
    assert owners == ["mappoints.hip"], owners
    assert not named_outside(TABLE_ONLY, {"mappoints.hip"}), "reach the table through MapPointsLock (csrc/host_internal.h)"


def test_the_guard_notices_a_hand_summed_begin(tmp_path):
    """A scratch copy of csrc/ whose matcher.hip begins the arena by a size of its own again, one that writes the pinned
    mirror by hand, and one whose mappoints_search.hip looks into the table handle."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp", ".inc"):
            (tmp_path / p.name).write_text(p.read_text())
    assert not named_outside(ARENA_ONLY, ARENA, tmp_path) and not named_outside(TABLE_ONLY, {"mappoints.hip"}, tmp_path)
    m = tmp_path / "matcher.hip"
    text = m.read_text()
    assert text.count("  HIPCHK(arena_stage(device, &ar, stage));\n") >= 1
    m.write_text(text.replace("  HIPCHK(arena_stage(device, &ar, stage));\n", "  HIPCHK(arena_begin(device, 2 * n, &ar));\n", 1))
    assert named_outside(ARENA_ONLY, ARENA, tmp_path) == [("matcher.hip", "arena_begin")]
    m.write_text(text.replace("  HIPCHK(flush(ar));\n", "  std::memset(ar->hmirror, 0, 256);\n  HIPCHK(flush(ar));\n", 1))
    assert named_outside(ARENA_ONLY, ARENA, tmp_path) == [("matcher.hip", "hmirror")]
    m.write_text(text)
    s = tmp_path / "mappoints_search.hip"  # (where the searches on the table are)
    assert s.read_text().count("  MapPointsLock lock(mp);\n") >= 1
    s.write_text(s.read_text().replace("  MapPointsLock lock(mp);\n", "  std::lock_guard<std::mutex> lk(mp->m);\n", 1))
    assert named_outside(TABLE_ONLY, {"mappoints.hip"}, tmp_path) == [("mappoints_search.hip", "mp->m")]
    assert not named_outside(HANDLE_BLOCKS, set(), tmp_path)
    k = tmp_path / "kfpoints.hip"  # a call of the graph that reads its result from a pinned block of the handle again
    line = "  std::memcpy(count, mirror_of(ar, dCount), (size_t)n_kf * 4);\n"
    assert k.read_text().count(line) == 1
    k.write_text(k.read_text().replace(line, "  std::memcpy(count, g->pin, (size_t)n_kf * 4);\n"))
    assert named_outside(HANDLE_BLOCKS, set(), tmp_path) == [("kfpoints.hip", "g->pin")]
