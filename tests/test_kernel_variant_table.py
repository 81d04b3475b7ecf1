"""CPU drift guard of tests/kernel_variants.py: every run-time switch csrc/ reads is accounted for exactly once, and every
switch the tables name is still read -- a renamed switch would otherwise make its variant test the default form."""
import re
from pathlib import Path

import kernel_variants as kv

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"

# Per-handle switches: defaults of an orbfe_extractor_set_* / orbfe_set_* call that the GPU suite already drives through
# the setter (tests/test_gpu_extractor.py, tests/test_gpu_cpp_classes.py).
PER_HANDLE = {
    "ORBFE_STREAMS",        # set_streams
    "ORBFE_LANES",          # set_schedule
    "ORBFE_FAST_MODE",      # set_fast_mode
    "ORBFE_FUSED",          # set_fused
    "ORBFE_PYRBLUR",        # set_pyramid_blur
    "ORBFE_PYR_CHAIN",      # set_pyramid_chain
    "ORBFE_DESC_TILES",     # set_desc_tiles
    "ORBFE_BLUR_HFIRST",    # set_blur_pass_order
    "ORBFE_COPY_UNALIGNED",  # read at create: tests/test_gpu_kernel_variants.py sets it in process
}

# Switches that DO change results, by design: the blur arithmetic, and the profiling switches that cut work out of a
# kernel or a stage (the bench refuses their results unless told not to check).
NOT_RESULT_NEUTRAL = {
    "ORBFE_BLUR_SPEC",        # which OpenCV GaussianBlur arithmetic; set_blur_spec, tested per spec
    "ORBFE_FAST_CUTOFF",      # k_fast_cells stops after a phase
    "ORBFE_KNOCKOUT",         # skips a stage's launches
    "ORBFE_KNOCKOUT_AFTER",
    "ORBFE_BLUR_ABLATE",      # drops parts of a kernel's work
    "ORBFE_ORIENT_ABLATE",
    "ORBFE_DESC_TILES_ABLATE",
}

# Placement of the handle's streams on the hardware queues: what runs where, not what a kernel computes.
SCHEDULING_ONLY = {
    "ORBFE_STREAM_PRIORITY",
    "ORBFE_STREAM_SKEW",
}


def switches_in_csrc(root=CSRC):
    """Every ORBFE_* name read through getenv("...") or occupancy_pad_bytes("NAME") (-> ORBFE_PAD_NAME) in csrc/."""
    found = set()
    for p in sorted(root.iterdir()):
        if p.suffix not in (".hip", ".h", ".cpp"):
            continue
        text = p.read_text()
        found.update(re.findall(r'getenv\(\s*"(ORBFE_[A-Z0-9_]+)"\s*\)', text))
        found.update("ORBFE_PAD_" + n for n in re.findall(r'occupancy_pad_bytes\(\s*"([A-Z0-9_]+)"', text))
    return found


def variant_switches():
    return {k for v in kv.VARIANTS.values() for k in v.env}


def test_the_scan_finds_the_switches():
    found = switches_in_csrc()
    # known readers of each kind: a scan that broke (a moved directory, a changed helper) must not pass vacuously
    assert {"ORBFE_OCTREE_T", "ORBFE_ORIENT_KPB", "ORBFE_BLUR_TILE", "ORBFE_STREAMS", "ORBFE_PAD_OCTREE"} <= found, found
    assert len(found) >= 30, sorted(found)


def test_every_switch_is_in_exactly_one_list():
    lists = {"VARIANTS": variant_switches(), "PER_HANDLE": PER_HANDLE, "NOT_RESULT_NEUTRAL": NOT_RESULT_NEUTRAL,
             "SCHEDULING_ONLY": SCHEDULING_ONLY}
    for name in sorted(switches_in_csrc()):
        where = [k for k, s in lists.items() if name in s]
        assert len(where) == 1, f"{name} is read in csrc/ and listed in {where or 'no list'}: add a variant (or a list entry)"


def test_every_listed_switch_is_still_read():
    found = switches_in_csrc()
    for lst in (variant_switches(), PER_HANDLE, NOT_RESULT_NEUTRAL, SCHEDULING_ONLY):
        stale = sorted(lst - found)
        assert not stale, f"no longer read anywhere in csrc/: {stale} (renamed? the variant would test the default form)"


def test_variant_entries_are_well_formed():
    for name, v in kv.VARIANTS.items():
        assert v.name == name and v.env and v.doc, name
        assert all(k.startswith("ORBFE_") and isinstance(val, str) for k, val in v.env.items()), name


# Switches with more than one non-default form: each value selects another template instance, so each is its own entry.
MULTI_VALUED = {"ORBFE_ORIENT_KPB": {"128", "256"}}  # k_orient_desc<128, ...> / <256, ...> (default 64)


def test_every_value_of_a_multi_valued_switch_has_its_entry():
    for switch, values in MULTI_VALUED.items():
        got = {v.env[switch] for v in kv.VARIANTS.values() if switch in v.env}
        assert got == values, f"{switch}: variants for {sorted(got)}, the kernel forms are {sorted(values)}"


def test_the_guard_notices_a_renamed_switch(tmp_path):
    """A scratch copy of csrc/ with one getenv string renamed: the scan no longer finds the old name, so the reverse
    check reports the variant's switch as stale and the forward check the new name as unlisted."""
    for p in CSRC.iterdir():
        if p.suffix in (".hip", ".h", ".cpp"):
            (tmp_path / p.name).write_text(p.read_text().replace('getenv("ORBFE_BLUR_TILE")', 'getenv("ORBFE_BLUR_TILES")'))
    found = switches_in_csrc(tmp_path)
    assert "ORBFE_BLUR_TILE" not in found and "ORBFE_BLUR_TILES" in found
    assert "ORBFE_BLUR_TILE" in variant_switches() - found
