"""CPU drift guard for tests/stream_order.py: every cross-stream wait in csrc/ is pinned by a case or listed, with a reason,
in NOT_CASED -- in exactly one of the two -- and every listed site still exists.  A wait added later then needs a case.

A site key is "file:function:call(arguments)": the enclosing function (a top-level definition), the call
(hipStreamWaitEvent / hipEventSynchronize) and its arguments whitespace-normalised, hipStreamWaitEvent's flags dropped.
One key may stand for several lines (one event waited on in two places of one function)."""
import re
from collections import Counter
from pathlib import Path

import stream_order as so

CSRC = Path(__file__).resolve().parent.parent / "orb_slam2_annotate_amd" / "csrc"
CALLS = ("hipStreamWaitEvent", "hipEventSynchronize")
_DEF = re.compile(r'^(?:extern "C"\s+)?(?:static\s+|inline\s+)*[A-Za-z_][\w:<>,\*&\s]*?\b([A-Za-z_]\w*)\s*\(')


def _args(text, start):
    """The argument list of the call whose '(' is at text[start]."""
    depth, i = 0, start
    while True:
        c = text[i]
        depth += c == "("
        depth -= c == ")"
        if depth == 0:
            return text[start + 1:i]
        i += 1


def _split(args):
    out, depth, cur = [], 0, ""
    for c in args:
        if c in "([":
            depth += 1
        elif c in ")]":
            depth -= 1
        if c == "," and depth == 0:
            out.append(cur)
            cur = ""
        else:
            cur += c
    out.append(cur)
    return [" ".join(a.split()) for a in out]


def sites():
    """key -> number of call sites."""
    found = Counter()
    for path in sorted(list(CSRC.glob("*.hip")) + list(CSRC.glob("*.cpp")) + list(CSRC.glob("*.h"))):
        text = path.read_text()
        lines = text.split("\n")
        offsets, pos = [], 0
        for ln in lines:
            offsets.append(pos)
            pos += len(ln) + 1
        defs = []  # (line index, function name) of every top-level definition
        for i, ln in enumerate(lines):
            m = _DEF.match(ln)
            if not m or ln.startswith(("#", "//", "namespace", "struct", "using", "template", "return")):
                continue
            rest = "\n".join(lines[i:i + 6])
            brace, semi = rest.find("{"), rest.find(";")
            if brace >= 0 and (semi < 0 or brace < semi):
                defs.append((i, m.group(1)))
        for call in CALLS:
            for m in re.finditer(r"\b" + call + r"\s*\(", text):
                line = text.count("\n", 0, m.start())
                if lines[line].lstrip().startswith("//"):
                    continue
                func = [name for i, name in defs if i <= line][-1]
                a = _split(_args(text, m.end() - 1))
                if call == "hipStreamWaitEvent":
                    a = a[:2]
                found[f"{path.name}:{func}:{call}({', '.join(a)})"] += 1
    return found


def test_the_scan_finds_the_known_waits():
    s = sites()
    assert sum(s.values()) >= 20, s
    assert "extractor_pipeline.hip:run_pipeline:hipStreamWaitEvent(s, e->evConsumerDone)" in s
    assert "frames.hip:frame_use:hipStreamWaitEvent(ar->stream, f->ready)" in s


def test_every_wait_is_cased_or_listed_exactly_once():
    s = sites()
    listed = Counter()
    for case in so.CASES.values():
        listed.update(case.pins)
    listed.update(list(so.NOT_CASED))
    twice = sorted(k for k, n in listed.items() if n > 1)
    assert not twice, f"listed in more than one place: {twice}"
    missing = sorted(k for k in s if k not in listed)
    assert not missing, f"cross-stream waits in csrc/ that no stream_order case pins and NOT_CASED does not list: {missing}"
    gone = sorted(k for k in listed if k not in s)
    assert not gone, f"listed in stream_order.py but no longer in csrc/: {gone}"


def test_not_cased_reasons_are_one_line():
    for key, reason in so.NOT_CASED.items():
        assert reason.strip() and "\n" not in reason, key


def test_cases_have_docstrings_and_bugs_a_case():
    for name, case in so.CASES.items():
        assert case.run.__name__ == name and (case.run.__doc__ or "").strip(), name
        assert case.pins or case.bug, f"case {name} pins no wait and names no bug"
