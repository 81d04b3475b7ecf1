"""The drop-in wrappers with the reference's exact class signatures (include/ORBextractor.h,
include/ORBmatcher.h + src/ORBmatcher_orbfe.cc) need OpenCV and the reference's SLAM headers, neither of
which exists in this image, so they cannot be built here.  What can be checked: (1) they parse
(g++ -fsyntax-only, C++11 like the reference's CMakeLists.txt:13-25) against declaration-only stubs, which
catches typos and drift against orbfe_classes.hpp / orbfe.h; (2) the public method list of
include/ORBmatcher.h equals the reference header's, signature for signature (the reference's list is recorded in
tests/golden/orbmatcher_ref_methods.json by tools/gen_ref_golden.py)."""
import json
import re
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
STUBS = ROOT / "tests" / "cpp" / "stubs"
REF_METHODS = ROOT / "tests" / "golden" / "orbmatcher_ref_methods.json"


def _syntax(src: Path):
    p = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", f"-I{STUBS}", f"-I{ROOT / 'include'}", str(src)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]


def test_orbmatcher_dropin_parses():
    _syntax(ROOT / "src" / "ORBmatcher_orbfe.cc")


def test_orbextractor_dropin_parses(tmp_path):
    src = tmp_path / "use_extractor.cc"
    src.write_text('#include "ORBextractor.h"\n'
                   "int main() { ORB_SLAM2::ORBextractor e(1000, 1.2f, 8, 20, 7); cv::Mat im, d; std::vector<cv::KeyPoint> k;\n"
                   "  e(im, cv::Mat(), k, d); std::vector<float> s = e.GetScaleFactors(); return e.GetLevels() + (int)s.size() +\n"
                   "  (int)e.mvImagePyramid.size(); }\n")
    _syntax(src)


def _methods(text):
    """public member functions of class ORBmatcher as normalised 'ret name(arg types)' strings"""
    body = text[text.index("class ORBmatcher"):]
    body = body[:body.index("protected:")]
    body = re.sub(r"//[^\n]*", "", body)
    out = set()
    for m in re.finditer(r"(static\s+)?(int|float|bool)\s+(\w+)\s*\(([^;{]*)\)\s*;", body):
        args = []
        for a in m.group(4).split(","):
            a = re.sub(r"=[^,]*", "", a)             # default values
            a = a.replace("std::", "").replace("const ", "").strip()
            a = re.sub(r"\s*([&*<>])\s*", r"\1", a)
            a = re.sub(r"(\w+)$", "", a).strip() if re.search(r"[&*>\s]\w+$", a) else a   # drop the parameter name
            args.append(re.sub(r"\s+", " ", a))
        out.add(f"{m.group(2)} {m.group(3)}({', '.join(args)})")
    return out


def test_orbmatcher_header_has_the_reference_signatures():
    mine = _methods((ROOT / "include" / "ORBmatcher.h").read_text())
    ref = set(json.loads(REF_METHODS.read_text()))  # _methods() of the reference's include/ORBmatcher.h
    assert len(ref) == 12  # DescriptorDistance + the 11 searches of include/ORBmatcher.h:55-97
    assert mine == ref, f"only here: {sorted(mine - ref)}\nonly in the reference: {sorted(ref - mine)}"
