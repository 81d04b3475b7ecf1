"""Engineered edge cases for the FeatureVector searches -- SearchByBoW in both forms and SearchForTriangulation, with the
rotation histogram they share -- and an independent plain-Python restatement of the three.  No GPU here:
tests/test_bow_edges.py pins the oracle (oracle/orb_oracle.c) to the restatement on every case and shows that each case takes
the branch it names and defeats the wrong readings it lists; tests/test_gpu_bow_edges.py runs the same cases through the
kernels of csrc/k_match.hip (k_search_by_bow<1|2|4>, k_search_by_bow_multi, k_search_by_bow_batch, k_search_triangulation,
k_search_triangulation_multi, k_rot_prune).

Restated from the reference, float steps in np.float32, double exactly where the reference promotes:

    CheckDistEpipolarLine                              src/ORBmatcher.cc:156-175
    SearchByBoW(KeyFrame, Frame)                       src/ORBmatcher.cc:185-325
    SearchByBoW(KeyFrame, KeyFrame)                    src/ORBmatcher.cc:610-743
    SearchForTriangulation                             src/ORBmatcher.cc:754-928
    ComputeThreeMaxima                                 src/ORBmatcher.cc:1777-1821 (window_edges.three_maxima)

Every restatement takes the operands the orc_* functions take and a tally that counts the same exits as
orc_bow_branch_counts under the names of oracle_lib.BOW_BRANCHES, plus the four histogram decisions of
oracle_lib.WINDOW_BRANCHES (HIST_BRANCHES below).

`variant` names one WRONG reading (VARIANTS); the restatement then computes that reading.  A case lists in `catches` the
variants whose answer on it differs from the right one: that is the proof that the case decides between the two, without a
mutated kernel.

Equal minima inside one BoW query: bestDist2 becomes bestDist1, and (float)b < nnratio * (float)b is false for every
nnratio <= 1, so with the reference's ratios "first minimum wins" never reaches the output -- the tie refuses under either
order.  The tie cases therefore come twice: at 0.75 (refused) and at nnratio = 1.5, which the constructor accepts like any
other float and which lets the tie pass, so that the position the kernels report is visible.
"""
from __future__ import annotations

import bisect
import dataclasses
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

from window_edges import HISTO_LENGTH, SF, TH_LOW, _prune, bits, c_round, f32, hamming, nxt, rot_bin, three_maxima

KINDS = ("bow_frame", "bow_kf", "tri")
HIST_BRANCHES = ("hist_pruned", "max2_below_tenth", "max3_below_tenth", "maxima_all_kept")
VARIANTS = ("low_inclusive_swapped", "ratio_exact", "ratio_le", "bow_last_min_wins", "tri_first_min_wins",
            "second_ignores_own_lane", "second_ignores_equal", "claim_not_seen", "claim_lost_across_64", "mask2_ignored",
            "tri_mask2_ignored", "only_stereo_ignores_candidate", "epipole_gate_on_stereo", "epipole_gate_le", "epipolar_fused",
            "epipolar_gate_float", "den_zero_passes", "bin_half_to_even", "bin_no_wrap", "maxima_ge", "tenth_le",
            "position_truncated_8bit")
SIGMA2 = (SF * SF).astype(np.float32)
VGA = (0.0, 640.0, 0.0, 480.0)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
f64 = np.float64


# ---- restatement ----------------------------------------------------------------------------------------------------
def featvec(nodes):
    """DBoW2::FeatureVector of addFeature(node[i], i), i ascending: (ascending node ids, per node the feature indices)"""
    nodes = [int(v) for v in nodes]
    ids = sorted(set(nodes))
    return ids, [[i for i, v in enumerate(nodes) if v == k] for k in ids]


def _walk(ids1, ids2, T):
    """std::map iteration with lower_bound, :211-300"""
    a = b = 0
    while a < len(ids1) and b < len(ids2):
        if ids1[a] == ids2[b]:
            T["node_shared"] += 1
            yield a, b
            a += 1; b += 1
        elif ids1[a] < ids2[b]:
            na = bisect.bisect_left(ids1, ids2[b])
            T["node_only_in_1"] += na - a; a = na
        else:
            nb = bisect.bisect_left(ids2, ids1[a])
            T["node_only_in_2"] += nb - b; b = nb


def _dist_matrix(d1, d2):
    if len(d1) == 0 or len(d2) == 0:
        return np.zeros((len(d1), len(d2)), np.int32)
    return _POP[d1[:, None, :] ^ d2[None, :, :]].sum(2)


def _bin(a1, a2, variant):
    """:274-279"""
    if variant not in ("bin_half_to_even", "bin_no_wrap"):
        return rot_bin(a1, a2)
    rot = f32(a1) - f32(a2)
    if float(rot) < 0.0 and variant != "bin_no_wrap":
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(1.0 / HISTO_LENGTH)))
    b = int(round(v)) if variant == "bin_half_to_even" else c_round(v)      # Python's round(): half to even
    return 0 if b == HISTO_LENGTH else b


def _maxima_variant(sizes, T, variant):
    """ComputeThreeMaxima with >= in the scan (maxima_ge) or <= at the tenth (tenth_le); sizes: bin -> count"""
    ge = (lambda s, m: s >= m) if variant == "maxima_ge" else (lambda s, m: s > m)
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = None
    for i in sorted(sizes):
        s = sizes[i]
        if ge(s, max1):
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif ge(s, max2):
            max3, max2, i3, i2 = max2, s, i2, i
        elif ge(s, max3):
            max3, i3 = s, i
    tenth = f32(0.1) * f32(max1)
    below = (lambda m: f32(m) <= tenth) if variant == "tenth_le" else (lambda m: f32(m) < tenth)
    if below(max2):
        i2 = i3 = None; T["max2_below_tenth"] += 1
    elif below(max3):
        i3 = None; T["max3_below_tenth"] += 1
    else:
        T["maxima_all_kept"] += 1
    return i1, i2, i3


def _prune_hist(entries, arr, T, variant):
    """:303-322.  entries: (bin, index into arr) in push order"""
    if variant not in ("maxima_ge", "tenth_le", "bin_no_wrap"):
        hist = [[] for _ in range(HISTO_LENGTH)]
        for b, j in entries:
            hist[b].append(j)
        return _prune(hist, arr, T)
    sizes = {b: 0 for b in range(HISTO_LENGTH)}      # (bin_no_wrap: a negative bin is a bin of its own, scanned first)
    for b, _ in entries:
        sizes[b] = sizes.get(b, 0) + 1
    keep = _maxima_variant(sizes, T, variant)
    removed = 0
    for b, j in entries:
        if b not in keep:
            arr[j] = -1; removed += 1; T["hist_pruned"] += 1
    return removed


def _ratio_ok(best1, best2, nnratio, variant):
    """:265 / :688 -- int to float, float product, float compare"""
    if variant == "ratio_exact":
        return float(best1) < float(f32(nnratio)) * float(best2)
    prod = f32(f32(nnratio) * f32(best2))
    return bool(f32(best1) <= prod) if variant == "ratio_le" else bool(f32(best1) < prod)


def search_bow(s1, s2, nnratio, check_ori, kf, variant=None):
    """src/ORBmatcher.cc:185-325 (kf False: vpMapPointMatches over the frame's features) and :610-743 (kf True:
    vpMatches12 over key frame 1's)"""
    T = Counter()
    strict = kf != (variant == "low_inclusive_swapped")                     # :263 <= TH_LOW, :686 < TH_LOW
    n1, n2 = len(s1["desc"]), len(s2["desc"])
    match = [-1] * (n1 if kf else n2)
    D = _dist_matrix(s1["desc"], s2["desc"])
    ids1, lists1 = featvec(s1["nodes"])
    ids2, lists2 = featvec(s2["nodes"])
    entries, nm = [], 0
    for a, b in _walk(ids1, ids2, T):
        L1, L2 = lists1[a], lists2[b]
        claimed = set()                                                     # positions in L2 (a feature lies in one node only)
        for qi, i1 in enumerate(L1):
            if variant == "claim_lost_across_64" and qi and qi % 64 == 0:
                claimed.clear()
            if not s1["has"][i1]:                                           # :225 / :647
                T["query_masked"] += 1
                continue
            best1, best2, bpos, cand = 256, 256, -1, []
            for p, i2 in enumerate(L2):
                if p in claimed and variant != "claim_not_seen":            # :242 / :664
                    T["cand_claimed"] += 1
                    continue
                if kf and not s2["has"][i2] and variant != "mask2_ignored":
                    T["cand_masked"] += 1
                    continue
                d = int(D[i1, i2])
                cand.append((p, d))
                if d < best1:                                               # :251-260
                    best2, best1, bpos = best1, d, p; T["better_best"] += 1
                elif d < best2:
                    T["equal_best_becomes_second" if d == best1 else "better_second"] += 1
                    best2 = d
                else:
                    T["not_better"] += 1
            if cand and variant == "bow_last_min_wins":
                bpos = max(p for p, d in cand if d == best1)
            elif cand and variant == "position_truncated_8bit":
                bpos = min((d, p & 255) for p, d in cand)[1]
            elif cand and variant == "second_ignores_own_lane":
                best2 = min([d for p, d in cand if p % 64 != bpos % 64], default=256)
            elif cand and variant == "second_ignores_equal":
                best2 = min([d for p, d in cand if d > best1], default=256)
            if (best1 < TH_LOW) if strict else (best1 <= TH_LOW):
                if _ratio_ok(best1, best2, nnratio, variant):
                    i2 = L2[bpos]
                    claimed.add(bpos)
                    out = i1 if kf else i2
                    match[out] = i2 if kf else i1
                    if check_ori:
                        entries.append((_bin(s1["ang"][i1], s2["ang"][i2], variant), out))
                    nm += 1; T["accepted"] += 1
                    if best1 == TH_LOW:
                        T["threshold_pass_at_50"] += 1
                    if best2 == 256:
                        T["ratio_second_is_256"] += 1
                else:
                    T["ratio_reject"] += 1
            elif bpos < 0:
                T["no_candidate"] += 1
            else:
                T["threshold_reject"] += 1
    if check_ori:
        nm -= _prune_hist(entries, match, T, variant)
    return (nm, match), T


def epipolar_terms(x1, y1, x2, y2, F, fused=False):
    """:159-165 -> (num, den); fused: every sum of products evaluated in double and rounded once"""
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    F = np.asarray(F, np.float32).reshape(9)
    if fused:
        line = [f32(f64(x1) * f64(F[k]) + f64(y1) * f64(F[3 + k]) + f64(F[6 + k])) for k in range(3)]
        a, b, c = line
        return f32(f64(a) * f64(x2) + f64(b) * f64(y2) + f64(c)), f32(f64(a) * f64(a) + f64(b) * f64(b))
    a, b, c = [f32(f32(f32(x1 * F[k]) + f32(y1 * F[3 + k])) + F[6 + k]) for k in range(3)]
    return f32(f32(f32(a * x2) + f32(b * y2)) + c), f32(f32(a * a) + f32(b * b))


def _epipolar_ok(x1, y1, x2, y2, F, sigma2, T, variant):
    """CheckDistEpipolarLine, :156-175"""
    num, den = epipolar_terms(x1, y1, x2, y2, F, variant == "epipolar_fused")
    if den == 0:                                                            # :167
        if variant == "den_zero_passes":
            return True
        T["tri_den_zero"] += 1
        return False
    dsqr = f32(f32(num * num) / den)                                        # :170
    if variant == "epipolar_gate_float":
        ok = bool(dsqr < f32(f32(3.84) * f32(sigma2)))
    else:
        ok = float(dsqr) < 3.84 * float(f32(sigma2))                        # :172 float < double * float: in double
    if not ok:
        T["tri_epipolar_reject"] += 1
    return ok


def search_tri(s1, s2, F12, ex, ey, sf2, sig2, only_stereo, check_ori, variant=None):
    """src/ORBmatcher.cc:754-928"""
    T = Counter()
    n1 = len(s1["desc"])
    match = [-1] * n1
    D = _dist_matrix(s1["desc"], s2["desc"])
    ids1, lists1 = featvec(s1["nodes"])
    ids2, lists2 = featvec(s2["nodes"])
    entries, nm = [], 0
    ex, ey = f32(ex), f32(ey)
    for a, b in _walk(ids1, ids2, T):
        L2 = lists2[b]
        for i1 in lists1[a]:
            if s1["has"][i1]:                                               # :802
                T["tri_query_has_mp"] += 1
                continue
            st1 = float(s1["ur"][i1]) >= 0                                  # :805
            if only_stereo and not st1:
                T["tri_query_mono_only_stereo"] += 1
                continue
            best, bi, passed = TH_LOW, -1, []
            for p, i2 in enumerate(L2):
                if s2["has"][i2] and variant != "tri_mask2_ignored":        # :827 (vbMatched2 is never set)
                    T["tri_cand_has_mp"] += 1
                    continue
                st2 = float(s2["ur"][i2]) >= 0
                if only_stereo and not st2 and variant != "only_stereo_ignores_candidate":
                    T["tri_cand_mono_only_stereo"] += 1
                    continue
                d = int(D[i1, i2])
                if d > TH_LOW:                                              # :840
                    T["tri_dist_above_th"] += 1
                    continue
                if d > best or (variant == "tri_first_min_wins" and d == best and bi >= 0):
                    T["tri_dist_above_best"] += 1
                    continue
                o = int(s2["oct"][i2])
                if (not st1 and not st2) or variant == "epipole_gate_on_stereo":         # :845-854
                    dx, dy = f32(ex - f32(s2["x"][i2])), f32(ey - f32(s2["y"][i2]))
                    lhs, rhs = f32(f32(dx * dx) + f32(dy * dy)), f32(f32(100.0) * f32(sf2[o]))
                    if (lhs <= rhs) if variant == "epipole_gate_le" else (lhs < rhs):
                        T["tri_epipole_reject"] += 1
                        continue
                else:
                    T["tri_epipole_skipped_stereo"] += 1
                if _epipolar_ok(s1["x"][i1], s1["y"][i1], s2["x"][i2], s2["y"][i2], F12, sig2[o], T, variant):   # :856
                    T["tri_first_accept" if bi < 0 else "tri_replaced_equal" if d == best else "tri_replaced_smaller"] += 1
                    best, bi = d, i2
                    passed.append((p, d))
            if passed and variant == "position_truncated_8bit":
                bi = L2[255 - min((d, 255 - (p & 255)) for p, d in passed)[1]]
            if bi >= 0:                                                     # :863
                match[i1] = bi
                nm += 1; T["accepted"] += 1
                if check_ori:
                    entries.append((_bin(s1["ang"][i1], s2["ang"][bi], variant), i1))
            else:
                T["tri_no_match"] += 1
    if check_ori:
        nm -= _prune_hist(entries, match, T, variant)
    return (nm, match), T


# ---- cases ----------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    kind: str                      # one of KINDS
    s1: dict                       # desc, nodes, has, ang, x, y, oct, ur of side 1 (the key frame whose features are the queries)
    s2: dict                       # the same of side 2 (the searched frame / key frame)
    nnratio: float = 0.75
    check_ori: bool = False
    tri: dict = field(default_factory=dict)       # F12, ex, ey, sf2, sig2, only_stereo
    expect: dict = field(default_factory=dict)    # branch -> exact count the oracle must report
    want: object = None            # the match array spelled out
    catches: tuple = ()            # variants whose answer differs on this case


Z = np.zeros(32, np.uint8)
ONE = bits(1, 255)                 # a query at distance 1 from the zero descriptor: bits(d - 1) is d away, both <= 50 bits
F_LINE_Y0 = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0], np.float32)     # with x1 = y1 = 0: the line y = 0, den = 1, dsqr = y2^2
FAR = 1000.0


def side(desc, nodes=None, has=None, ang=None, x=None, y=None, octave=None, ur=None, active=1):
    """one side's arrays; defaults: one node (id 7), every feature active, angle 0, position (0, 0), octave 0, monocular"""
    n = len(desc)
    arr = lambda v, d, t: np.full(n, d, t) if v is None else np.asarray(v, t).reshape(n)  # noqa: E731
    return dict(desc=np.stack(desc).astype(np.uint8) if n else np.zeros((0, 32), np.uint8),
                nodes=arr(nodes, 7, np.int64), has=arr(has, active, np.uint8), ang=arr(ang, 0.0, np.float32),
                x=arr(x, 0.0, np.float32), y=arr(y, 0.0, np.float32), oct=arr(octave, 0, np.int32), ur=arr(ur, -1.0, np.float32))


def tri_args(**kw):
    d = dict(F12=F_LINE_Y0, ex=FAR, ey=FAR, sf2=SF, sig2=SIGMA2, only_stereo=False)
    d.update(kw)
    return d


def mk(name, kind, q, c, expect=None, want=None, catches=(), nnratio=0.75, check_ori=False, s1=None, s2=None, **tri):
    """q / c: descriptor lists of side 1 / side 2 (or ready sides through s1 / s2).  "has" means "takes part": for the two
    BoW forms a feature with a map point, for triangulation one without"""
    act = 0 if kind == "tri" else 1
    s1 = side(q, active=act) if s1 is None else s1
    s2 = side(c, active=act) if s2 is None else s2
    return Case(name, kind, s1, s2, nnratio, check_ori, tri_args(**tri) if kind == "tri" else {}, dict(expect or {}), want,
                tuple(catches))


def ratio_rounding_pairs(nnratio):
    """(best1, best2), best1 <= TH_LOW, where the float product nnratio * best2 rounds to exactly best1 although the real
    product is larger: the reference refuses, an unrounded or fused evaluation accepts"""
    r = f32(nnratio)
    out = []
    for b1 in range(1, TH_LOW + 1):
        for b2 in range(b1, 257):
            if _ratio_ok(b1, b2, r, None) != _ratio_ok(b1, b2, r, "ratio_exact"):
                out.append((b1, b2))
    return out


def threshold_cases():
    out = []
    for kind in ("bow_frame", "bow_kf"):
        for d in (49, 50, 51):
            for far in (256, 100):
                cand = [bits(d - 1)] + ([bits(99, 100)] if far == 100 else [])
                ok = d <= 50 if kind == "bow_frame" else d < 50
                exp = dict(accepted=int(ok), threshold_reject=int(not ok), ratio_second_is_256=int(ok and far == 256))
                if kind == "bow_frame":
                    exp["threshold_pass_at_50"] = int(d == 50)
                w = [0 if ok else -1] + [-1] * (far == 100) if kind == "bow_frame" else [0 if ok else -1]
                out.append(mk(f"{kind}_best_{d}_second_{far}", kind, [ONE], cand, exp, w,
                              ("low_inclusive_swapped",) if d == 50 else ()))
    for d in (50, 51):
        out.append(mk(f"tri_best_{d}", "tri", [ONE], [bits(d - 1)], dict(accepted=int(d == 50), tri_dist_above_th=int(d == 51),
                                                                          tri_first_accept=int(d == 50), tri_no_match=int(d == 51)),
                      [0 if d == 50 else -1]))
    # nothing left to compare with: the only candidate is claimed by the first query / masked
    out.append(mk("bow_frame_no_candidate_all_claimed", "bow_frame", [Z, Z], [bits(5)], dict(no_candidate=1, cand_claimed=1, accepted=1), [0]))
    out.append(mk("bow_kf_no_candidate_all_masked", "bow_kf", [Z], None, dict(no_candidate=1, cand_masked=2), [-1],
                  s2=side([bits(5), bits(6)], has=[0, 0])))
    out.append(mk("tri_no_candidate_all_with_map_point", "tri", [Z], None, dict(tri_no_match=1, tri_cand_has_mp=2), [-1],
                  s2=side([bits(5), bits(6)], has=[1, 1])))
    return out


def ratio_cases():
    out = []
    for kind in ("bow_frame", "bow_kf"):
        # integer-exact equality: 0.75f * 40 = 30 exactly, 30 < 30 is false
        out.append(mk(f"{kind}_ratio_0.75_30_40_equal", kind, [Z], [bits(30), bits(40, 100)], dict(ratio_reject=1), None, ("ratio_le",)))
        out.append(mk(f"{kind}_ratio_0.75_30_41_passes", kind, [Z], [bits(30), bits(41, 100)], dict(accepted=1, better_second=1)))
        for r in (0.6, 0.8):
            pairs = ratio_rounding_pairs(r)
            assert pairs, r
            for b1, b2 in pairs:
                out.append(mk(f"{kind}_ratio_{r}_{b1}_{b2}_rounds_to_equal", kind, [Z], [bits(b1), bits(b2, 100)], dict(ratio_reject=1),
                              [-1, -1] if kind == "bow_frame" else [-1], ("ratio_exact", "ratio_le"), nnratio=r))
                out.append(mk(f"{kind}_ratio_{r}_{b1}_{b2 + 1}_passes", kind, [Z], [bits(b1), bits(b2 + 1, 100)], dict(accepted=1),
                              [0, -1] if kind == "bow_frame" else [0], nnratio=r))
    return out


CNT2 = (2, 64, 65, 128, 129, 256, 257, 300)


def _cands(cnt2, placed, filler=40):
    """cnt2 candidate descriptors at distance `filler` from Z except the placed {position: distance}"""
    return [bits(placed.get(p, filler), (p * 3) % 200) for p in range(cnt2)]


def _want(kind, cnt2, pos):
    """match array of a one-query case whose answer is candidate `pos` (None: no match)"""
    if kind == "bow_frame":
        w = [-1] * cnt2
        if pos is not None:
            w[pos] = 0
        return w
    return [-1 if pos is None else pos]


def reduction_cases():
    out = []
    for cnt2 in CNT2:
        for kind in KINDS:
            bow = kind != "tri"
            # the best alone at a chosen position (second best: the filler, 10 < 0.75 * 40)
            for pos in sorted({0, 63, 64, cnt2 - 1}):
                if pos < cnt2:
                    cat = ("position_truncated_8bit",) if pos > 255 else ()
                    out.append(mk(f"{kind}_cnt2_{cnt2}_best_at_{pos}", kind, [Z], _cands(cnt2, {pos: 10}), dict(accepted=1),
                                  _want(kind, cnt2, pos), cat))
            # the second best in the winner's own lane (p, p + 64, p + 128): 10 < 0.75 * 12 = 9 is false
            for gap in (64, 128):
                if 1 + gap < cnt2 and bow:
                    out.append(mk(f"{kind}_cnt2_{cnt2}_second_in_own_lane_plus_{gap}", kind, [Z], _cands(cnt2, {1: 10, 1 + gap: 12}),
                                  dict(ratio_reject=1), _want(kind, cnt2, None), ("second_ignores_own_lane",)))
                    out.append(mk(f"{kind}_cnt2_{cnt2}_second_first_in_own_lane_plus_{gap}", kind, [Z], _cands(cnt2, {1: 12, 1 + gap: 10}),
                                  dict(ratio_reject=1), _want(kind, cnt2, None), ("second_ignores_own_lane",)))
            # the second best equal to the best, in another lane: refused (10 < 0.75 * 10 is false)
            if bow:
                for a, b in ((0, cnt2 - 1), (63, 64), (5, 69), (3, 259)):
                    if a < b < cnt2:
                        # 0.75: the tie refuses whichever of the two is called the best; 1.5: it passes and the FIRST is matched
                        out.append(mk(f"{kind}_cnt2_{cnt2}_equal_minima_{a}_{b}_refused", kind, [Z], _cands(cnt2, {a: 10, b: 10}),
                                      dict(ratio_reject=1, equal_best_becomes_second=1 + (a >= 2)), _want(kind, cnt2, None),
                                      ("second_ignores_equal",)))    # (a >= 2: the second of the fillers before `a` counts too)
                        out.append(mk(f"{kind}_cnt2_{cnt2}_equal_minima_{a}_{b}_first_wins", kind, [Z], _cands(cnt2, {a: 10, b: 10}),
                                      dict(accepted=1, equal_best_becomes_second=1 + (a >= 2)), _want(kind, cnt2, a), ("bow_last_min_wins",),
                                      nnratio=1.5))
            else:
                for a, b in ((0, cnt2 - 1), (63, 64), (5, 69), (3, 259)):
                    if a < b < cnt2:
                        cat = ("tri_first_min_wins",) + (("position_truncated_8bit",) if b > 255 else ())
                        out.append(mk(f"tri_cnt2_{cnt2}_equal_minima_{a}_{b}_last_wins", "tri", [Z], _cands(cnt2, {a: 10, b: 10}),
                                      dict(accepted=1, tri_replaced_equal=max(a, 1)), [b], cat))    # (the fillers before `a` tie too)
    return out


def claim_cases():
    out = []
    W = bits(30, 100)
    for kind in ("bow_frame", "bow_kf"):
        fr = kind == "bow_frame"
        # both queries prefer candidate 0: the second takes its runner-up ...
        out.append(mk(f"{kind}_second_query_takes_runner_up", kind, [Z, Z], [bits(5), bits(9, 50)], dict(accepted=2, cand_claimed=1),
                      [0, 1], ("claim_not_seen",)))
        # ... or fails the ratio test it would have passed with the claimed one (20 < 0.75 * 22 is false)
        out.append(mk(f"{kind}_claim_removes_the_best_ratio_fails", kind, [Z, Z], [bits(5), bits(20, 50), bits(22, 100)],
                      dict(accepted=1, cand_claimed=1, ratio_reject=1), [0, -1, -1] if fr else [0, -1], ("claim_not_seen",)))
        # the claim of query 63 must be seen by query 64 (and of 127 by 128): the others are far from everything
        for cnt1 in (65, 129):
            q = [bits(200)] * cnt1
            q[63] = q[64] = Z
            c = [bits(5), bits(9, 50)]
            w = {63: 0, 64: 1}
            if cnt1 == 129:
                q[127] = q[128] = W
                c += [W ^ bits(5), W ^ bits(9, 50)]
                w.update({127: 2, 128: 3})
            want = [k for k, _ in sorted(w.items(), key=lambda kv: kv[1])] if fr else [w.get(i, -1) for i in range(cnt1)]
            out.append(mk(f"{kind}_cnt1_{cnt1}_claim_crosses_64", kind, q, c, dict(accepted=len(w), threshold_reject=cnt1 - len(w)), want,
                          ("claim_lost_across_64", "claim_not_seen")))
        # a query without a map point is skipped before it can claim
        out.append(mk(f"{kind}_masked_query_claims_nothing", kind, None, [bits(5), bits(9, 50)], dict(query_masked=1, accepted=1, cand_claimed=0),
                      [1, -1] if fr else [-1, 0], s1=side([Z, Z], has=[0, 1])))
    out.append(mk("bow_kf_masked_candidate_is_not_the_best", "bow_kf", [Z], None, dict(cand_masked=1, accepted=1, ratio_second_is_256=1), [1],
                  ("mask2_ignored",), s2=side([bits(5), bits(9, 50)], has=[0, 1])))
    return out


def _per_node(sizes, ids, nq=2):
    """one call with a node per entry of `sizes`: nq queries (Z, then a copy) and that many candidates, the best last"""
    d1, n1, d2, n2 = [], [], [], []
    for sz, nid in zip(sizes, ids):
        d1 += [Z] * nq; n1 += [nid] * nq
        d2 += _cands(sz, {sz - 1: 10, 0: 14}) if sz > 1 else [bits(10)]
        n2 += [nid] * sz
    return side(d1, n1), side(d2, n2)


def shape_cases():
    out = []
    for kind in ("bow_frame", "bow_kf"):
        for tag, sizes in (("nodes_10_100_200_300", (10, 100, 200, 300)), ("max_100", (30, 100, 64)), ("max_64", (64, 1, 17))):
            s1, s2 = _per_node(sizes, [11 * (k + 1) for k in range(len(sizes))])
            # per node: query 0 takes the last candidate (10 < 0.75 * 14), query 1 then candidate 0 (14 < 0.75 * 40)
            out.append(mk(f"{kind}_{tag}", kind, None, None, dict(node_shared=len(sizes), cand_claimed=len(sizes)), s1=s1, s2=s2,
                          catches=("position_truncated_8bit",) if max(sizes) > 256 else ()))
        # node-id walk: first and last shared, nodes only on one side in between, ids up to 2^31
        one = lambda ids: side([bits(k + 1, 9 * k) for k in range(len(ids))], ids)  # noqa: E731
        out.append(mk(f"{kind}_node_walk_sparse_ids", kind, None, None, dict(node_shared=3, node_only_in_1=1, node_only_in_2=2, accepted=3),
                      s1=one([1, 5, 9, 2 ** 31]), s2=one([1, 4, 6, 9, 2 ** 31])))
        out.append(mk(f"{kind}_node_walk_single_node_side_1", kind, None, None, dict(node_shared=1, node_only_in_2=2, accepted=1),
                      s1=one([9]), s2=one([1, 4, 9, 12])))
        out.append(mk(f"{kind}_node_walk_single_node_side_2", kind, None, None, dict(node_shared=1, node_only_in_1=3, accepted=1),
                      s1=one([1, 4, 5, 2 ** 31 - 1, 2 ** 31 + 5]), s2=one([2 ** 31 - 1])))
        out.append(mk(f"{kind}_disjoint_node_sets", kind, None, None, dict(node_shared=0, accepted=0), s1=one([2, 4, 6]), s2=one([1, 3, 5, 7])))
        out.append(mk(f"{kind}_empty_frames", kind, [], [], dict(node_shared=0), []))
        # 50 identical descriptors in one node: every query ties, the ratio test refuses all (from test_bow_edge_cases)
        ang = np.linspace(0, 359, 50).astype(np.float32)
        out.append(mk(f"{kind}_all_identical_descriptors", kind, None, None, dict(ratio_reject=50, equal_best_becomes_second=50),
                      [-1] * 50, ("second_ignores_equal",), check_ori=True, s1=side([Z] * 50, ang=ang), s2=side([Z] * 50, ang=ang)))
    return out


def sum_of_squares_operands(target):
    """floats (dx, dy) with fl(fl(dx*dx) + fl(dy*dy)) == target, found by stepping dy"""
    target = f32(target)
    dx = f32(0.8 * np.sqrt(float(target)))
    dy0 = f32(np.sqrt(float(target) - float(dx) ** 2))
    dy = (dy0.view(np.int32) + np.arange(-4096, 4097, dtype=np.int32)).view(np.float32)
    got = ((dx * dx).astype(np.float32) + (dy * dy).astype(np.float32)).astype(np.float32)
    k = np.flatnonzero(got == target)
    assert k.size, target
    return dx, dy[k[0]]


def dsqr_operands(target):
    """floats (la, lb, lc) with fl(fl(lc*lc) / fl(fl(la*la) + fl(lb*lb))) == target, la = 1: found by stepping lb"""
    target = f32(target)
    for lc in (f32(m * 2.0 ** e) for e in range(-6, 8) for m in (1.0, 1.5, 1.25, 1.75)):
        d0 = float(lc) ** 2 / float(target)
        if not 1.05 < d0 < 1.95:
            continue
        lb0 = f32(np.sqrt(d0 - 1.0))
        lb = (lb0.view(np.int32) + np.arange(-20000, 20001, dtype=np.int32)).view(np.float32)
        den = (f32(1.0) + (lb * lb).astype(np.float32)).astype(np.float32)
        got = ((lc * lc).astype(np.float32) / den).astype(np.float32)
        k = np.flatnonzero(got == target)
        if k.size:
            return f32(1.0), lb[k[0]], lc
    raise AssertionError(("no operands", target))


def gate_floats(sigma2):
    """the floats around the double 3.84 * sigma2: (largest below it, smallest not below it)"""
    t = 3.84 * float(f32(sigma2))
    lo = f32(t)
    if float(lo) >= t:
        lo = nxt(lo, False)
    assert float(lo) < t <= float(nxt(lo))
    return lo, nxt(lo)


def float_gate_sigma():
    """a level sigma^2 in the range dsqr_operands() reaches for which dsqr < 3.84f * sigma2 in float and the reference's
    double compare disagree on one of the two floats around the limit -> (sigma2, that float)"""
    s = f32(1.21)
    for _ in range(100000):
        lo, hi = gate_floats(s)
        g = f32(f32(3.84) * s)
        if not lo < g:
            return s, lo          # double: passes; float: refuses
        if hi < g:
            return s, hi          # double: refuses; float: passes
        s = nxt(s)
    raise AssertionError("no sigma")


def fused_tuple():
    """(x1, y1, F12, x2, y2, sigma2): unfused and fused num / den give different dsqr, and sigma2 puts the double gate
    between them; found by a seeded search in the way of window_edges.fma_triple"""
    rng = np.random.default_rng(11)
    while True:
        x1, y1, x2, y2 = [f32(v) for v in rng.uniform(50, 600, 4)]
        F = (rng.uniform(-1, 1, 9) * [1e-6, 1e-5, 1e-3, 1e-5, 1e-6, 1e-3, 1e-3, 1e-3, 0.3]).astype(np.float32)
        (n0, d0), (n1, d1) = epipolar_terms(x1, y1, x2, y2, F), epipolar_terms(x1, y1, x2, y2, F, True)
        if d0 == 0 or d1 == 0:
            continue
        a, b = f32(f32(n0 * n0) / d0), f32(f32(n1 * n1) / d1)
        if a == b or not 1e-3 < min(a, b) < 1e3:
            continue
        lo, hi = (a, b) if a < b else (b, a)
        s = f32(float(hi) / 3.84)
        for cand in (nxt(s, False), s, nxt(s)):
            if float(lo) < 3.84 * float(cand) <= float(hi):
                return x1, y1, F, x2, y2, cand


def tri_cases():
    out = []
    T = lambda name, q, c, expect, want, catches=(), **kw: out.append(mk(name, "tri", q, c, expect, want, catches, **kw))  # noqa: E731
    T("tri_query_with_map_point_skipped", None, [bits(5)], dict(tri_query_has_mp=1, accepted=1), [-1, 0], s1=side([Z, Z], has=[1, 0]))
    T("tri_mono_query_under_only_stereo", None, None, dict(tri_query_mono_only_stereo=1, accepted=1, tri_epipole_skipped_stereo=1), [-1, 0],
      s1=side([Z, Z], has=[0, 0], ur=[-1, 3]), s2=side([bits(5)], has=[0], ur=[2]), only_stereo=True)
    T("tri_candidate_with_map_point_skipped", [Z], None, dict(tri_cand_has_mp=1, accepted=1), [1], ("tri_mask2_ignored",),
      s2=side([bits(5), bits(9, 50)], has=[1, 0]))
    T("tri_mono_candidate_under_only_stereo", None, None, dict(tri_cand_mono_only_stereo=1, accepted=1), [1], ("only_stereo_ignores_candidate",),
      s1=side([Z], has=[0], ur=[0.0]), s2=side([bits(5), bits(9, 50)], has=[0, 0], ur=[-1, 0.0]), only_stereo=True)
    # bestDist moves only on a pass: 5 fails the epipolar test (y2 = 50 off the line y = 0), the later 9 is taken; then the
    # later smaller / equal / larger ones
    T("tri_smaller_fails_epipolar_larger_taken", [Z], None, dict(tri_epipolar_reject=1, tri_first_accept=1, accepted=1), [1],
      s2=side([bits(5), bits(9, 50)], has=[0, 0], y=[50.0, 0.0]))
    T("tri_replaced_by_smaller_equal_then_larger_refused", [Z], [bits(9), bits(5, 50), bits(5, 100), bits(7, 150)],
      dict(tri_first_accept=1, tri_replaced_smaller=1, tri_replaced_equal=1, tri_dist_above_best=1), [2], ("tri_first_min_wins",))
    # the epipole gate: |e - kp2|^2 one float below / at / above 100 * scaleFactor[octave]; the line passes through kp2
    for o in (0, 1):
        lim = f32(f32(100.0) * SF[o])
        for tag, lhs in (("below", nxt(lim, False)), ("at", lim), ("above", nxt(lim))):
            dx, dy = sum_of_squares_operands(lhs)
            x2, y2, ex, ey = dx, dy, f32(0.0), f32(0.0)          # the epipole at the origin: ex - x2 = -dx exactly
            F = np.array([0, 0, 0, 0, 0, 0, 0, 1, -y2], np.float32)
            rej = tag == "below"
            for st_tag, ur1, ur2 in (("mono_mono", -1, -1), ("query_stereo", 0.0, -1), ("candidate_stereo", -1, 0.0)):
                mono = st_tag == "mono_mono"
                exp = dict(tri_epipole_reject=int(rej and mono), tri_epipole_skipped_stereo=int(not mono), accepted=int(not (rej and mono)))
                cat = (("epipole_gate_le",) if tag == "at" and mono else ()) + (("epipole_gate_on_stereo",) if rej and not mono else ())
                T(f"tri_epipole_{tag}_octave_{o}_{st_tag}", None, None, exp, [-1 if rej and mono else 0], cat,
                  s1=side([Z], has=[0], ur=[ur1]), s2=side([bits(5)], has=[0], x=[x2], y=[y2], octave=[o], ur=[ur2]), F12=F, ex=ex, ey=ey)
    # den == 0: F12 zero, and la = lb = 0 with lc != 0
    for tag, F in (("f12_zero", np.zeros(9, np.float32)), ("only_lc", np.array([0, 0, 0, 0, 0, 0, 0, 0, 1], np.float32))):
        T(f"tri_den_zero_{tag}", [Z], [bits(5)], dict(tri_den_zero=1, tri_no_match=1), [-1], ("den_zero_passes",), F12=F)
    # dsqr one float below / at / above the double 3.84 * sigma2: x1 = y1 = x2 = y2 = 0, so la, lb, lc, num are F12's last row
    gs, gd = float_gate_sigma()
    for tag, s2v in (("sf_octave_1", SIGMA2[1]), ("float_gate_disagrees", gs)):
        lo, hi = gate_floats(s2v)
        sig = SIGMA2.copy()
        sig[0] = s2v
        for pos, dsqr in (("below", nxt(lo, False)), ("at", lo), ("above", hi)):
            la, lb, lc = dsqr_operands(dsqr)
            ok = pos != "above"
            cat = ("epipolar_gate_float",) if tag == "float_gate_disagrees" and dsqr == gd else ()
            T(f"tri_dsqr_{pos}_gate_{tag}", [Z], [bits(5)], dict(tri_epipolar_reject=int(not ok), accepted=int(ok)), [0 if ok else -1], cat,
              F12=np.array([0, 0, 0, 0, 0, 0, la, lb, lc], np.float32), sig2=sig)
    x1, y1, F, x2, y2, s2v = fused_tuple()
    sig = SIGMA2.copy()
    sig[0] = s2v
    T("tri_epipolar_terms_not_contracted", None, None, {}, None, ("epipolar_fused",), s1=side([Z], has=[0], x=[x1], y=[y1], ur=[0.0]),
      s2=side([bits(5)], has=[0], x=[x2], y=[y2]), F12=F, sig2=sig)
    # the 4-queries-per-workgroup split and the 64-stride of the candidate scan: query i wants candidate (7 i) mod cnt2
    for nq in (1, 3, 4, 5, 9):
        for cnt2 in (1, 64, 65, 130):
            P = [bits(24, 28 * i) for i in range(nq)]
            c = [bits(200)] * cnt2
            w = []
            for i in range(nq):
                p = (7 * i) % cnt2
                if cnt2 > 1 or i == 0:
                    c[p] = P[i] ^ bits(3, 252)
                w.append(p if cnt2 > 1 or i == 0 else -1)
            T(f"tri_nq_{nq}_cnt2_{cnt2}", P, c, dict(accepted=sum(v >= 0 for v in w)), w)
    return out


def half_way_angles():
    """float angle pairs (a1, a2) whose rot * (1/30f) is exactly k + 0.5 with k even: round() gives k + 1, half-to-even k"""
    out = []
    for a2 in (0.0, 7.5, 11.25):
        for a1 in np.arange(0.0, 360.0, 0.125, dtype=np.float32):
            rot = f32(a1) - f32(a2)
            if rot < 0:
                continue
            v = float(f32(rot * f32(1.0 / HISTO_LENGTH)))
            if v - np.floor(v) == 0.5 and int(np.floor(v)) % 2 == 0:
                out.append((float(a1), a2, int(np.floor(v)) + 1))
    return out


def _pairs_case(name, kind, pairs, expect, want=None, catches=(), check_ori=True):
    """one node per (angle 1, angle 2) pair, one query and one candidate at distance 5 in each: every pair is accepted, the
    histogram decides what stays.  Feature k of either side belongs to pair k"""
    n = len(pairs)
    act = 0 if kind == "tri" else 1
    s1 = side([Z] * n, nodes=np.arange(n) * 3 + 1, ang=[p[0] for p in pairs], active=act)
    s2 = side([bits(5)] * n, nodes=np.arange(n) * 3 + 1, ang=[p[1] for p in pairs], active=act)
    return mk(name, kind, None, None, expect, want, catches, check_ori=check_ori, s1=s1, s2=s2)


def rotation_cases():
    out = []
    H = lambda name, pairs, expect, want=None, catches=(), kind="bow_frame", **kw: out.append(  # noqa: E731
        _pairs_case(name, kind, pairs, expect, want, catches, **kw))
    hw = half_way_angles()
    by_bin = {}
    for a1, a2, b in hw:
        by_bin.setdefault(b, []).append((a1, a2))
    assert {1, 5, 9} <= set(by_bin)
    # three entries each in bins 1, 5, 9 through half-way angles, one each in bins 0 and 4: the single ones go.  Half-to-even
    # moves the nine into bins 0, 4, 8 and nothing is pruned
    pairs = [by_bin[b][k % len(by_bin[b])] for b in (1, 5, 9) for k in range(3)] + [(0.0, 0.0), (120.0, 0.0)]
    for kind in KINDS:
        H(f"{kind}_rot_half_way_decides_pruning", pairs, dict(hist_pruned=2, maxima_all_kept=1, accepted=11), list(range(9)) + [-1, -1],
          ("bin_half_to_even",), kind=kind)
    # -0.0f - 0.0f = -0.0f: not < 0, bin 0; with two more in bin 0 and one in bin 1
    H("rot_negative_zero_difference", [(-0.0, 0.0), (0.0, 0.0), (10.0, 10.0), (30.0, 0.0)], dict(hist_pruned=0, max3_below_tenth=1), [0, 1, 2, 3])
    # a tiny negative difference: rot + 360 rounds to 360.0f, bin 12 (not 0, not 30).  Bins 0, 1, 2 hold three each, bin 12
    # these two: pruned.  Without the wrap they would fall into bin 0
    a2 = nxt(100.0)
    assert f32(f32(f32(100.0) - a2) + f32(360.0)) == f32(360.0)
    for kind in KINDS:
        H(f"{kind}_rot_tiny_negative_becomes_360", [(100.0, a2)] * 2 + [(0.0, 0.0)] * 3 + [(30.0, 0.0)] * 3 + [(60.0, 0.0)] * 3,
          dict(hist_pruned=2, maxima_all_kept=1), [-1, -1] + list(range(2, 11)), ("bin_no_wrap",), kind=kind)
    # -30 is 330, bin 11, with two more there; bins 0 and 1 hold three each: nothing goes.  Unwrapped it is a bin of its own
    H("rot_negative_difference_wraps_to_330", [(0.0, 30.0)] + [(330.0, 0.0)] * 2 + [(0.0, 0.0)] * 3 + [(30.0, 0.0)] * 3,
      dict(hist_pruned=0, maxima_all_kept=1), list(range(9)), ("bin_no_wrap",))
    # just below and at a bin edge (15 degrees: 0.49999997 -> bin 0, 0.5 -> bin 1); bin 0: 1 + 2, bin 1: the one at the edge,
    # bins 2 and 3: three each -- the one at the edge goes
    b15 = nxt(15.0, False)            # (the float below 15 still multiplies to 0.5f: step down to the first that does not)
    while f32(b15 * f32(1.0 / HISTO_LENGTH)) >= f32(0.5):
        b15 = nxt(b15, False)
    assert 14.9999 < b15 < 15.0 and rot_bin(b15, 0.0) == 0 and rot_bin(nxt(b15), 0.0) == 1
    b15 = float(b15)
    H("rot_below_and_at_bin_edge", [(b15, 0.0), (15.0, 0.0)] + [(0.0, 0.0)] * 2 + [(60.0, 0.0)] * 3 + [(90.0, 0.0)] * 3,
      dict(hist_pruned=1, maxima_all_kept=1), [0, -1] + list(range(2, 10)), ("bin_half_to_even",))
    return out


def histogram_cases():
    out = []
    H = lambda name, pairs, expect, want=None, catches=(), kind="bow_frame", **kw: out.append(  # noqa: E731
        _pairs_case(name, kind, pairs, expect, want, catches, **kw))
    B = lambda b, n: [(30.0 * b, 0.0)] * n  # noqa: E731
    for kind in KINDS:
        # ties between bins: the first bin in index order keeps the higher place; of four equal bins the fourth goes
        H(f"{kind}_hist_tied_bins_first_index_wins", B(2, 2) + B(5, 2) + B(7, 2) + B(9, 2), dict(hist_pruned=2, maxima_all_kept=1),
          [0, 1, 2, 3, 4, 5, -1, -1], ("maxima_ge",), kind=kind)
        # max2 == 0.1f * max1 exactly is not below (strict <)
        H(f"{kind}_hist_tenth_10_1_1", B(0, 10) + B(1, 1) + B(2, 1), dict(maxima_all_kept=1, hist_pruned=0), list(range(12)), ("tenth_le",), kind=kind)
    H("hist_tenth_30_3_2", B(0, 30) + B(1, 3) + B(2, 2), dict(max3_below_tenth=1, hist_pruned=2), list(range(33)) + [-1, -1], ("tenth_le",))
    H("hist_tenth_11_1_0", B(0, 11) + B(1, 1), dict(max2_below_tenth=1, hist_pruned=1), list(range(11)) + [-1])
    # the stride-256 loop of the pruning kernel: arrays of 255 / 256 / 257 entries, all matched, entries 0, 254 and the last in
    # minor bins that are pruned
    for n in (255, 256, 257):
        pairs = B(0, n)
        w = list(range(n))
        for k, b in ((0, 3), (254, 4), (n - 1, 5)):
            pairs[k] = (30.0 * b, 0.0); w[k] = -1
        for kind in KINDS:
            H(f"{kind}_hist_{n}_matches", pairs, dict(accepted=n, hist_pruned=len(set((0, 254, n - 1))), max2_below_tenth=1), w, kind=kind)
    H("hist_check_ori_off", B(0, 20) + B(1, 1), dict(accepted=21, hist_pruned=0, max2_below_tenth=0, maxima_all_kept=0), list(range(21)),
      check_ori=False)
    for kind in KINDS:
        # zero matches: 0 < 0.1f * 0 is false twice, "all kept" of nothing
        out.append(mk(f"{kind}_hist_zero_matches", kind, [Z], [bits(120)], dict(accepted=0, maxima_all_kept=1), check_ori=True))
    return out


def named_cases():
    return threshold_cases() + ratio_cases() + reduction_cases() + claim_cases() + shape_cases() + tri_cases() + rotation_cases() + histogram_cases()


# ---- seeded cases: 200 small ones per search --------------------------------------------------------------------------
def _seeded_side(rng, n, protos, node_ids, kind, big):
    pr = rng.integers(0, len(protos), n)
    # a prototype with one of a few nested flip patterns: equal distances, near-threshold distances and ratio rejects all occur
    k = rng.choice(np.array([0, 0, 3, 3, 6, 10, 18, 25, 25, 32, 44, 60]), n)
    st = rng.choice(np.array([0, 0, 64, 128]), n)
    desc = np.stack([protos[p] ^ bits(int(kk), int(s)) for p, kk, s in zip(pr, k, st)]) if n else np.zeros((0, 32), np.uint8)
    # the node follows the prototype (as a vocabulary would), with a few strays
    nodes = np.where(rng.random(n) < 0.9, node_ids[pr % len(node_ids)], rng.choice(node_ids, n) if n else 0)
    x = (300.0 + rng.integers(-40, 41, n) * 0.5).astype(np.float32)
    y = (200.0 + rng.integers(-3, 4, n) * rng.choice(np.array([0.0, 0.5, 1.0, 4.0]), n)).astype(np.float32)
    return side(list(desc), nodes=nodes, has=(rng.random(n) < (0.35 if kind == "tri" else 0.8)).astype(np.uint8),
                ang=(rng.integers(0, 48, n) * 7.5).astype(np.float32) if not big else (rng.integers(0, 5, n) * 30.0).astype(np.float32),
                x=x, y=y, octave=rng.integers(0, 4, n), ur=np.where(rng.random(n) < 0.4, x - 3.0, -1.0))


def seeded_case(kind, seed):
    rng = np.random.default_rng([0xB0E, KINDS.index(kind), seed])
    big = seed % 20 == 7                                     # up to 400 a side in up to 3 nodes: 2 and 4 slots, the LDS path
    n_nodes = int(rng.integers(1, 4)) if big else int(rng.integers(1, 13))
    n1, n2 = (int(rng.integers(150, 401)), int(rng.integers(150, 401))) if big else (int(rng.integers(0, 90)), int(rng.integers(0, 90)))
    ids = np.sort(rng.choice(np.arange(1, 5000), n_nodes, replace=False)) * (1 if seed % 3 else 400000)
    protos = [bits(int(rng.integers(90, 140)), int(rng.integers(0, 256))) for _ in range(max(n_nodes, 2))]
    ids2 = ids.copy()
    if seed % 4 == 1 and n_nodes > 2:
        ids2[rng.integers(0, n_nodes)] += 1                  # a node the other side does not have
    s1 = _seeded_side(rng, n1, protos, ids, kind, big)
    s2 = _seeded_side(rng, n2, protos, ids2, kind, big)
    tri = {}
    if kind == "tri":
        # the line y = 200 (x1, y1 enter through F12's first two rows in a third of the seeds); the epipole sits inside the
        # cloud of key points in half of them
        F = np.array([0, 0, 0, 0, 0, 0, 0, 1, -200], np.float32)
        if seed % 3 == 0:
            F[[1, 4]] = [1e-3, -1.5e-3]
        e = (310.0, 201.0) if seed % 2 else (900.0, 700.0)
        tri = tri_args(F12=F, ex=e[0], ey=e[1], only_stereo=bool(seed % 5 == 0))
    return Case(f"seeded_{kind}_{seed}", kind, s1, s2, float(rng.choice([0.6, 0.75, 0.8])), bool(seed % 4 != 2), tri)


def seeded_cases(per_kind=200):
    return [seeded_case(k, s) for k in KINDS for s in range(per_kind)]


# ---- runners: one case through the restatement, the oracle, the device ----------------------------------------------
def run_restatement(c: Case, variant=None):
    if c.kind == "tri":
        t = c.tri
        (n, m), T = search_tri(c.s1, c.s2, t["F12"], t["ex"], t["ey"], t["sf2"], t["sig2"], t["only_stereo"], c.check_ori, variant)
    else:
        (n, m), T = search_bow(c.s1, c.s2, c.nnratio, c.check_ori, c.kind == "bow_kf", variant)
    return [int(n), [int(v) for v in m]], T


def _oracle_call(c: Case):
    import oracle_lib as orc
    a, b = c.s1, c.s2
    fv1, fv2 = orc.FeatVec(a["nodes"]), orc.FeatVec(b["nodes"])
    if c.kind == "bow_frame":
        return orc.search_by_bow(a["desc"], a["has"], a["ang"], fv1, b["desc"], b["ang"], fv2, c.nnratio, c.check_ori)
    if c.kind == "bow_kf":
        return orc.search_by_bow_kf(a["desc"], a["has"], a["ang"], fv1, b["desc"], b["has"], b["ang"], fv2, c.nnratio, c.check_ori)
    t = c.tri
    return orc.search_for_triangulation(a["desc"], a["has"], a["x"], a["y"], a["ang"], (a["ur"] >= 0).astype(np.uint8), fv1, b["desc"],
                                        b["has"], b["x"], b["y"], b["ang"], b["oct"], (b["ur"] >= 0).astype(np.uint8), fv2, t["F12"],
                                        float(t["ex"]), float(t["ey"]), t["sf2"], t["sig2"], t["only_stereo"], c.check_ori)


def run_oracle(c: Case):
    """the oracle's result and its counters: the BoW set plus the four histogram decisions of the window set"""
    import oracle_lib as orc
    n, m = _oracle_call(c)
    T = Counter(orc.bow_branch_counts())
    w = orc.window_branch_counts()
    assert all(v == 0 for k, v in w.items() if k not in HIST_BRANCHES), w
    T.update({k: w[k] for k in HIST_BRANCHES})
    return [int(n), m.tolist()], T


def _gpu_fv(amd, s):
    return amd.FeatureVector.from_node_of_feature(np.asarray(s["nodes"]).astype(np.uint32))


def gpu_resident(amd, s):
    v = amd.FrameView(s["x"], s["y"], s["oct"], s["desc"], VGA, angle=s["ang"], u_right=s["ur"])
    return v.upload(_gpu_fv(amd, s))


def multi_problems(c: Case):
    """the case as problem 1 of 3: problem 0 shares no node with the common side (all -1, count 0), problem 2 is the case
    with the varied side's descriptors rotated by one feature (and, for triangulation, another F12 and epipole).  The common
    side is the frame for (KF, Frame) -- SearchByBoWMulti -- and key frame 1 otherwise"""
    key = "s1" if c.kind == "bow_frame" else "s2"
    s = getattr(c, key)
    a = dict(s, nodes=s["nodes"] + 7000001)
    b = dict(s, desc=np.roll(s["desc"], 1, axis=0), has=np.roll(s["has"], 1))
    ca, cb = dataclasses.replace(c, **{key: a}), dataclasses.replace(c, **{key: b})
    if c.kind == "tri":
        F = np.asarray(c.tri["F12"], np.float32).copy()
        F[8] += f32(0.75)
        cb.tri = dict(c.tri, F12=F, ex=f32(c.tri["ex"]) - f32(3.0), ey=f32(c.tri["ey"]) + f32(1.0))
    return [ca, c, cb]


def run_gpu_multi(amd, cases):
    """K problems that share their common side (see multi_problems) in ONE SearchByBoWMulti / SearchByBoWKFMulti /
    SearchForTriangulationMulti call -> K results"""
    c = cases[0]
    m = amd.ORBmatcher(c.nnratio, c.check_ori)
    if c.kind == "bow_frame":
        common = gpu_resident(amd, c.s2)
        varied = [gpu_resident(amd, x.s1) for x in cases]
        cnt, got = m.SearchByBoWMulti(varied, [x.s1["has"] for x in cases], common)
    else:
        common = gpu_resident(amd, c.s1)
        varied = [gpu_resident(amd, x.s2) for x in cases]
        if c.kind == "bow_kf":
            cnt, got = m.SearchByBoWKFMulti(common, c.s1["has"], varied, [x.s2["has"] for x in cases])
        else:
            t = c.tri
            cnt, got = m.SearchForTriangulationMulti(common, c.s1["has"], varied, [x.s2["has"] for x in cases],
                                                     [x.tri["F12"] for x in cases], [(x.tri["ex"], x.tri["ey"]) for x in cases],
                                                     t["sf2"], t["sig2"], t["only_stereo"])
    out = [[int(cnt[k]), got[k].tolist()] for k in range(len(cases))]
    for r in varied + [common]:
        r.close()
    return out


def run_gpu(amd, c: Case, route):
    """route: "host" (arrays per call), "resident" (uploaded frames), "multi" (problem 1 of 3 of one multi call)"""
    if route == "multi":
        return run_gpu_multi(amd, multi_problems(c))[1]
    a, b = c.s1, c.s2
    m = amd.ORBmatcher(c.nnratio, c.check_ori)
    if route == "host":
        fv1, fv2 = _gpu_fv(amd, a), _gpu_fv(amd, b)
        if c.kind == "tri":
            t = c.tri
            n, pairs = m.SearchForTriangulation(a["desc"], a["has"], a["x"], a["y"], a["ang"], (a["ur"] >= 0).astype(np.uint8), fv1, b["desc"],
                                                b["has"], b["x"], b["y"], b["ang"], b["oct"], (b["ur"] >= 0).astype(np.uint8), fv2, t["F12"],
                                                float(t["ex"]), float(t["ey"]), t["sf2"], t["sig2"], t["only_stereo"])
            match = np.full(len(a["desc"]), -1, np.int64)
            if len(pairs):
                match[pairs[:, 0]] = pairs[:, 1]
            return [int(n), match.tolist()]
        n, got = m.SearchByBoW(a["desc"], a["has"], a["ang"], fv1, b["desc"], b["ang"], fv2, has_mp2=b["has"] if c.kind == "bow_kf" else None)
        return [int(n), got.tolist()]
    assert route == "resident", route
    if c.kind == "tri":                                     # the resident form of SearchForTriangulation is the multi call with K = 1
        return run_gpu_multi(amd, [c])[0]
    R1, R2 = gpu_resident(amd, a), gpu_resident(amd, b)
    n, got = m.SearchByBoWResident(R1, a["has"], R2, has_mp2=b["has"] if c.kind == "bow_kf" else None)
    R1.close()
    R2.close()
    return [int(n), got.tolist()]


# ---- the device-resident batch (k_search_by_bow_batch): frames placed in the nodes of a small vocabulary --------------------
BATCH_K = 10


def batch_vocabulary_arrays():
    """a two-level, 10-ary vocabulary whose level-1 centroids are rows 1..10 of the 256 x 256 Sylvester-Hadamard matrix
    (pairwise exactly 128 bits apart); the leaves are their parent with 4 bits flipped in the last byte pair, weight 1.
    A descriptor within 50 bits of centroid j is >= 78 bits from every other one: it lands in node j + 1"""
    i = np.arange(256)
    cent = np.stack([np.packbits(np.array([bin(int(r) & int(j)).count("1") & 1 for j in i], np.uint8), bitorder="little")
                     for r in range(1, BATCH_K + 1)])
    parent = np.concatenate([np.zeros(BATCH_K, np.int32), np.repeat(np.arange(1, BATCH_K + 1), BATCH_K).astype(np.int32)])
    leaf = np.concatenate([np.zeros(BATCH_K, np.uint8), np.ones(BATCH_K * BATCH_K, np.uint8)])
    kids = np.stack([cent[p] ^ bits(4, 200 + 5 * k) for p in range(BATCH_K) for k in range(BATCH_K)])
    weight = np.concatenate([np.zeros(BATCH_K), np.ones(BATCH_K * BATCH_K)])
    return (BATCH_K, 2, parent, leaf, np.concatenate([cent, kids]), weight), cent


def fits_batch(c: Case):
    """(KF, Frame) cases the batch form can hold: every key-frame feature has a map point, every descriptor is a pattern of
    at most 50 bits, at most 10 nodes, at most 320 features a side"""
    if c.kind != "bow_frame" or not c.s1["has"].all():
        return False
    pop = lambda d: int(_POP[d].sum(1).max()) if len(d) else 0  # noqa: E731
    ids = set(c.s1["nodes"].tolist()) | set(c.s2["nodes"].tolist())
    return pop(c.s1["desc"]) <= 50 and pop(c.s2["desc"]) <= 50 and len(ids) <= BATCH_K and max(len(c.s1["desc"]), len(c.s2["desc"])) <= 320


def batch_frames(c: Case, cent):
    """the two sides of a fitting case as frames of the batch: descriptor = centroid of the node's rank XOR the case's
    pattern -> [(descriptors, angles, intended level-1 node ids)] for side 1 and side 2"""
    ids = sorted(set(c.s1["nodes"].tolist()) | set(c.s2["nodes"].tolist()))
    out = []
    for s in (c.s1, c.s2):
        rank = np.array([ids.index(v) for v in s["nodes"].tolist()], np.int64)
        out.append((cent[rank] ^ s["desc"] if len(rank) else np.zeros((0, 32), np.uint8), s["ang"], (rank + 1).astype(np.uint32)))
    return out


def run_gpu_batch(voc, frames, capacity, nnratio, check_ori=True):
    """frames: [(descriptors, angles, ...)] -> (match[B - 1, capacity], n_matches[B - 1]) of SearchByBoW(frame t - 1, frame t)
    through bow_match_consecutive_batch_device, and the device FeatureVectors (nodes, offsets, indices, count) of the frames.
    The operands are torch tensors written here: no extractor takes part"""
    import torch
    dev = torch.device("cuda", 0)
    B = len(frames)
    kp = np.zeros((B, capacity, 7), np.float32)
    desc = np.zeros((B, capacity, 32), np.uint8)
    n = np.zeros(B, np.int32)
    for t, fr in enumerate(frames):
        k = len(fr[0])
        n[t] = k
        desc[t, :k] = fr[0]
        kp[t, :k, 3] = fr[1]
    d_kp, d_desc, d_n = torch.from_numpy(kp).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(n).to(dev)
    d_match = torch.zeros((B - 1, capacity), dtype=torch.int32, device=dev)
    d_nm = torch.zeros((B - 1,), dtype=torch.int32, device=dev)
    d_nodes = torch.zeros((B, capacity), dtype=torch.int32, device=dev)
    d_off = torch.zeros((B, capacity + 1), dtype=torch.int32, device=dev)
    d_idx = torch.zeros((B, capacity), dtype=torch.int32, device=dev)
    d_cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    voc.featvec_batch_device(d_desc.data_ptr(), d_n.data_ptr(), B, capacity, d_nodes.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(),
                             d_cnt.data_ptr(), levelsup=1)
    voc.bow_match_consecutive_batch_device(B, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), capacity, d_match.data_ptr(),
                                           d_nm.data_ptr(), nnratio=nnratio, check_orientation=check_ori, levelsup=1)
    torch.cuda.synchronize()
    fv = (d_nodes.cpu().numpy(), d_off.cpu().numpy(), d_idx.cpu().numpy(), d_cnt.cpu().numpy())
    return d_match.cpu().numpy(), d_nm.cpu().numpy(), fv
