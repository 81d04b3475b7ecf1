"""Engineered edge cases for the Frame grid and the window searches built on it, and an independent plain-Python
restatement of those searches.  No GPU here: tests/test_window_edges.py pins the oracle (oracle/orb_oracle.c) to the
restatement on every case and shows that each case takes the branch it names; tests/test_gpu_window_edges.py runs the
same cases through the kernels of csrc/k_window.hip.

Restated from the reference, float steps in np.float32, double exactly where the reference promotes:

    Frame::AssignFeaturesToGrid / PosInGrid            src/Frame.cc:246-267, 417-427
    Frame::GetFeaturesInArea                           src/Frame.cc:358-415
    SearchByProjection(Frame, map points)              src/ORBmatcher.cc:51-138, RadiusByViewingCos :146-152
    SearchByProjection(KeyFrame, Scw, ...)   (Sim3)    src/ORBmatcher.cc:335-449 (after the projection, :407-448)
    SearchForInitialization                            src/ORBmatcher.cc:469-600
    Fuse, with and without the chi-square gate         src/ORBmatcher.cc:940-1110 (:1006-1075), :1112-1249 (:1184-1222)
    SearchBySim3                                       src/ORBmatcher.cc:1251-1482 (:1340-1375, :1420-1455, :1460-1475)
    SearchByProjection(CurrentFrame, LastFrame)        src/ORBmatcher.cc:1484-1630 (:1541-1627)
    SearchByProjection(CurrentFrame, KeyFrame, ...)    src/ORBmatcher.cc:1641-1770 (:1697-1767)
    ComputeThreeMaxima                                 src/ORBmatcher.cc:1777-1821

Every restatement takes the operands the orc_* functions take (the state after the caller's projection) and a tally that
counts the same exits as orc_window_branch_counts, under the names of oracle_lib.WINDOW_BRANCHES.

A branch that cannot be reached: none of the counters.  One case of the list the cases were written from cannot exist:
"a feature whose rounding cell lies outside the floor/ceil cell range of a window that geometrically contains it" -- for a
feature inside the grid, with fx*w <= (x+r)*w (float multiplication is monotone) round(fx*w) = floor(fx*w + .5) <=
ceil(fx*w) <= ceil((x+r)*w), and round(fx*w) >= floor(fx*w) >= floor((x-r)*w): the rounding cell is always inside the
range.  What does exist is a feature the window contains whose rounding cell lies outside the GRID (63.5 -> column 64, -0.5
-> column -1): it is in no cell and no window returns it.  `grid_rounding` holds those, and test_window_edges.py asserts
the inequality above on every (feature, window) pair of the case set.
"""
from __future__ import annotations

import math
from collections import Counter
from dataclasses import dataclass, field

import numpy as np

f32 = np.float32
TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30
INT_MAX = 2 ** 31 - 1
SF = (1.2 ** np.arange(8)).astype(np.float32)
INV_SIGMA2 = (1.0 / (SF * SF)).astype(np.float32)
UNIT = (0.0, 64.0, 0.0, 48.0)           # wInv = hInv = 1 exactly: cells are integer pixels
VGA = (0.0, 640.0, 0.0, 480.0)          # wInv = 0.1f, inexact
OFFSET = (-12.5, 655.25, -8.0, 490.5)   # non-zero minima
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def c_round(v):  # C round(): half away from zero
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


# ---- Frame grid (src/Frame.cc:246-267, 417-427) and GetFeaturesInArea (:358-415) ------------------------------------
def py_grid(x, y, bounds):
    minx, maxx, miny, maxy = bounds
    winv = f32(64.0) / (f32(maxx) - f32(minx))      # src/Frame.cc:109-110
    hinv = f32(48.0) / (f32(maxy) - f32(miny))
    grid = [[[] for _ in range(48)] for _ in range(64)]
    for i in range(len(x)):
        px = c_round(float((f32(x[i]) - f32(minx)) * winv))    # :422-423
        py = c_round(float((f32(y[i]) - f32(miny)) * hinv))
        if 0 <= px < 64 and 0 <= py < 48:                      # :426-427
            grid[px][py].append(i)
    return grid, winv, hinv


def py_area(grid, winv, hinv, X, Y, octv, bounds, x, y, r, lo, hi, tally=None):
    T = tally if tally is not None else Counter()
    minx, _, miny, _ = [f32(b) for b in bounds]
    x, y, r = f32(x), f32(y), f32(r)
    out = []
    a = int(math.floor(float((x - minx - r) * winv)))          # :365
    if a < 0:
        a = 0; T["clamp_minx"] += 1
    if a >= 64:
        T["empty_minx_past"] += 1
        return out
    b = int(math.ceil(float((x - minx + r) * winv)))           # :369
    if b > 63:
        b = 63; T["clamp_maxx"] += 1
    if b < 0:
        T["empty_maxx_neg"] += 1
        return out
    c = int(math.floor(float((y - miny - r) * hinv)))          # :373
    if c < 0:
        c = 0; T["clamp_miny"] += 1
    if c >= 48:
        T["empty_miny_past"] += 1
        return out
    d = int(math.ceil(float((y - miny + r) * hinv)))           # :377
    if d > 47:
        d = 47; T["clamp_maxy"] += 1
    if d < 0:
        T["empty_maxy_neg"] += 1
        return out
    chk = lo > 0 or hi >= 0                                    # :382
    for ix in range(a, b + 1):
        for iy in range(c, d + 1):
            for i in grid[ix][iy]:
                if chk:
                    if octv[i] < lo:
                        T["level_reject_low"] += 1
                        continue
                    if hi >= 0 and octv[i] > hi:
                        T["level_reject_high"] += 1
                        continue
                if abs(f32(X[i]) - x) < r and abs(f32(Y[i]) - y) < r:   # :405-409
                    out.append(i); T["area_accept"] += 1
                else:
                    T["radius_reject"] += 1
    return out


class RFrame:
    """what the restatements read of a Frame / KeyFrame"""

    def __init__(self, x, y, octave, desc, bounds, angle=None, u_right=None):
        self.x, self.y = np.asarray(x, np.float32), np.asarray(y, np.float32)
        self.octave = np.asarray(octave, np.int32)
        self.desc = np.asarray(desc, np.uint8).reshape(-1, 32)
        self.angle = np.zeros(len(self.x), np.float32) if angle is None else np.asarray(angle, np.float32)
        self.ur = None if u_right is None else np.asarray(u_right, np.float32)
        self.bounds = tuple(bounds)
        self.N = len(self.x)
        self.grid, self.winv, self.hinv = py_grid(self.x, self.y, bounds)

    def area(self, x, y, r, lo, hi, T):
        return py_area(self.grid, self.winv, self.hinv, self.x, self.y, self.octave, self.bounds, x, y, r, lo, hi, T)


def three_maxima(sizes, T):
    """src/ORBmatcher.cc:1777-1821"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1, i3, i2, i1 = max2, max1, s, i2, i1, i
        elif s > max2:
            max3, max2, i3, i2 = max2, s, i2, i
        elif s > max3:
            max3, i3 = s, i
    tenth = f32(0.1) * f32(max1)                               # :1812 0.1f*(float)max1, int promoted to float
    if f32(max2) < tenth:
        i2 = i3 = -1; T["max2_below_tenth"] += 1
    elif f32(max3) < tenth:                                    # :1817
        i3 = -1; T["max3_below_tenth"] += 1
    else:
        T["maxima_all_kept"] += 1
    return i1, i2, i3


def rot_bin(a1, a2):
    """:1593-1598 (the same five lines in every search with a histogram)"""
    rot = f32(a1) - f32(a2)
    if float(rot) < 0.0:
        rot = f32(rot + f32(360.0))
    b = c_round(float(f32(rot * f32(1.0 / HISTO_LENGTH))))
    return 0 if b == HISTO_LENGTH else b


def _prune(hist, arr, T):
    """:1608-1627 / :1748-1767 -- every entry of a dropped bin is cleared and counted"""
    removed = 0
    keep = three_maxima([len(h) for h in hist], T)
    for b in range(HISTO_LENGTH):
        if b in keep:
            continue
        for j in hist[b]:
            arr[j] = -1; removed += 1; T["hist_pruned"] += 1
    return removed


def _stereo_ok(F, idx, ur_q, radius, T):
    """:100-105, :1567-1573 -- True: candidate stays"""
    if F.ur is None:
        return True
    if f32(F.ur[idx]) > 0:
        er = abs(f32(f32(ur_q) - f32(F.ur[idx])))
        if er > radius:
            T["stereo_reject"] += 1
            return False
        T["stereo_pass"] += 1
    else:
        T["stereo_skipped"] += 1
    return True


def search_mappoints(F, sf, blocked0, in_view, level, view_cos, px, py, pxr, md, obs, th, nnratio):
    """src/ORBmatcher.cc:51-138"""
    T = Counter()
    nm, match = 0, [-1] * F.N
    blocked = [False] * F.N if blocked0 is None else [bool(b) for b in blocked0]
    b_factor = float(f32(th)) != 1.0                                       # :55
    for i in range(len(in_view)):
        if not in_view[i]:
            continue
        lv = int(level[i])
        r = f32(2.5) if float(f32(view_cos[i])) > 0.998 else f32(4.0)      # :148 (double compare)
        if b_factor:
            r = f32(r * f32(th))                                           # :73-74
        radius = f32(r * f32(sf[lv]))
        cand = F.area(px[i], py[i], radius, lv - 1, lv, T)                 # :77
        if not cand:
            continue
        best, best2, lev, lev2, bi = 256, 256, -1, -1, -1
        for idx in cand:
            if blocked[idx]:                                               # :95-98
                T["blocked"] += 1
                continue
            if not _stereo_ok(F, idx, pxr[i] if pxr is not None else 0, radius, T):
                continue
            d = hamming(md[i], F.desc[idx])
            if d < best:                                                   # :111-118
                best2, best, lev2, lev, bi = best, d, lev, int(F.octave[idx]), idx
                T["better_best"] += 1
            else:
                if d == best:
                    T["tie_ignored"] += 1
                if d < best2:                                              # :119-123
                    lev2, best2 = int(F.octave[idx]), d
                    T["better_second"] += 1
        if best <= TH_HIGH:                                                # :127
            over = f32(best) > f32(nnratio) * f32(best2)                   # :129 int > float * int: in float
            if lev == lev2 and over:
                T["ratio_reject"] += 1
                continue
            if over:
                T["ratio_pass_levels_differ"] += 1
            match[bi] = i
            blocked[bi] = True if obs is None else bool(obs[i])            # Observations() > 0 of the new point
            nm += 1; T["accepted"] += 1
        elif bi < 0:
            T["no_candidate"] += 1
        else:
            T["threshold_reject"] += 1
    return (nm, match), T


def _best_claim(F, cand, blocked, desc_q, T, stereo=None):
    best, bi = 256, -1
    for i2 in cand:
        if blocked[i2]:
            T["blocked"] += 1
            continue
        if stereo is not None and not _stereo_ok(F, i2, stereo[0], stereo[1], T):
            continue
        d = hamming(desc_q, F.desc[i2])
        if d < best:
            best, bi = d, i2; T["better_best"] += 1
        elif d == best:
            T["tie_ignored"] += 1
    return best, bi


def _after_best(best, bi, th, T):
    if best <= th:
        T["accepted"] += 1
        return True
    T["no_candidate" if bi < 0 else "threshold_reject"] += 1
    return False


def search_lastframe(Cur, sf, mbf, valid, u, v, invzc, last_octave, last_angle, md, obs, blocked0, mode, th, check_ori):
    """src/ORBmatcher.cc:1541-1627"""
    T = Counter()
    nm, match = 0, [-1] * Cur.N
    blocked = [False] * Cur.N if blocked0 is None else [bool(b) for b in blocked0]
    hist = [[] for _ in range(HISTO_LENGTH)]
    for i in range(len(valid)):
        if not valid[i]:
            continue
        o = int(last_octave[i])
        radius = f32(f32(th) * f32(sf[o]))                                 # :1541
        lo, hi = ((o, -1) if mode == 1 else (0, o) if mode == 2 else (o - 1, o + 1))    # :1545-1550
        cand = Cur.area(u[i], v[i], radius, lo, hi, T)
        if not cand:
            continue
        ur = 0
        if Cur.ur is not None:
            ur = f32(f32(u[i]) - f32(f32(mbf) * f32(invzc[i])))            # :1569 multiply, then subtract
        best, bi = _best_claim(Cur, cand, blocked, md[i], T, (ur, radius))
        if _after_best(best, bi, TH_HIGH, T):                              # :1586
            match[bi] = i
            blocked[bi] = True if obs is None else bool(obs[i])
            nm += 1
            if check_ori:
                hist[rot_bin(last_angle[i], Cur.angle[bi])].append(bi)
    if check_ori:
        nm -= _prune(hist, match, T)
    return (nm, match), T


def search_reloc(Cur, sf, valid, u, v, level, kf_angle, md, blocked0, th, orb_dist, check_ori):
    """src/ORBmatcher.cc:1697-1767"""
    T = Counter()
    nm, match = 0, [-1] * Cur.N
    blocked = [False] * Cur.N if blocked0 is None else [bool(b) for b in blocked0]
    hist = [[] for _ in range(HISTO_LENGTH)]
    for i in range(len(valid)):
        if not valid[i]:
            continue
        lv = int(level[i])
        radius = f32(f32(th) * f32(sf[lv]))                                # :1697
        cand = Cur.area(u[i], v[i], radius, lv - 1, lv + 1, T)             # :1699
        if not cand:
            continue
        best, bi = _best_claim(Cur, cand, blocked, md[i], T)
        if _after_best(best, bi, orb_dist, T):                             # :1726
            match[bi] = i
            blocked[bi] = True
            nm += 1
            if check_ori:
                hist[rot_bin(kf_angle[i], Cur.angle[bi])].append(bi)
    if check_ori:
        nm -= _prune(hist, match, T)
    return (nm, match), T


def _best_in_levels(KF, cand, lv, desc_q, T, init, blocked=None, gate=None):
    """the inner loop Sim3 projection (:420-440), Fuse (:1013-1067, :1191-1214) and SearchBySim3 (:1349-1370) share"""
    best, bi = init, -1
    for idx in cand:
        if blocked is not None and blocked[idx]:                           # :423
            T["blocked"] += 1
            continue
        kl = int(KF.octave[idx])
        if kl < lv - 1:                                                    # :428
            T["level_reject_low"] += 1
            continue
        if kl > lv:
            T["level_reject_high"] += 1
            continue
        if gate is not None and not gate(idx, kl):
            continue
        d = hamming(desc_q, KF.desc[idx])
        if d < best:
            best, bi = d, idx; T["better_best"] += 1
        elif d == best:
            T["tie_ignored"] += 1
    return best, bi


def search_sim3proj(KF, sf, valid, u, v, level, md, matched0, th):
    """src/ORBmatcher.cc:407-448"""
    T = Counter()
    nm, match = 0, [-1] * KF.N
    matched = [False] * KF.N if matched0 is None else [bool(b) for b in matched0]
    for i in range(len(valid)):
        if not valid[i]:
            continue
        lv = int(level[i])
        radius = f32(f32(th) * f32(sf[lv]))                                # :408
        cand = KF.area(u[i], v[i], radius, -1, -1, T)                      # :410
        if not cand:
            continue
        best, bi = _best_in_levels(KF, cand, lv, md[i], T, 256, matched)
        if _after_best(best, bi, TH_LOW, T):                               # :442
            match[bi] = i; matched[bi] = True; nm += 1
    return (nm, match), T


def search_init(F1, F2, prev, window, nnratio, check_ori):
    """src/ORBmatcher.cc:469-600"""
    T = Counter()
    nm = 0
    m12, m21, mdist = [-1] * F1.N, [-1] * F2.N, [INT_MAX] * F2.N
    prev = np.array(prev, np.float32).copy()
    hist = [[] for _ in range(HISTO_LENGTH)]
    for i1 in range(F1.N):
        l1 = int(F1.octave[i1])
        if l1 > 0:                                                         # :488
            continue
        cand = F2.area(prev[i1, 0], prev[i1, 1], f32(window), l1, l1, T)   # :494
        if not cand:
            continue
        best, best2, bi = INT_MAX, INT_MAX, -1
        for i2 in cand:
            d = hamming(F1.desc[i1], F2.desc[i2])
            if mdist[i2] <= d:                                             # :515
                T["init_refused"] += 1
                continue
            if d < best:
                best2, best, bi = best, d, i2; T["better_best"] += 1
            else:
                if d == best:
                    T["tie_ignored"] += 1
                if d < best2:
                    best2 = d; T["better_second"] += 1
        if best <= TH_LOW:                                                 # :532
            if f32(best) < f32(f32(best2) * f32(nnratio)):                 # :534
                if m21[bi] >= 0:                                           # :536-541
                    m12[m21[bi]] = -1; nm -= 1; T["init_overwrite"] += 1
                m12[i1], m21[bi], mdist[bi] = bi, i1, best
                nm += 1; T["accepted"] += 1
                if check_ori:
                    hist[rot_bin(F1.angle[i1], F2.angle[bi])].append(i1)   # :551-558
            else:
                T["ratio_reject"] += 1
        elif bi < 0:
            T["no_candidate"] += 1
        else:
            T["threshold_reject"] += 1
    if check_ori:                                                          # :567-591
        keep = three_maxima([len(h) for h in hist], T)
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for idx1 in hist[b]:
                if m12[idx1] >= 0:
                    m12[idx1] = -1; nm -= 1; T["hist_pruned"] += 1
                else:
                    T["hist_prune_already_unmatched"] += 1
    for i1 in range(F1.N):                                                 # :595-597
        if m12[i1] >= 0:
            prev[i1, 0], prev[i1, 1] = F2.x[m12[i1]], F2.y[m12[i1]]
    return (nm, m12, prev), T


def search_fuse(KF, sf, inv_sigma2, valid, u, v, ur, level, md, th, chi2):
    """src/ORBmatcher.cc:1006-1075 (chi2) and :1184-1222 (the Sim3 overload, no gate)"""
    T = Counter()
    out = [-1] * len(valid)
    for i in range(len(valid)):
        if not valid[i]:
            continue
        lv = int(level[i])
        radius = f32(f32(th) * f32(sf[lv]))                                # :1006
        cand = KF.area(u[i], v[i], radius, -1, -1, T)                      # :1008

        def gate(idx, kl, i=i):
            ex, ey = f32(f32(u[i]) - KF.x[idx]), f32(f32(v[i]) - KF.y[idx])
            if KF.ur is not None and f32(KF.ur[idx]) >= 0:                 # :1030
                er = f32(f32(ur[i]) - KF.ur[idx])
                e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))  # :1039
                if float(f32(e2 * f32(inv_sigma2[kl]))) > 7.8:             # :1041 float product, double compare
                    T["chi2_stereo_reject"] += 1
                    return False
                T["chi2_stereo_pass"] += 1
            else:
                e2 = f32(f32(ex * ex) + f32(ey * ey))                      # :1050
                if float(f32(e2 * f32(inv_sigma2[kl]))) > 5.99:            # :1052
                    T["chi2_mono_reject"] += 1
                    return False
                T["chi2_mono_pass"] += 1
            return True
        best, bi = _best_in_levels(KF, cand, lv, md[i], T, 256, None, gate if chi2 else None)
        if _after_best(best, bi, TH_LOW, T):                               # :1070
            out[i] = bi
    return (out,), T


def search_sim3(KF1, KF2, sf1, sf2, valid1, u1, v1, level1, desc1, valid2, u2, v2, level2, desc2, th):
    """src/ORBmatcher.cc:1340-1375, :1420-1455, the agreement check :1460-1475"""
    T = Counter()

    def one_way(KF, sf, valid, u, v, level, desc):
        out = [-1] * len(valid)
        for i in range(len(valid)):
            if not valid[i]:
                continue
            lv = int(level[i])
            radius = f32(f32(th) * f32(sf[lv]))
            cand = KF.area(u[i], v[i], radius, -1, -1, T)
            best, bi = _best_in_levels(KF, cand, lv, desc[i], T, INT_MAX)
            if _after_best(best, bi, TH_HIGH, T):
                out[i] = bi
        return out
    m1 = one_way(KF2, sf2, valid1, u1, v1, level1, desc1)
    m2 = one_way(KF1, sf1, valid2, u2, v2, level2, desc2)
    m12, n = [-1] * KF1.N, 0
    for i1 in range(KF1.N):
        if m1[i1] >= 0 and m2[m1[i1]] == i1:
            m12[i1] = m1[i1]; n += 1; T["sim3_mutual"] += 1
        elif m1[i1] >= 0:
            T["sim3_one_way_only"] += 1
    return (n, m12), T


# ---- cases ----------------------------------------------------------------------------------------------------------
def bits(k, start=0):
    """a descriptor at Hamming distance k from the zero descriptor; different `start`s give different descriptors"""
    d = np.zeros(32, np.uint8)
    for b in range(start, start + k):
        b %= 256
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def nxt(v, up=True):
    return np.nextafter(f32(v), f32(np.inf if up else -np.inf))


@dataclass
class Case:
    name: str
    kind: str                      # area | mappoints | lastframe | reloc | sim3proj | init | fuse | sim3
    frame: dict                    # x, y, octave, desc, bounds, angle, u_right  (the searched frame)
    args: dict
    expect: dict = field(default_factory=dict)    # branch -> exact count the oracle must report
    want: object = None            # outcome spelled out (compared with the oracle's first result array)
    frame1: dict | None = None     # init: F1; sim3: KF1 (frame is F2 / KF2)


def mk_frame(pts, bounds, ur=None):
    """pts: (x, y, octave, angle, descriptor)"""
    return dict(x=np.array([p[0] for p in pts], np.float32), y=np.array([p[1] for p in pts], np.float32),
                octave=np.array([p[2] for p in pts], np.int32), angle=np.array([p[3] for p in pts], np.float32),
                desc=np.stack([p[4] for p in pts]) if pts else np.zeros((0, 32), np.uint8), bounds=bounds,
                u_right=None if ur is None else np.array(ur, np.float32))


def pad_frame(fr, form):
    """The same features in the three grid forms of the device: 'sparse' (as built, k_grid_build_count's counting
    path), 'crowded' (70 more in one cell: its bitonic fallback), 'large' (n > 8192: k_grid_build).  The filler is
    appended -- indices of the case's own features do not move -- and sits in grid cell (50, 40) at octave 7, outside
    every window of the named cases (the CPU test asserts that no result changes)."""
    if form == "sparse":
        return fr
    k = 70 if form == "crowded" else 8200
    minx, maxx, miny, maxy = fr["bounds"]
    cx = f32(minx + (maxx - minx) * 50.0 / 64.0)
    cy = f32(miny + (maxy - miny) * 40.0 / 48.0)
    out = dict(fr)
    out["x"] = np.concatenate([fr["x"], np.full(k, cx, np.float32)])
    out["y"] = np.concatenate([fr["y"], np.full(k, cy, np.float32)])
    out["octave"] = np.concatenate([fr["octave"], np.full(k, 7, np.int32)])
    out["angle"] = np.concatenate([fr["angle"], np.zeros(k, np.float32)])
    out["desc"] = np.concatenate([fr["desc"], np.repeat(bits(200)[None], k, 0)])
    if fr["u_right"] is not None:
        out["u_right"] = np.concatenate([fr["u_right"], np.full(k, -1, np.float32)])
    return out


def padded_case(c, form):
    """the case on pad_frame(frame, form); SearchBySim3's per-feature arrays of the padded frame grow with it (invalid)"""
    import dataclasses
    fr = pad_frame(c.frame, form)
    k = len(fr["x"]) - len(c.frame["x"])
    args = c.args
    if c.kind == "sim3" and k:
        args = dict(args)
        for key in ("valid2", "u2", "v2", "level2"):
            args[key] = np.concatenate([args[key], np.zeros(k, args[key].dtype)])
        args["desc2"] = np.concatenate([args["desc2"], np.zeros((k, 32), np.uint8)])
    return dataclasses.replace(c, frame=fr, args=args)


def _scale(bounds, x, y):
    """a position given in cells of the UNIT grid -> the same cell position under `bounds` (exact for UNIT)"""
    minx, maxx, miny, maxy = bounds
    return f32(minx + x * (maxx - minx) / 64.0), f32(miny + y * (maxy - miny) / 48.0)


Z = np.zeros(32, np.uint8)


def area_cases():
    out = []
    pts = [(10.5, 10.5, 0), (-0.5, 5.0, 0), (-0.49, 5.0, 0), (63.5, 5.0, 0), (5.0, 47.5, 0), (0.0, 20.0, 1), (64.0, 20.0, 1),
           (-0.0, 21.0, 1), (20.0, 20.0, 0), (23.0, 20.0, 2), (20.0, 23.0, 3), (11.5, 10.5, 1), (30.0, 5.0, 0), (30.0, 6.0, 1),
           (30.0, 7.0, 2), (30.0, 8.0, 3), (63.49, 30.0, 0), (5.0, 47.49, 0), (2.5, 2.5, 0), (3.5, 2.5, 0), (-1.5, 2.0, 0)]
    fr = mk_frame([(x, y, o, 0.0, Z) for x, y, o in pts], UNIT)
    A = lambda name, q, expect, want=None: out.append(Case(name, "area", fr, dict(q=q), expect, want))  # noqa: E731
    # the grid itself: 10.5 -> 11 (half away from zero), -0.5 -> -1 dropped, -0.49 -> 0, 63.5 / 47.5 / maxX -> dropped
    # (two windows that together contain every feature and leave out grid cell (50, 40), where pad_frame() puts its filler)
    A("grid_rounding", [(20.0, 24.0, f32(26.0), -1, -1), (60.0, 10.0, f32(24.0), -1, -1)],
      dict(clamp_minx=1, clamp_maxx=1, clamp_miny=2, clamp_maxy=1),
      [[2, 5, 7, 18, 19, 17, 0, 11, 8, 10, 9, 12, 13, 14, 15], [16]])
    A("half_cell_column", [(11.0, 10.5, f32(0.75), -1, -1), (10.0, 10.5, f32(0.75), -1, -1)], dict(area_accept=3),
      [[0, 11], [0]])
    A("integer_window_edges", [(21.0, 21.0, f32(2.0), -1, -1)], dict(radius_reject=2, area_accept=1), [[8]])
    A("empty_right_left_below_above", [(70.0, 10.0, f32(5.0), -1, -1), (-7.0, 10.0, f32(5.0), -1, -1),
                                       (10.0, 54.0, f32(5.0), -1, -1), (10.0, -7.0, f32(5.0), -1, -1)],
      dict(empty_minx_past=1, empty_maxx_neg=1, empty_miny_past=1, empty_maxy_neg=1), [[], [], [], []])
    # x - r == 64 exactly: floor(64) = 64 >= 64 returns; x + r == -1: ceil(-1) < 0 returns; x + r == -0.5: ceil = -0 -> kept
    A("empty_exactly_at_the_edge", [(69.0, 10.0, f32(5.0), -1, -1), (-6.0, 10.0, f32(5.0), -1, -1),
                                    (-5.5, 2.0, f32(5.0), -1, -1)],
      dict(empty_minx_past=1, empty_maxx_neg=1, clamp_minx=2))
    A("clamped_each_side", [(1.0, 20.0, f32(3.0), -1, -1), (62.0, 30.0, f32(3.0), -1, -1), (2.5, 1.0, f32(3.0), -1, -1),
                            (5.0, 46.0, f32(3.0), -1, -1)], dict(clamp_minx=2, clamp_maxx=1, clamp_miny=1, clamp_maxy=1),
      [[5, 7], [16], [18, 19], [17]])
    A("dx_equals_r", [(20.0, 20.0, f32(3.0), -1, -1), (20.0, 20.0, nxt(3.0), -1, -1), (20.0, 20.0, nxt(3.0, False), -1, -1)],
      dict(area_accept=5), [[8], [8, 10, 9], [8]])
    lv = [(-1, -1), (0, -1), (2, -1), (0, 3), (1, 2), (3, 1)]
    A("level_sign_combinations", [(30.0, 6.5, f32(4.0), lo, hi) for lo, hi in lv],
      dict(level_reject_low=2 + 1 + 3, level_reject_high=1 + 1), [[12, 13, 14, 15], [12, 13, 14, 15], [14, 15], [12, 13, 14, 15],
                                                                  [13, 14], []])
    A("negative_zero_and_min_edge", [(0.0, 20.5, f32(1.0), -1, -1), (-0.0, 20.5, f32(1.0), -1, -1)], dict(clamp_minx=2),
      [[5, 7], [5, 7]])
    # the same constructions under the two inexact bounds (cells of 10 px / 10.43 px; positions scaled cell for cell)
    for tag, bounds in (("vga", VGA), ("offset", OFFSET)):
        sp = [(*_scale(bounds, x, y), o, 0.0, Z) for x, y, o in pts]
        fr2 = mk_frame(sp, bounds)
        qs = []
        for (x, y, r) in [(20, 24, 26), (60, 10, 24), (11, 10.5, 0.75), (21, 21, 2), (70, 10, 5), (-7, 10, 5), (10, 54, 5), (10, -7, 5),
                          (1, 20, 3), (62, 30, 3), (2.5, 1, 3), (5, 46, 3), (20, 20, 3), (30, 6.5, 4)]:
            sx, sy = _scale(bounds, x, y)
            rr = f32(r * (bounds[1] - bounds[0]) / 64.0)
            qs += [(sx, sy, rr, -1, -1), (sx, sy, nxt(rr), 1, 2)]
        # |dx| == r with the scaled coordinates: r taken as the float difference itself, and one float above
        d = abs(f32(sp[9][0]) - f32(sp[8][0]))
        qs += [(sp[8][0], sp[8][1], d, -1, -1), (sp[8][0], sp[8][1], nxt(d), -1, -1)]
        out.append(Case(f"grid_edges_{tag}", "area", fr2, dict(q=qs),
                        dict(empty_minx_past=2, empty_maxx_neg=2, empty_miny_past=2, empty_maxy_neg=2)))
    return out


def _q(n, **kw):
    """query-side arrays of n points with defaults"""
    d = dict(valid=np.ones(n, np.uint8), level=np.zeros(n, np.int32), angle=np.zeros(n, np.float32),
             desc=np.zeros((n, 32), np.uint8))
    d.update(kw)
    return d


def best_cases():
    """best-of-window decisions through the key-frame (relocalisation) form: CLAIM_BEST with a caller threshold"""
    out = []
    R = lambda name, pts, u, v, expect, want=None, **kw: out.append(Case(  # noqa: E731
        name, "reloc", mk_frame(pts, UNIT), dict(u=np.array(u, np.float32), v=np.array(v, np.float32),
                                                 **{**_q(len(u)), **dict(th=3.0, orb_dist=100, check_ori=False, blocked=None), **kw}),
        expect, want))
    for th_name, th in (("th_low", TH_LOW), ("th_high", TH_HIGH), ("orbdist_64", 64)):
        pts = [(10.0, 10.0, 0, 0.0, bits(th)), (30.0, 10.0, 0, 0.0, bits(th + 1))]
        R(f"distance_at_{th_name}_and_one_above", pts, [10.0, 30.0], [10.0, 10.0], dict(accepted=1, threshold_reject=1),
          [0, 1 - 2], orb_dist=th)
    pts = [(10.0, 10.0, 0, 0.0, bits(5)), (11.0, 10.0, 0, 0.0, bits(6))]
    R("every_candidate_blocked", pts, [10.5], [10.0], dict(blocked=2, no_candidate=1), [-1, -1], blocked=np.ones(2, np.uint8))
    # equal minima: the LATER index sits in the lower grid column and is scanned first
    pts = [(12.0, 10.0, 0, 0.0, bits(7, 0)), (9.0, 10.0, 0, 0.0, bits(7, 8))]
    R("two_equal_minima_scan_order", pts, [10.5], [10.0], dict(tie_ignored=1, accepted=1), [-1, 0])
    pts = [(12.0, 10.0, 0, 0.0, bits(7, 0)), (10.0, 11.0, 0, 0.0, bits(7, 16)), (9.0, 12.0, 0, 0.0, bits(7, 8))]
    R("three_equal_minima_scan_order", pts, [10.5], [10.5], dict(tie_ignored=2, accepted=1), [-1, -1, 0])
    pts = [(10.2, 10.0, 0, 0.0, bits(7, 0)), (10.1, 10.0, 0, 0.0, bits(7, 8))]
    R("two_equal_minima_same_cell_index_order", pts, [10.0], [10.0], dict(tie_ignored=1, accepted=1), [0, -1])
    # list lengths 7, 8, 9, 16, 17, 32 (the host's initial capacity) and 33 (regrowth), the minimum at several positions;
    # candidates in one grid row, one per column from column 5: scan order == index order
    for n in (7, 8, 9, 16, 17, 32, 33):
        for pos in sorted({0, 7, 8, n - 1}):
            if pos >= n:
                continue
            pts = [(5.0 + k, 10.0, 0, 0.0, bits(20 if k != pos else 9, k)) for k in range(n)]
            w = [-1] * n
            w[pos] = 0
            R(f"list_of_{n}_min_at_{pos}", pts, [5.0 + (n - 1) / 2.0], [10.0], dict(accepted=1, area_accept=n), w, th=20.0)
    # nq 1024 / 1025: queries 0 and 1024 (a thread's register slot and its memory slot) want the same feature
    for nq in (1024, 1025):
        pts = [(10.0, 10.0, 0, 0.0, bits(3)), (12.0, 10.0, 0, 0.0, bits(30))]
        u = np.full(nq, 40.0, np.float32)
        u[0] = 11.0
        u[-1] = 11.0
        w = [0, nq - 1]
        R(f"nq_{nq}_first_and_last_collide", pts, u, np.full(nq, 10.0, np.float32), dict(accepted=2, blocked=1), w)
    return out


def stereo_cases():
    out = []
    # uRight 0.0f / -0.0f / -1 are "no right coordinate" for the projection searches (> 0); the smallest positive float is one
    tiny = np.float32(1e-45)
    pts = [(10.0 + 4 * k, 10.0, 0, 0.0, bits(5)) for k in range(4)]
    ur = [0.0, -0.0, -1.0, tiny]
    fr = mk_frame(pts, UNIT, ur)
    u = np.array([p[0] for p in pts], np.float32)
    q = _q(4)
    # projected right coordinate 50: er = 50 > radius 1.5 wherever the check runs
    out.append(Case("uright_zero_is_monocular_for_projection", "mappoints", fr,
                    dict(in_view=q["valid"], level=q["level"], view_cos=np.full(4, 0.9, np.float32), px=u, py=np.full(4, 10.0, np.float32),
                         pxr=np.full(4, 50.0, np.float32), desc=q["desc"], obs=None, blocked=None, th=0.375, nnratio=0.8),
                    dict(stereo_skipped=3, stereo_reject=1, accepted=3), [0, 1, 2, -1]))
    # er == radius (kept: strict >) and one float above (dropped); radius = th * sf[0] = 2
    # (second point: ur = 4 - 1 = 3, uRight = 1 - 2^-22, er = 2 + 2^-22, the float above 2)
    pts = [(10.0, 10.0, 0, 0.0, bits(5)), (4.0, 20.0, 0, 0.0, bits(5))]
    fr = mk_frame(pts, UNIT, [7.0, 1.0 - 2.0 ** -22])
    assert f32(f32(3.0) - f32(1.0 - 2.0 ** -22)) == nxt(2.0)
    out.append(Case("er_equals_radius_lastframe", "lastframe", fr,
                    dict(**_q(2), u=np.array([10.0, 4.0], np.float32), v=np.array([10.0, 20.0], np.float32), mbf=1.0,
                         invzc=np.ones(2, np.float32), obs=None, blocked=None, mode=0, th=2.0, check_ori=False),
                    dict(stereo_pass=1, stereo_reject=1), [0, -1]))
    pts = [(10.0, 10.0, 0, 0.0, bits(5)), (20.0, 10.0, 0, 0.0, bits(5))]
    fr = mk_frame(pts, UNIT, [8.0, 18.0])
    assert f32(nxt(20.0) - f32(18.0)) > f32(2.0)
    out.append(Case("er_equals_radius_mappoints", "mappoints", fr,
                    dict(in_view=np.ones(2, np.uint8), level=np.zeros(2, np.int32), view_cos=np.full(2, 0.9, np.float32),
                         px=np.array([10.0, 20.0], np.float32), py=np.full(2, 10.0, np.float32),
                         pxr=np.array([10.0, nxt(20.0)], np.float32), desc=np.zeros((2, 32), np.uint8), obs=None, blocked=None,
                         th=0.5, nnratio=0.8),
                    dict(stereo_pass=1, stereo_reject=1), [0, -1]))
    # u - mbf * invzc where a fused multiply-add rounds differently from multiply-then-subtract: uRight is placed so that
    # er == radius for the two-step value and er > radius for the fused one
    u0, mbf, iz = fma_triple()
    two_step = f32(u0 - f32(mbf * iz))
    fused = f32(np.float64(u0) - np.float64(mbf) * np.float64(iz))
    assert two_step != fused
    lo_, hi_ = (two_step, fused) if two_step < fused else (fused, two_step)
    radius = f32(2.0)
    # right coordinate exactly `radius` away from the two-step value on the side away from the fused one
    urv = f32(two_step - radius) if fused > two_step else f32(two_step + radius)
    assert abs(f32(two_step - urv)) == radius and abs(f32(fused - urv)) > radius
    fr = mk_frame([(u0, 10.0, 0, 0.0, bits(5))], VGA, [urv])
    out.append(Case("lastframe_ur_not_contracted", "lastframe", fr,
                    dict(**_q(1), u=np.array([u0], np.float32), v=np.full(1, 10.0, np.float32), mbf=float(mbf),
                         invzc=np.array([iz], np.float32), obs=None, blocked=None, mode=0, th=2.0, check_ori=False),
                    dict(stereo_pass=1, accepted=1), [0]))
    return out


def fma_triple():
    """(u, mbf, invzc) floats with fl(u - fl(mbf * invzc)) != fl(u - mbf * invzc), u inside a 640-px image and the
    right coordinate positive; found by a seeded search"""
    rng = np.random.default_rng(7)
    while True:
        u = rng.uniform(100, 600, 4096).astype(np.float32)
        mbf = np.float32(40.0) + rng.uniform(0, 1, 4096).astype(np.float32)
        iz = rng.uniform(0.05, 1.0, 4096).astype(np.float32)
        two = (u - (mbf * iz).astype(np.float32)).astype(np.float32)
        fused = (u.astype(np.float64) - mbf.astype(np.float64) * iz.astype(np.float64)).astype(np.float32)
        k = np.flatnonzero((two != fused) & (two > 50))
        if k.size:
            return u[k[0]], mbf[k[0]], iz[k[0]]


def mappoint_cases():
    out = []

    def M(name, pts, px, py, expect, want, ur=None, **kw):
        n = len(px)
        a = dict(in_view=np.ones(n, np.uint8), level=np.zeros(n, np.int32), view_cos=np.full(n, 0.9, np.float32),
                 px=np.array(px, np.float32), py=np.array(py, np.float32), pxr=None, desc=np.zeros((n, 32), np.uint8), obs=None,
                 blocked=None, th=1.0, nnratio=0.8)
        a.update(kw)
        out.append(Case(name, "mappoints", mk_frame(pts, UNIT, ur), a, expect, want))
    # viewCos: the two floats adjacent to the double 0.998 -- radius 4 below, 2.5 above; the feature sits 3 px away
    below = f32(0.998)
    if float(below) > 0.998:
        below = nxt(below, False)
    above = nxt(below)
    assert float(below) <= 0.998 < float(above)
    pts = [(13.0, 10.0, 0, 0.0, bits(5)), (33.0, 10.0, 0, 0.0, bits(5))]
    M("viewcos_either_side_of_0998", pts, [10.0, 30.0], [10.0, 10.0], dict(accepted=1, radius_reject=1), [0, -1],
      view_cos=np.array([below, above], np.float32))
    # th == 1.0: no factor; the next float multiplies (radius 4 -> 4.0000005: a feature exactly 4 px away comes in)
    pts = [(14.0, 10.0, 0, 0.0, bits(5))]
    M("th_exactly_one", pts, [10.0], [10.0], dict(radius_reject=1), [-1], th=1.0)
    M("th_next_float_above_one", pts, [10.0], [10.0], dict(accepted=1), [0], th=float(nxt(1.0)))
    # ratio: bestDist > nnratio * bestDist2 rejects (same level only).  0.8f * 50 = 40.000001 in float: 40 passes, 41 fails
    for ratio, d2, eq in ((0.8, 50, 40), (0.6, 50, 30)):
        prod = f32(f32(ratio) * f32(d2))
        for tag, d1 in (("below", eq - 1), ("at", eq), ("above", eq + 1)):
            rej = bool(f32(d1) > prod)
            for lev_tag, o2 in (("same_level", 0), ("other_level", 1)):
                pts = [(10.0, 10.0, 0, 0.0, bits(d1)), (11.0, 10.0, o2, 0.0, bits(d2, 100))]
                exp = dict(better_second=1)
                if rej and o2 == 0:
                    exp.update(ratio_reject=1)
                    w = [-1, -1]
                else:
                    exp.update(accepted=1, ratio_pass_levels_differ=1 if rej else 0)
                    w = [0, -1]
                M(f"ratio_{ratio}_{tag}_{lev_tag}", pts, [10.5], [10.0], exp, w, level=np.ones(1, np.int32), nnratio=ratio)
    M("single_candidate_bestlevel2_unset", [(10.0, 10.0, 0, 0.0, bits(90))], [10.0], [10.0],
      dict(accepted=1, better_second=0, ratio_pass_levels_differ=0), [0])
    # the second best is blocked at entry: it never becomes bestDist2, so the ratio test does not see it
    pts = [(10.0, 10.0, 0, 0.0, bits(45)), (11.0, 10.0, 0, 0.0, bits(46, 100))]
    M("second_best_blocked", pts, [10.5], [10.0], dict(blocked=1, accepted=1, better_second=0), [0, -1],
      blocked=np.array([0, 1], np.uint8))
    M("second_best_free_rejects", pts, [10.5], [10.0], dict(ratio_reject=1, better_second=1), [-1, -1])
    # a point without observations leaves its feature free: the later point overwrites the match (and both count)
    pts = [(10.0, 10.0, 0, 0.0, bits(5))]
    M("obs_zero_leaves_feature_free", pts, [10.0, 10.5], [10.0, 10.0], dict(accepted=2, blocked=0), [1],
      obs=np.array([0, 1], np.uint8))
    M("obs_positive_blocks_feature", pts, [10.0, 10.5], [10.0, 10.0], dict(accepted=1, blocked=1), [0],
      obs=np.array([1, 1], np.uint8))
    # level window [level - 1, level] at level 0: (-1, 0) checks levels (maxLevel >= 0) and keeps octave 0 only
    pts = [(10.0, 10.0, 0, 0.0, bits(5)), (11.0, 10.0, 1, 0.0, bits(1, 50))]
    M("level_window_at_level_zero", pts, [10.5], [10.0], dict(level_reject_high=1, accepted=1), [0, -1])
    return out


def fuse_cases():
    """the chi-square gate one float below, at and one float above 5.99 / 7.8 AFTER the float product: e2 * invSigma2 is
    steered through invSigma2 (a table the caller passes), e2 = 3*3 + 0 = 9 (+ 0 for the right coordinate)"""
    out = []
    for k, (arm, limit, ur_kf, tag, p, rejected) in enumerate(_gate_targets()):
        # key point of octave k reads GATE_SIGMA[k]; the query's level is k, so the level window [k - 1, k] keeps it
        fr = mk_frame([(13.0, 10.0, k, 0.0, bits(5))], UNIT, [ur_kf])
        a = dict(**_q(1, level=np.full(1, k, np.int32)), u=np.array([10.0], np.float32), v=np.array([10.0], np.float32),
                 ur=np.array([0.0], np.float32), th=4.0, chi2=True, inv_sigma2=GATE_SIGMA)
        assert f32(f32(9.0) * GATE_SIGMA[k]) == p
        key = f"chi2_{arm}_{'reject' if rejected else 'pass'}"
        out.append(Case(f"gate_{arm}_{tag}", "fuse", fr, a, {key: 1}, [-1 if rejected else 0]))
    # a stereo key point whose right coordinate is -0.0f: >= 0 is true for negative zero as well (e2 = 9 + 4 > 7.8)
    fr = mk_frame([(13.0, 10.0, 6, 0.0, bits(5))], UNIT, [-0.0])
    out.append(Case("gate_negative_zero_uright_is_stereo", "fuse", fr,
                    dict(**_q(1, level=np.full(1, 6, np.int32)), u=np.array([10.0], np.float32), v=np.array([10.0], np.float32),
                         ur=np.array([2.0], np.float32), th=4.0, chi2=True, inv_sigma2=GATE_SIGMA), dict(chi2_stereo_reject=1), [-1]))
    # level window at level 0, with and without the gate; distance at TH_LOW and above
    pts = [(10.0, 10.0, 0, 0.0, bits(TH_LOW)), (11.0, 10.0, 1, 0.0, bits(1, 60)), (30.0, 10.0, 0, 0.0, bits(TH_LOW + 1))]
    for chi2 in (True, False):
        fr = mk_frame(pts, UNIT)
        out.append(Case(f"level_zero_and_th_low_chi2_{int(chi2)}", "fuse", fr,
                        dict(**_q(2), u=np.array([10.5, 30.0], np.float32), v=np.array([10.0, 10.0], np.float32), ur=None,
                             th=3.0, chi2=chi2, inv_sigma2=INV_SIGMA2),
                        dict(level_reject_high=1, accepted=1, threshold_reject=1), [0, -1]))
    # equal minima in two columns, later index first in scan order (the device takes the first in scan order)
    pts = [(12.0, 10.0, 0, 0.0, bits(7, 0)), (9.0, 10.0, 0, 0.0, bits(7, 8)), (10.0, 10.0, 2, 0.0, bits(0))]
    out.append(Case("fuse_equal_minima_scan_order", "fuse", mk_frame(pts, UNIT),
                    dict(**_q(1), u=np.array([10.5], np.float32), v=np.array([10.0], np.float32), ur=None, th=3.0, chi2=False,
                         inv_sigma2=INV_SIGMA2), dict(tie_ignored=1, level_reject_high=1), [1]))
    return out


def _gate_targets():
    """(arm, limit, key point's uRight, tag, product, rejected): the floats around the double limits.  uRight == 0.0f takes
    the STEREO arm (>= 0)"""
    out = []
    for arm, limit, ur_kf in (("mono", 5.99, -1.0), ("stereo", 7.8, 0.0)):
        p_at = f32(limit)
        if float(p_at) > limit:
            p_at = nxt(p_at, False)          # the largest float <= limit: not rejected (strict >)
        assert float(p_at) <= limit < float(nxt(p_at))
        out += [(arm, limit, ur_kf, "below", nxt(p_at, False), False), (arm, limit, ur_kf, "at", p_at, False),
                (arm, limit, ur_kf, "above", nxt(p_at), True)]
    return out


def _gate_sigma():
    """mvInvLevelSigma2 with entry k chosen so that fl(9 * sigma[k]) is the k-th product of _gate_targets(); 1 beyond"""
    sig = np.ones(8, np.float32)
    for k, t in enumerate(_gate_targets()):
        sig[k] = _factor_for(f32(9.0), t[4])
    return sig


def _factor_for(a, p):
    """a float f with fl(a * f) == p (searched around p / a)"""
    f = f32(p / a)
    for _ in range(64):
        got = f32(a * f)
        if got == p:
            return f
        f = nxt(f, bool(got < p))
    raise AssertionError("no factor")


def hist_cases():
    """rotation histogram through the key-frame form (every take is pushed, a pruned entry clears its feature)"""
    out = []

    def H(name, pairs, expect, want=None, check_ori=True, kind="reloc"):
        """pairs: (query angle, feature angle); query k sits on feature k, far from the others"""
        n = len(pairs)
        pts = [(2.0 + 3.0 * (k % 20), 2.0 + 3.0 * (k // 20), 0, a2, bits(5)) for k, (_, a2) in enumerate(pairs)]
        u = np.array([p[0] for p in pts], np.float32)
        v = np.array([p[1] for p in pts], np.float32)
        a = dict(**_q(n, angle=np.array([a1 for a1, _ in pairs], np.float32)), u=u, v=v, th=1.0, orb_dist=100,
                 check_ori=check_ori, blocked=None)
        out.append(Case(name, kind, mk_frame(pts, UNIT), a, expect, want))
    # 15 -> round(0.5) = 1, 45 -> round(1.5) = 2, 345 -> round(11.5) = 12 (half away from zero; truncation and
    # round-half-even give 0 / 1 or 2 / 11 or 12).  Three bins of one entry each: all kept
    H("rot_bin_edges_15_45_345", [(15.0, 0.0), (45.0, 0.0), (345.0, 0.0)], dict(maxima_all_kept=1, hist_pruned=0), [0, 1, 2])
    # bin membership made visible: 10 entries in bin 1 (15 deg exactly), 10 in bin 2 (45), 10 in bin 12 (345), one each in
    # bins 0, 3 and 11 -- the one-entry bins are pruned; a wrong rounding moves the edge entries into them
    H("rot_bin_edges_decide_pruning", [(15.0, 0.0)] * 10 + [(45.0, 0.0)] * 10 + [(345.0, 0.0)] * 10 +
      [(0.0, 0.0), (90.0, 0.0), (330.0, 0.0)], dict(hist_pruned=3, maxima_all_kept=1),
      list(range(30)) + [-1, -1, -1])
    H("equal_angles_bin_zero", [(77.0, 77.0)] * 3 + [(100.0, 10.0)], dict(hist_pruned=0, max3_below_tenth=1), [0, 1, 2, 3])
    # a1 - a2 a tiny negative: rot + 360 rounds to 360.0f, bin 12 (not 0, not 30)
    a2 = nxt(100.0)
    assert f32(f32(f32(100.0) - a2) + f32(360.0)) == f32(360.0)
    # (bins 0, 1, 2 hold three each, bin 12 these two: pruned.  In bin 0 they would make it five and nothing would go)
    H("tiny_negative_becomes_360", [(100.0, a2)] * 2 + [(0.0, 0.0)] * 3 + [(30.0, 0.0)] * 3 + [(60.0, 0.0)] * 3,
      dict(hist_pruned=2, maxima_all_kept=1), [-1, -1] + list(range(2, 11)))
    # 10 % rule: max2 == 0.1f * max1 exactly is NOT below (strict <): 10/1 keeps bin 2, 20/2/1 drops the third
    # (1 < 0.1f * 20 = 2.0000000298 in float -> 2.0f), 20/1 drops the second: 1 < 2
    H("tenth_10_1", [(0.0, 0.0)] * 10 + [(30.0, 0.0)], dict(max2_below_tenth=0, hist_pruned=0), list(range(11)))
    H("tenth_20_2_2", [(0.0, 0.0)] * 20 + [(30.0, 0.0)] * 2 + [(60.0, 0.0)] * 2, dict(maxima_all_kept=1, hist_pruned=0),
      list(range(24)))
    H("tenth_20_2_1", [(0.0, 0.0)] * 20 + [(30.0, 0.0)] * 2 + [(60.0, 0.0)], dict(max3_below_tenth=1, hist_pruned=1),
      list(range(22)) + [-1])
    H("tenth_20_1", [(0.0, 0.0)] * 20 + [(30.0, 0.0)], dict(max2_below_tenth=1, hist_pruned=1), list(range(20)) + [-1])
    # ties between bins: the first bin in index order keeps the higher place; with four equal bins the fourth goes
    H("tied_bins", [(0.0, 0.0)] * 2 + [(30.0, 0.0)] * 2 + [(60.0, 0.0)] * 2 + [(90.0, 0.0)] * 2, dict(hist_pruned=2, maxima_all_kept=1),
      [0, 1, 2, 3, 4, 5, -1, -1])
    H("two_bins_only", [(0.0, 0.0)] * 3 + [(30.0, 0.0)] * 3, dict(hist_pruned=0, max3_below_tenth=1), list(range(6)))
    H("check_ori_off", [(0.0, 0.0)] * 20 + [(30.0, 0.0)], dict(max2_below_tenth=0, maxima_all_kept=0, hist_pruned=0), list(range(21)),
      check_ori=False)
    # no match at all: an empty histogram (0 < 0.1f * 0 is false twice: "all kept" of nothing)
    out.append(Case("no_match_at_all", "reloc", mk_frame([(10.0, 10.0, 0, 0.0, bits(120))], UNIT),
                    dict(**_q(1), u=np.array([10.0], np.float32), v=np.array([10.0], np.float32), th=1.0, orb_dist=100,
                         check_ori=True, blocked=None), dict(threshold_reject=1, maxima_all_kept=1), [-1]))
    # the last-frame form pushes a feature twice when its first holder does not block it
    pts = [(10.0, 10.0, 0, 0.0, bits(5)), (30.0, 10.0, 0, 0.0, bits(5)), (40.0, 10.0, 0, 0.0, bits(5))]
    out.append(Case("lastframe_feature_pushed_twice", "lastframe", mk_frame(pts, UNIT),
                    dict(**_q(4, angle=np.array([90.0, 90.0, 0.0, 0.0], np.float32)), u=np.array([10.0, 10.5, 30.0, 40.0], np.float32),
                         v=np.full(4, 10.0, np.float32), mbf=0.0, invzc=None, obs=np.array([0, 1, 1, 1], np.uint8), blocked=None,
                         mode=0, th=2.0, check_ori=True), dict(accepted=4, hist_pruned=0, max3_below_tenth=1), [1, 2, 3]))
    return out


def init_cases():
    out = []

    def I(name, p1, p2, expect, want, window=5, nnratio=0.9, check_ori=False, prev=None):
        f1, f2 = mk_frame(p1, UNIT), mk_frame(p2, UNIT)
        prev = np.stack([f1["x"], f1["y"]], 1) if prev is None else np.array(prev, np.float32)
        out.append(Case(name, "init", f2, dict(prev=prev, window=window, nnratio=nnratio, check_ori=check_ori), expect, want, frame1=f1))
    far = (40.0, 30.0, 0, 0.0, bits(120, 40))  # a second candidate far in Hamming distance keeps the ratio test easy
    # a later query takes the feature at a smaller distance: the earlier match is cleared, nmatches decremented
    I("later_query_takes_feature", [(10.0, 10.0, 0, 0.0, bits(10)), (10.5, 10.0, 0, 0.0, bits(4))], [(10.0, 10.0, 0, 0.0, Z)],
      dict(init_overwrite=1, accepted=2), [-1, 0])
    I("later_query_refused_at_equal_distance", [(10.0, 10.0, 0, 0.0, bits(10)), (10.5, 10.0, 0, 0.0, bits(10, 50))],
      [(10.0, 10.0, 0, 0.0, Z)], dict(init_refused=1, accepted=1, no_candidate=1), [0, -1])
    # ratio: bestDist < bestDist2 * 0.9f strict; 0.9f * 50 = 45.000000745 -> 45.0f in float: 45 < 45 is false
    I("ratio_at_equality_rejects", [(10.0, 10.0, 0, 0.0, Z)], [(10.0, 10.0, 0, 0.0, bits(45)), (11.0, 10.0, 0, 0.0, bits(50, 100))],
      dict(ratio_reject=1), [-1])
    I("ratio_one_below_accepts", [(10.0, 10.0, 0, 0.0, Z)], [(10.0, 10.0, 0, 0.0, bits(44)), (11.0, 10.0, 0, 0.0, bits(50, 100))],
      dict(accepted=1, better_second=1), [0])
    I("single_candidate_bestdist2_int_max", [(10.0, 10.0, 0, 0.0, Z)], [(10.0, 10.0, 0, 0.0, bits(50))], dict(accepted=1, better_second=0), [0])
    I("threshold_one_above_th_low", [(10.0, 10.0, 0, 0.0, Z)], [(10.0, 10.0, 0, 0.0, bits(51))], dict(threshold_reject=1), [-1])
    I("level_one_of_f1_skipped", [(10.0, 10.0, 1, 0.0, Z), (10.0, 10.0, 0, 0.0, Z)], [(10.0, 10.0, 0, 0.0, bits(3)), (11.0, 10.0, 1, 0.0, bits(1, 9))],
      dict(accepted=1, level_reject_high=1), [-1, 0])
    # prev_x / prev_y: a matched query moves to its feature, an unmatched one keeps what it had
    I("prev_updated_for_matched_only", [(10.0, 10.0, 0, 0.0, Z), (30.0, 30.0, 0, 0.0, Z)], [(12.0, 11.0, 0, 0.0, bits(3))],
      dict(accepted=1), [0, -1], prev=[(11.0, 10.0), (31.5, 29.5)])
    # a replaced query stays in the histogram: its bin is pruned, it is already unmatched and is not counted again.
    # queries 0..9 -> bin 0; query 10 (angle 90, bin 3) takes feature 10 and is then replaced by query 11 (bin 0)
    p2 = [(2.0 + 3.0 * k, 5.0, 0, 0.0, Z) for k in range(11)]
    p1 = [(2.0 + 3.0 * k, 5.0, 0, 0.0, bits(3, k)) for k in range(10)] + [(32.0, 5.0, 0, 90.0, bits(10)), (32.5, 5.0, 0, 0.0, bits(4))]
    I("replaced_query_still_in_histogram", p1, p2, dict(init_overwrite=1, hist_prune_already_unmatched=1, hist_pruned=0, max2_below_tenth=1),
      list(range(10)) + [-1, 10], window=1, check_ori=True)
    # the same with the pruned entry still matched: counted
    p1b = [(2.0 + 3.0 * k, 5.0, 0, 0.0, bits(3, k)) for k in range(20)]
    p2b = [(2.0 + 3.0 * k, 5.0, 0, 0.0, Z) for k in range(20)]
    p1b += [(8.0, 20.0, 0, 90.0, bits(3))]
    p2b += [(8.0, 20.0, 0, 0.0, Z)]
    I("pruned_entry_still_matched", p1b, p2b, dict(hist_pruned=1, max2_below_tenth=1), list(range(20)) + [-1], window=1, check_ori=True)
    return out


def sim3_cases():
    out = []
    # KF1 features 0..2, KF2 features 0..2.  Pair 0 agrees both ways; KF1's 1 points at KF2's 1, which points back at
    # KF1's 2 (one direction only); KF1's 2 is invalid.  Then both valid but pointing elsewhere, and one side all invalid
    k1 = [(10.0, 10.0, 0, 0.0, bits(2)), (20.0, 10.0, 0, 0.0, bits(4, 20)), (20.5, 10.0, 0, 0.0, bits(4, 40))]
    k2 = [(30.0, 30.0, 0, 0.0, bits(3)), (40.0, 30.0, 0, 0.0, bits(4, 60)), (50.0, 30.0, 0, 0.0, bits(90, 100))]

    def S(name, valid1, valid2, u2, expect, want):
        a = dict(valid1=np.array(valid1, np.uint8), u1=np.array([30.0, 40.0, 50.0], np.float32), v1=np.full(3, 30.0, np.float32),
                 level1=np.zeros(3, np.int32), desc1=np.stack([bits(3), bits(4, 60), bits(90, 100)]),
                 valid2=np.array(valid2, np.uint8), u2=np.array(u2, np.float32), v2=np.full(3, 10.0, np.float32),
                 level2=np.zeros(3, np.int32), desc2=np.stack([bits(2), bits(4, 40), bits(4, 40)]), th=1.0)
        out.append(Case(name, "sim3", mk_frame(k2, UNIT), a, expect, want, frame1=mk_frame(k1, UNIT)))
    S("agree_one_direction_only", [1, 1, 0], [1, 1, 0], [10.0, 20.5, 0.0], dict(sim3_mutual=1, sim3_one_way_only=1), [0, -1, -1])
    S("both_valid_pointing_elsewhere", [1, 1, 1], [1, 1, 1], [10.0, 20.5, 20.5], dict(sim3_mutual=2, sim3_one_way_only=1), [0, -1, 2])
    S("empty_valid_on_one_side", [1, 1, 1], [0, 0, 0], [10.0, 20.0, 20.5], dict(sim3_mutual=0, sim3_one_way_only=3), [-1, -1, -1])
    return out


def sim3proj_cases():
    pts = [(10.0, 10.0, 0, 0.0, bits(TH_LOW)), (30.0, 10.0, 0, 0.0, bits(TH_LOW + 1)), (40.0, 10.0, 2, 0.0, bits(1)),
           (40.5, 10.0, 0, 0.0, bits(9)), (50.0, 10.0, 0, 0.0, bits(2))]
    a = dict(**_q(5, level=np.array([0, 0, 1, 0, 0], np.int32)), u=np.array([10.0, 30.0, 40.0, 50.0, 50.5], np.float32),
             v=np.full(5, 10.0, np.float32), th=2.0, matched=np.array([0, 0, 0, 0, 0], np.uint8))
    c1 = Case("sim3proj_th_low_levels_and_claims", "sim3proj", mk_frame(pts, UNIT), a,
              dict(accepted=3, threshold_reject=1, level_reject_high=1, blocked=1, no_candidate=1), [0, -1, -1, 2, 3])
    a2 = dict(a, matched=np.array([1, 0, 0, 0, 0], np.uint8))
    c2 = Case("sim3proj_matched_at_entry", "sim3proj", mk_frame(pts, UNIT), a2, dict(blocked=2, no_candidate=2), [-1, -1, -1, 2, 3])
    return [c1, c2]


def named_cases():
    return (area_cases() + best_cases() + stereo_cases() + mappoint_cases() + fuse_cases() + hist_cases() + init_cases() +
            sim3_cases() + sim3proj_cases())


# ---- seeded cases: 200 small ones per search ------------------------------------------------------------------------
KINDS = ("area", "mappoints", "lastframe", "reloc", "sim3proj", "init", "fuse", "sim3")
_BOUNDS3 = (UNIT, VGA, OFFSET)


def _seeded_frame(rng, bounds, stereo):
    n = int(rng.integers(20, 61))
    minx, maxx, miny, maxy = bounds
    x = (np.floor(rng.uniform(minx - 2, maxx + 2, n) * 2) / 2).astype(np.float32)   # 0.5-px lattice
    y = (np.floor(rng.uniform(miny - 2, maxy + 2, n) * 2) / 2).astype(np.float32)
    k = n // 3
    x[:k] = np.clip(x[:k], minx, minx + (maxx - minx) / 8)                          # a dense corner: shared windows
    y[:k] = np.clip(y[:k], miny, miny + (maxy - miny) / 8)
    pool = np.stack([bits(int(d), int(s)) for d, s in zip(rng.integers(0, 60, 8), rng.integers(0, 200, 8))])
    fr = dict(x=x, y=y, octave=rng.integers(0, 4, n).astype(np.int32), angle=(rng.integers(0, 48, n) * 7.5).astype(np.float32),
              desc=pool[rng.integers(0, 8, n)], bounds=bounds, u_right=None)
    if stereo:
        fr["u_right"] = np.where(rng.random(n) < 0.7, x - rng.integers(0, 6, n), rng.choice([-1.0, 0.0], n)).astype(np.float32)
    return fr, pool


def _seeded_queries(rng, fr, pool):
    nq = int(rng.integers(20, 81))
    src = rng.integers(0, len(fr["x"]), nq)                                         # several queries per feature
    u = (fr["x"][src] + rng.integers(-4, 5, nq) * 0.5).astype(np.float32)
    v = (fr["y"][src] + rng.integers(-4, 5, nq) * 0.5).astype(np.float32)
    q = dict(valid=(rng.random(nq) < 0.9).astype(np.uint8), level=np.clip(fr["octave"][src] + rng.integers(0, 2, nq), 0, 7).astype(np.int32),
             angle=(rng.integers(0, 48, nq) * 7.5).astype(np.float32), desc=pool[rng.integers(0, 8, nq)])
    return q, u, v, src


def seeded_case(kind, seed):
    rng = np.random.default_rng([KINDS.index(kind), seed])
    bounds = _BOUNDS3[seed % 3]
    stereo = kind in ("mappoints", "lastframe", "fuse") and seed % 2 == 0
    fr, pool = _seeded_frame(rng, bounds, stereo)
    q, u, v, src = _seeded_queries(rng, fr, pool)
    n, nq = len(fr["x"]), len(u)
    scale = (bounds[1] - bounds[0]) / 64.0
    th = float(rng.integers(1, 4)) * (1.0 if bounds is UNIT else 4.0)
    name = f"seeded_{kind}_{seed}"
    blocked = (rng.random(n) < 0.15).astype(np.uint8) if seed % 4 else None
    if kind == "area":
        lv = [(-1, -1), (0, -1), (2, -1), (0, 3), (1, 2), (3, 1)]
        qs = [(u[i], v[i], f32(rng.integers(1, 8) * max(1.0, scale / 2)), *lv[rng.integers(0, 6)]) for i in range(nq)]
        return Case(name, kind, fr, dict(q=qs))
    if kind == "mappoints":
        return Case(name, kind, fr, dict(in_view=q["valid"], level=q["level"], view_cos=rng.choice(np.array([0.9, 0.998, 0.9995], np.float32), nq),
                                         px=u, py=v, pxr=(u - rng.integers(0, 6, nq)).astype(np.float32) if stereo else None, desc=q["desc"],
                                         obs=(rng.random(nq) < 0.7).astype(np.uint8) if seed % 3 else None, blocked=blocked,
                                         th=th if seed % 5 else 1.0, nnratio=0.8 if seed % 2 else 0.6))
    if kind == "lastframe":
        return Case(name, kind, fr, dict(**q, u=u, v=v, mbf=4.0, invzc=(rng.integers(0, 6, nq) * 0.25).astype(np.float32),
                                         obs=(rng.random(nq) < 0.7).astype(np.uint8) if seed % 3 else None, blocked=blocked,
                                         mode=seed % 3, th=th * 2, check_ori=bool(seed % 4 != 1)))
    if kind == "reloc":
        return Case(name, kind, fr, dict(**q, u=u, v=v, th=th * 2, orb_dist=int(rng.choice([100, 64, 30])), check_ori=bool(seed % 4 != 1),
                                         blocked=blocked))
    if kind == "sim3proj":
        return Case(name, kind, fr, dict(**q, u=u, v=v, th=float(int(th * 2)), matched=blocked))
    if kind == "fuse":
        return Case(name, kind, fr, dict(**q, u=u, v=v, ur=(u - rng.integers(0, 6, nq)).astype(np.float32), th=th, chi2=bool(seed % 3),
                                         inv_sigma2=(INV_SIGMA2 * f32(1.0 if bounds is UNIT else 0.05)).astype(np.float32)))
    if kind == "init":
        fr["octave"] = np.where(rng.random(n) < 0.8, 0, 1).astype(np.int32)
        f1 = dict(x=u, y=v, octave=np.where(rng.random(nq) < 0.85, 0, 1).astype(np.int32), angle=q["angle"], desc=q["desc"], bounds=bounds,
                  u_right=None)
        return Case(name, kind, fr, dict(prev=np.stack([u, v], 1), window=int(max(1, th)), nnratio=0.9, check_ori=bool(seed % 4 != 1)), frame1=f1)
    if kind == "sim3":
        f1, pool1 = _seeded_frame(rng, bounds, False)
        n1 = len(f1["x"])
        s2 = rng.integers(0, n, n1)          # KF1 point i1 projects near KF2 feature s2[i1] and carries its descriptor
        f1["desc"] = fr["desc"][s2].copy()
        u1 = (fr["x"][s2] + rng.integers(-2, 3, n1) * 0.5).astype(np.float32)
        v1 = (fr["y"][s2] + rng.integers(-2, 3, n1) * 0.5).astype(np.float32)
        back = np.zeros(n, np.int64)
        back[s2] = np.arange(n1)             # KF2 feature s2[i1] projects back near KF1 feature i1 (the last one wins)
        u2 = (f1["x"][back] + rng.integers(-2, 3, n) * 0.5).astype(np.float32)
        v2 = (f1["y"][back] + rng.integers(-2, 3, n) * 0.5).astype(np.float32)
        return Case(name, kind, fr, dict(valid1=(rng.random(n1) < 0.9).astype(np.uint8), u1=u1, v1=v1, level1=np.clip(fr["octave"][s2] + rng.integers(0, 2, n1), 0, 7).astype(np.int32),
                                         desc1=f1["desc"], valid2=(rng.random(n) < 0.9).astype(np.uint8), u2=u2, v2=v2,
                                         level2=np.clip(f1["octave"][back] + rng.integers(0, 2, n), 0, 7).astype(np.int32), desc2=fr["desc"],
                                         th=th * 2), frame1=f1)
    raise ValueError(kind)


def seeded_cases(per_kind=200):
    return [seeded_case(k, s) for k in KINDS for s in range(per_kind)]


# ---- runners: one case through the restatement, the oracle, the device ----------------------------------------------
def _norm(res):
    """results as plain lists (counts as ints, index arrays as lists, float arrays as their bit patterns)"""
    out = []
    for r in res:
        if isinstance(r, (int, np.integer)):
            out.append(int(r))
        elif isinstance(r, list) and r and isinstance(r[0], list):
            out.append([[int(v) for v in w] for w in r])
        else:
            a = np.asarray(r)
            out.append(np.ascontiguousarray(a, np.float32).view(np.uint32).tolist() if a.dtype.kind == "f" else a.tolist())
    return out


def run_restatement(c: Case):
    F = RFrame(**{k: c.frame[k] for k in ("x", "y", "octave", "desc", "bounds", "angle", "u_right")})
    a = c.args
    if c.kind == "area":
        T = Counter()
        return _norm([[F.area(x, y, r, lo, hi, T) for (x, y, r, lo, hi) in a["q"]]]), T
    if c.kind == "mappoints":
        r, T = search_mappoints(F, SF, a["blocked"], a["in_view"], a["level"], a["view_cos"], a["px"], a["py"], a["pxr"], a["desc"], a["obs"],
                                a["th"], a["nnratio"])
    elif c.kind == "lastframe":
        r, T = search_lastframe(F, SF, a["mbf"], a["valid"], a["u"], a["v"], a["invzc"], a["level"], a["angle"], a["desc"], a["obs"],
                                a["blocked"], a["mode"], a["th"], a["check_ori"])
    elif c.kind == "reloc":
        r, T = search_reloc(F, SF, a["valid"], a["u"], a["v"], a["level"], a["angle"], a["desc"], a["blocked"], a["th"], a["orb_dist"],
                            a["check_ori"])
    elif c.kind == "sim3proj":
        r, T = search_sim3proj(F, SF, a["valid"], a["u"], a["v"], a["level"], a["desc"], a["matched"], a["th"])
    elif c.kind == "fuse":
        r, T = search_fuse(F, SF, a["inv_sigma2"], a["valid"], a["u"], a["v"], a["ur"], a["level"], a["desc"], a["th"], a["chi2"])
    else:
        F1 = RFrame(**{k: c.frame1[k] for k in ("x", "y", "octave", "desc", "bounds", "angle", "u_right")})
        if c.kind == "init":
            r, T = search_init(F1, F, a["prev"], a["window"], a["nnratio"], a["check_ori"])
        else:
            r, T = search_sim3(F1, F, SF, SF, a["valid1"], a["u1"], a["v1"], a["level1"], a["desc1"], a["valid2"], a["u2"], a["v2"],
                               a["level2"], a["desc2"], a["th"])
    return _norm(r), T


def _ur_or_zero(a, key, n):
    return a[key] if a[key] is not None else np.zeros(n, np.float32)


def run_oracle(c: Case, frame=None):
    import oracle_lib as orc
    fr = frame or c.frame
    mk = lambda f: orc.Frame(f["x"], f["y"], f["octave"], f["desc"], f["bounds"], angle=f["angle"], u_right=f["u_right"])  # noqa: E731
    F, a = mk(fr), c.args
    if c.kind == "area":
        tot, res = Counter(), []
        for (x, y, r, lo, hi) in a["q"]:
            res.append(F.features_in_area(x, y, r, lo, hi).tolist())
            tot.update(orc.window_branch_counts())
        return _norm([res]), tot
    if c.kind == "mappoints":
        pxr = a["pxr"] if a["pxr"] is not None else (np.zeros(len(a["px"]), np.float32) if fr["u_right"] is not None else None)
        r = orc.search_by_projection_mappoints(F, SF, a["blocked"], a["in_view"], a["level"], a["view_cos"], a["px"], a["py"], pxr, a["desc"],
                                               a["obs"], a["th"], a["nnratio"])
    elif c.kind == "lastframe":
        r = orc.search_by_projection_lastframe(F, SF, a["mbf"], a["valid"], a["u"], a["v"], a["invzc"], a["level"], a["angle"], a["desc"],
                                               a["obs"], a["mode"], a["th"], a["check_ori"], a["blocked"])
    elif c.kind == "reloc":
        r = orc.search_by_projection_reloc(F, SF, a["valid"], a["u"], a["v"], a["level"], a["angle"], a["desc"], a["blocked"], a["th"],
                                           a["orb_dist"], a["check_ori"])
    elif c.kind == "sim3proj":
        r = orc.search_by_projection_sim3(F, SF, a["valid"], a["u"], a["v"], a["level"], a["desc"], a["matched"], a["th"])
    elif c.kind == "fuse":
        r = (orc.fuse_search(F, SF, a["inv_sigma2"], a["valid"], a["u"], a["v"], _ur_or_zero(a, "ur", len(a["u"])), a["level"], a["desc"],
                             a["th"], a["chi2"]),)
    elif c.kind == "init":
        r = orc.search_for_initialization(mk(c.frame1), F, a["prev"].copy(), a["window"], a["nnratio"], a["check_ori"])
    else:
        r = orc.search_by_sim3(mk(c.frame1), F, SF, SF, a["valid1"], a["u1"], a["v1"], a["level1"], a["desc1"], a["valid2"], a["u2"],
                               a["v2"], a["level2"], a["desc2"], a["th"])
    return _norm(r), Counter(orc.window_branch_counts())


def gpu_frame(amd, f, resident):
    F = amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], f["bounds"], angle=f["angle"], u_right=f["u_right"])
    return F.upload() if resident else F


def run_gpu(amd, c: Case, resident, frame=None):
    """the single-call route of every search"""
    fr = frame or c.frame
    F, a = gpu_frame(amd, fr, resident), c.args
    if c.kind == "area":
        q = a["q"]
        got = F.GetFeaturesInArea(np.array([t[0] for t in q], np.float32), np.array([t[1] for t in q], np.float32),
                                  np.array([t[2] for t in q], np.float32), np.array([t[3] for t in q], np.int32),
                                  np.array([t[4] for t in q], np.int32), capacity=8)
        return _norm([[g.tolist() for g in got]])
    if c.kind == "mappoints":
        pxr = a["pxr"] if a["pxr"] is not None else (np.zeros(len(a["px"]), np.float32) if fr["u_right"] is not None else None)
        r = amd.ORBmatcher(a["nnratio"], True).SearchByProjection(F, SF, a["in_view"], a["level"], a["view_cos"], a["px"], a["py"], a["desc"],
                                                                  th=a["th"], proj_xr=pxr, blocked=a["blocked"], mp_obs_positive=a["obs"])
    elif c.kind == "lastframe":
        iz = a["invzc"] if a["invzc"] is not None else np.zeros(len(a["u"]), np.float32)
        r = amd.ORBmatcher(0.9, a["check_ori"]).SearchByProjectionLastFrame(F, SF, a["valid"], a["u"], a["v"], a["level"], a["angle"], a["desc"],
                                                                            a["th"], mode=a["mode"], mbf=a["mbf"], invzc=iz,
                                                                            obs_positive=a["obs"], blocked=a["blocked"])
    elif c.kind == "reloc":
        r = amd.ORBmatcher(0.9, a["check_ori"]).SearchByProjectionKeyFrame(F, SF, a["valid"], a["u"], a["v"], a["level"], a["angle"], a["desc"],
                                                                           a["th"], a["orb_dist"], blocked=a["blocked"])
    elif c.kind == "sim3proj":
        r = amd.ORBmatcher(0.75, True).SearchByProjectionSim3(F, SF, a["valid"], a["u"], a["v"], a["level"], a["desc"], a["th"], matched=a["matched"])
    elif c.kind == "fuse":
        r = (amd.ORBmatcher(0.6).FuseSearch(F, SF, a["valid"], a["u"], a["v"], a["level"], a["desc"], th=a["th"],
                                            inv_level_sigma2=a["inv_sigma2"] if a["chi2"] else None, ur=_ur_or_zero(a, "ur", len(a["u"]))),)
    elif c.kind == "init":
        prev = a["prev"].copy()
        n, m = amd.ORBmatcher(a["nnratio"], a["check_ori"]).SearchForInitialization(gpu_frame(amd, c.frame1, resident), F, prev, a["window"])
        r = (n, m, prev)
    else:
        r = amd.ORBmatcher(0.75).SearchBySim3(gpu_frame(amd, c.frame1, resident), F, SF, SF, a["valid1"], a["u1"], a["v1"], a["level1"],
                                              a["desc1"], a["valid2"], a["u2"], a["v2"], a["level2"], a["desc2"], a["th"])
    return _norm(r)


GATE_SIGMA = _gate_sigma()


def outcome(c: Case, res):
    """the result array a case's `want` spells out: the window lists, best_idx, or the match array behind the count"""
    return res[0] if c.kind in ("area", "fuse") else res[1]
