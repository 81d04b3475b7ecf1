"""Engineered stereo problems for Frame::ComputeStereoMatches (src/Frame.cc:512-686) and a numpy restatement of it.

Test infrastructure only (no GPU, no product import).  Two things live here:

* ``stereo_numpy``: a restatement of the reference's text in plain Python / numpy, independent of oracle/orb_oracle.c.
  Float steps the reference takes in ``float`` are ``np.float32``; the SAD is an integer (see ``_sad_strip``).  It also
  returns, per left keypoint, where the keypoint left the loop (``EXITS``) and the intermediate values, so a test can
  check that an engineered keypoint took the path it was built for.
* ``engineered_cases()`` / ``random_cases()``: named 320x200 stereo problems, 8 levels, scale 1.2 (level 7 is 89x56).
  Keypoint records and descriptors are hand-placed; images have controlled content so that the SAD curve of a chosen
  keypoint is known by construction.

Image content (level 0; the engineered SAD keypoints are all octave 0, where the pyramid is the image itself):

* texture: box-filtered seeded noise; the right image is the left one moved 7 px to the left plus +-4 grey levels of
  noise -> clean interior SAD minima with a non-zero floor (so the median of a population is not 0).
* "V zone": 23+ px of the triangular numbers T(t) = t(t+1)/2 (0..253) along x, the same in every row.  For a left
  patch centred at t = a and a right patch centred at t' = b: (T(a+dx) - T(a)) - (T(b+dx) - T(b)) = (a - b) dx, so
  SAD(inc) = 330 |a - (b0 + inc)| exactly: a V with its vertex wherever the case wants it (strip end -5 / +5, -4 / +4,
  or the centre), dist1 == dist3 at the vertex (deltaR = 0), and a disparity chosen by where the zones sit in the two
  images (0 for the clamp, 38 / 42 around maxD = 40, -2 for a negative one).
* constant zone: every SAD is 0; the first shift (-5) wins: rejected at the strip's end.
* period-3 zone: I[y, x] = P[y, x mod 3] in both images: SAD(inc) = 0 at three or four shifts; the first interior one wins.
* "cells" (median cases): a grid of V zones whose left patch carries an extra delta on its first column, which makes
  the SAD minimum exactly delta: the list of bestD values that reaches the median cut is chosen freely.

Two things the reference's text rules out, proved here and asserted in tests/test_stereo_edges.py:

* |deltaR| > 1 cannot happen.  SADs are integers.  bestincR is the FIRST shift with the minimal SAD (strict ``<``
  against an int that holds an integer exactly), and bestincR = -5 is rejected before the fit, so dist1 > dist2 and
  dist3 >= dist2.  With a = dist1 - dist2 >= 1 and b = dist3 - dist2 >= 0, deltaR = (a - b) / (2 (a + b)) and
  |a - b| <= a + b, so |deltaR| <= 1/2; all operands are integers below 2^18, exact in float, and the one rounding
  (the division) is monotonic, so the float result is within [-0.5, 0.5] too.
* For the same reason dist1 == dist2 == dist3 (0/0, NaN) cannot reach the fit: a + b >= 1.  Constant patches give
  eleven equal SADs, the first wins, and the keypoint leaves at ``bestincR == -L``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

import oracle_lib as orc

W, H, NLEVELS, SCALE = 320, 200, 8, 1.2
TH_HIGH, TH_LOW = 100, 50
F = np.float32

# exits of the per-keypoint loop, in the order of orc_stereo_branch_counts (oracle/orb_oracle.h)
EXITS = ("invalid_record", "row_out_of_range", "empty_row", "maxu_negative", "no_candidate", "hamming_above_th",
         "iniu_negative", "endu_past_cols", "guard_cy_low", "guard_cy_high", "guard_cxl_low", "guard_cxl_high",
         "guard_cxr_low", "bestinc_low_end", "bestinc_high_end", "delta_out_of_range", "delta_nan_passed",
         "disparity_out_of_range", "disparity_clamped", "accepted", "median_removed")
# proved unreachable in the module docstring
UNREACHABLE = ("delta_out_of_range", "delta_nan_passed")


# ------------------------------------------------------------------------------------------------------------------
# restatement
# ------------------------------------------------------------------------------------------------------------------
def _roundf(x) -> int:
    """C round() of a float: half away from zero (exact in double for |x| < 2^52)."""
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def _hamming(a, b) -> int:
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def _sad_strip(IL, IR, cy, cxL, cxR0):
    """The eleven L1 norms of :624-638 as integers.  IL / IR patches are 8-bit; after the centre is subtracted both are
    integers in [-255, 255], their difference is in [-510, 510], and the sum of 121 absolute values is at most
    121 * 510 = 61710 < 2^24: every partial sum is an integer a float (and a double) holds exactly, so the reference's
    float arithmetic and this integer one give the same numbers."""
    w, L = 5, 5
    pl = IL[cy - w: cy + w + 1, cxL - w: cxL + w + 1].astype(np.int64) - int(IL[cy, cxL])
    out = []
    for inc in range(-L, L + 1):
        c = cxR0 + inc
        pr = IR[cy - w: cy + w + 1, c - w: c + w + 1].astype(np.int64) - int(IR[cy, c])
        s = int(np.abs(pl - pr).sum())
        assert 0 <= s <= 121 * 510 < 2 ** 24
        out.append(s)
    return out


def stereo_numpy(sf, isf, kpL, dL, kpR, dR, pyrL, pyrR, mbf, mb):
    """-> (mvuRight, mvDepth, trace).  sf / isf: mvScaleFactors / mvInvScaleFactors (float32); pyrL / pyrR: lists of
    2-D uint8 levels.  Where the reference would index out of range or throw (records no extractor writes; a patch that
    leaves its level: cv::Mat::rowRange / colRange assert), the keypoint gets "no stereo", as in the oracle."""
    N, Nr = len(kpL), len(kpR)
    nlev = len(pyrL)
    u = np.full(N, -1.0, F)
    z = np.full(N, -1.0, F)
    trace = [dict(exit=None) for _ in range(N)]
    thOrbDist = (TH_HIGH + TH_LOW) // 2                                       # :517
    nRows = pyrL[0].shape[0]                                                  # :519
    rows = [[] for _ in range(nRows)]                                         # :522
    for iR in range(Nr):                                                      # :529-539
        kpY, octR = F(kpR["y"][iR]), int(kpR["octave"][iR])
        if octR < 0 or octR >= nlev or not (abs(kpY) < F(3.0e38)):
            continue
        r = F(2.0) * sf[octR]
        maxr = int(math.ceil(F(kpY + r)))
        minr = int(math.floor(F(kpY - r)))
        for yi in range(max(minr, 0), min(maxr, nRows - 1) + 1):
            rows[yi].append(iR)
    mbf, mb = F(mbf), F(mb)
    minD = F(0)
    maxD = F(mbf / mb)                                                        # :542-544
    vDistIdx = []
    for iL in range(N):                                                       # :550
        t = trace[iL]
        levelL, vL, uL = int(kpL["octave"][iL]), F(kpL["y"][iL]), F(kpL["x"][iL])
        if levelL < 0 or levelL >= nlev or not (abs(uL) < F(3.0e38)) or not (abs(vL) < F(3.0e38)):
            t["exit"] = "invalid_record"
            continue
        row = int(vL)                                                         # vRowIndices[vL]: truncation
        if row < 0 or row >= nRows:
            t["exit"] = "row_out_of_range"
            continue
        cand = rows[row]
        if not cand:                                                          # :559
            t["exit"] = "empty_row"
            continue
        minU, maxU = F(uL - maxD), F(uL - minD)
        if maxU < 0:                                                          # :565
            t["exit"] = "maxu_negative"
            continue
        bestDist, bestIdxR, inrange = TH_HIGH, 0, 0
        for iR in cand:                                                       # :574-595
            octR = int(kpR["octave"][iR])
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = F(kpR["x"][iR])
            if uR >= minU and uR <= maxU:
                inrange += 1
                d = _hamming(dL[iL], dR[iR])
                if d < bestDist:
                    bestDist, bestIdxR = d, iR
        t.update(bestDist=bestDist, bestIdxR=bestIdxR if bestDist < TH_HIGH else -1)
        if not bestDist < thOrbDist:                                          # :598
            t["exit"] = "no_candidate" if inrange == 0 else "hamming_above_th"
            continue
        uR0 = F(kpR["x"][bestIdxR])
        scaleFactor = isf[levelL]
        scaleduL = _roundf(F(uL * scaleFactor))
        scaledvL = _roundf(F(vL * scaleFactor))
        scaleduR0 = _roundf(F(uR0 * scaleFactor))
        w, L = 5, 5
        IL, IR = pyrL[levelL], pyrR[levelL]
        lh, lw = IL.shape
        iniu, endu = scaleduR0 + L - w, scaleduR0 + L + w + 1
        if iniu < 0:                                                          # :621
            t["exit"] = "iniu_negative"
            continue
        if endu >= lw:
            t["exit"] = "endu_past_cols"
            continue
        for name, hit in (("guard_cy_low", scaledvL < w), ("guard_cy_high", scaledvL + w >= lh),
                          ("guard_cxl_low", scaleduL < w), ("guard_cxl_high", scaleduL + w >= lw),
                          ("guard_cxr_low", scaleduR0 < L + w)):              # rowRange / colRange asserts
            if hit:
                t["exit"] = name
                break
        if t["exit"]:
            continue
        dists = _sad_strip(IL, IR, scaledvL, scaleduL, scaleduR0)
        bestD, bestincR = 2 ** 31 - 1, 0                                      # :613
        for k, dist in enumerate(dists):
            if F(dist) < F(bestD):                                            # float < int: the int is converted
                bestD, bestincR = int(F(dist)), k - L
        t.update(dists=dists, bestincR=bestincR, bestD=bestD)
        if bestincR == -L or bestincR == L:                                   # :640
            t["exit"] = "bestinc_low_end" if bestincR == -L else "bestinc_high_end"
            continue
        dist1, dist2, dist3 = (F(dists[L + bestincR + k]) for k in (-1, 0, 1))
        with np.errstate(all="ignore"):
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))   # :648
        t.update(fit=(float(dist1), float(dist2), float(dist3)), deltaR=deltaR)
        if deltaR < -1 or deltaR > 1:
            t["exit"] = "delta_out_of_range"
            continue
        bestuR = F(sf[levelL] * F(F(F(scaleduR0) + F(bestincR)) + deltaR))    # :654
        disparity = F(uL - bestuR)
        if disparity >= minD and disparity < maxD:                            # :658 (false for NaN)
            t["exit"] = "accepted"
            if disparity <= 0:
                t["clamped"] = True
                disparity = F(0.01)                                           # a float variable
                bestuR = F(np.float64(uL) - 0.01)                             # `uL-0.01` is a double expression
            z[iL] = F(mbf / disparity)
            u[iL] = bestuR
            vDistIdx.append((bestD, iL))
        else:
            t["exit"] = "disparity_out_of_range"
    if vDistIdx:                                                              # :672-685 (empty: UB in the reference)
        vDistIdx.sort()
        median = F(vDistIdx[len(vDistIdx) // 2][0])
        thDist = F(F(F(1.5) * F(1.4)) * median)
        for d, iL in reversed(vDistIdx):
            if F(d) < thDist:
                break
            u[iL] = -1
            z[iL] = -1
            trace[iL]["median_removed"] = True
    return u, z, trace


def branch_counts_of(trace):
    """the counters orc_stereo_branch_counts would show for this trace (same order as EXITS)"""
    c = dict.fromkeys(EXITS, 0)
    for t in trace:
        c[t["exit"]] += 1
        c["disparity_clamped"] += bool(t.get("clamped"))
        c["median_removed"] += bool(t.get("median_removed"))
        c["delta_nan_passed"] += bool("deltaR" in t and t["deltaR"] != t["deltaR"] and t["exit"] != "delta_out_of_range")
    return c


# ------------------------------------------------------------------------------------------------------------------
# images
# ------------------------------------------------------------------------------------------------------------------
DISP = 7            # texture disparity, level-0 pixels
MBF, MB = 100.0, 2.5  # maxD = 40 exactly


def _T(t):
    return t * (t + 1) // 2


def _texture(rng, h, w):
    n = rng.integers(0, 256, (h + 2, w + 2)).astype(np.float64)
    b = sum(n[dy: dy + h, dx: dx + w] for dy in range(3) for dx in range(3)) / 9.0
    b = (b - b.mean()) / b.std() * 45.0 + 128.0
    return np.clip(np.rint(b), 0, 255).astype(np.uint8)


# V zones of canvas A: name -> (row of the keypoints, x of t = 0 in the left image, in the right image); 25 rows high
V_ZONES = {"v0": (154, 50, 50), "v6": (154, 90, 84), "vm2": (154, 130, 132), "v38": (184, 60, 22), "v42": (184, 150, 108)}
CONST_ZONE = (154, 8, 40)      # row, x0, x1 (both images)
PERIOD_ZONE = (154, 170, 216)  # row, x0, x1 (both images)


def canvas_a():
    """the image pair every case but the median ones uses"""
    rng = np.random.default_rng(20240501)
    base = _texture(rng, H, W + DISP)
    left = base[:, :W].copy()
    right = np.clip(base[:, DISP:].astype(np.int16) + rng.integers(-4, 5, (H, W)), 0, 255).astype(np.uint8)
    for row, xl0, xr0 in V_ZONES.values():
        ramp = np.array([_T(t) for t in range(23)], np.uint8)
        left[row - 12: row + 13, xl0: xl0 + 23] = ramp
        right[row - 12: row + 13, xr0: xr0 + 23] = ramp
    row, x0, x1 = CONST_ZONE
    left[row - 12: row + 13, x0:x1] = 128
    right[row - 12: row + 13, x0:x1] = 128
    row, x0, x1 = PERIOD_ZONE
    P = rng.integers(0, 256, (25, 3)).astype(np.uint8)
    per = P[:, np.arange(x0, x1) % 3]
    left[row - 12: row + 13, x0:x1] = per
    right[row - 12: row + 13, x0:x1] = per
    return left, right


CELL_PITCH_X, CELL_PITCH_Y, CELL_COLS, CELL_ROWS = 27, 13, 11, 14


def cell_xy(k):
    """cell k of the median canvas -> (uL, uR, v) of its keypoint pair"""
    i, j = divmod(k, CELL_COLS)
    x0, y = 8 + CELL_PITCH_X * j, 11 + CELL_PITCH_Y * i
    return x0 + 12, x0 + 10, y


def canvas_cells(deltas):
    """one V cell per entry; cell k's SAD minimum is exactly deltas[k] (at shift 0, disparity about 2).  The delta sits
    on the left patch's first column (t = 5, T = 15), at most 240 per row: for a shift of +-1 the SAD is at least
    275 + sum |delta_r -+ 5| >= delta + 220, further out more, so shift 0 is the one minimum."""
    assert len(deltas) <= CELL_COLS * CELL_ROWS and max(deltas, default=0) <= 11 * 240
    left, right = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    ramp = np.array([_T(t) for t in range(23)], np.uint8)
    for k, delta in enumerate(deltas):
        uL, uR, y = cell_xy(k)
        left[y - 5: y + 6, uL - 10: uL + 13] = ramp
        right[y - 5: y + 6, uR - 10: uR + 13] = ramp
        rest = int(delta)
        for r in range(11):
            d = min(rest, 240)
            left[y - 5 + r, uL - 5] = 15 + d
            rest -= d
    return left, right


# ------------------------------------------------------------------------------------------------------------------
# records
# ------------------------------------------------------------------------------------------------------------------
_SF = None


def scale_factors():
    global _SF
    if _SF is None:
        _SF = orc.Oracle(1000, SCALE, NLEVELS, 20, 7).scale_factors()
    return _SF


def make_kp(x, y, octave=0):
    kp = np.zeros((), orc.KP_DTYPE)
    kp["x"], kp["y"], kp["octave"] = F(x), F(y), octave
    kp["size"] = F(31.0) * scale_factors()[min(max(int(octave), 0), NLEVELS - 1)]
    kp["response"], kp["class_id"] = 50.0, -1
    return kp


def flip_bits(base, k, rng):
    """a descriptor at Hamming distance exactly k from base"""
    bits = np.unpackbits(base)
    bits[rng.choice(256, size=k, replace=False)] ^= 1
    return np.packbits(bits)


@dataclass
class Case:
    name: str
    images: tuple                      # key into image_pairs()
    kpL: list = field(default_factory=list)
    dL: list = field(default_factory=list)
    kpR: list = field(default_factory=list)
    dR: list = field(default_factory=list)
    mbf: float = MBF
    mb: float = MB
    # (left index, exit the keypoint must leave by, extra trace fields that must hold) -- checked on the restatement's
    # trace in test_stereo_edges.py; the counter of that exit must be > 0 in the oracle as well
    expect: list = field(default_factory=list)
    host_ok: bool = True               # False: holds records orbfe_compute_stereo_matches answers with ORBFE_ERR_INVALID

    def left(self, x, y, octave=0, desc=None):
        self.kpL.append(make_kp(x, y, octave))
        self.dL.append(desc)
        return len(self.kpL) - 1

    def right(self, x, y, octave=0, desc=None):
        self.kpR.append(make_kp(x, y, octave))
        self.dR.append(desc)
        return len(self.kpR) - 1

    def arrays(self):
        f = lambda k: np.array(k, orc.KP_DTYPE) if len(k) else np.zeros(0, orc.KP_DTYPE)
        g = lambda d: np.stack(d).astype(np.uint8) if len(d) else np.zeros((0, 32), np.uint8)
        return f(self.kpL), g(self.dL), f(self.kpR), g(self.dR)


def _plain(c: Case, rng, n, ymax=92):
    """n matching pairs on the texture (rows 8..ymax, octaves 0..3), Hamming distance 0..40: the population the median
    cut works on; returns the left indices"""
    sf = scale_factors()
    out = []
    for _ in range(n):
        o = int(rng.choice(4, p=[0.5, 0.25, 0.15, 0.1]))
        s = float(sf[o])
        x = float(rng.integers(int(60 / s), int((W - 24) / s))) * s
        y = float(rng.integers(int(12 / s) + 6, int(ymax / s))) * s
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        out.append(c.left(x, y, o, base))
        c.right(F(x) - F(DISP), y, o, flip_bits(base, int(rng.integers(0, 41)), rng))
    return out


def _case(name, seed, plain=36, images=("A",)):
    c = Case(name, images)
    rng = np.random.default_rng(seed)
    _plain(c, rng, plain)
    return c, rng


def _pair(c, rng, uL, v, uR, dist=0, vR=None, octL=0, octR=0):
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    iL = c.left(uL, v, octL, base)
    iR = c.right(uR, v if vR is None else vR, octR, flip_bits(base, dist, rng))
    return iL, iR


def engineered_cases():
    """the named cases; every one carries the plain population unless it is about sizes"""
    cases = []
    add = cases.append
    TY = 112  # a texture row below the plain population's rows

    # ---- exits before the candidate scan ----
    c, rng = _case("empty_row", 101)
    i, _ = _pair(c, rng, 200, TY, 193, vR=TY + 9)              # the right twin's band ends 6 rows short
    c.expect.append((i, "empty_row", {}))
    add(c)

    c, rng = _case("records_the_device_form_guards", 102)       # the classes test_stereo_device_operands_are_not_trusted uses
    i, _ = _pair(c, rng, -3.0, TY, 1.0)                         # row has the twin; maxU = -3 < 0
    c.expect.append((i, "maxu_negative", {}))
    i, _ = _pair(c, rng, 200, -40.0, 193, vR=TY)
    c.expect.append((i, "row_out_of_range", {}))
    i, _ = _pair(c, rng, 200, 1.0e6, 193, vR=TY)
    c.expect.append((i, "row_out_of_range", {}))
    for x, y, o in ((np.nan, 50.0, 1), (100.0, np.inf, 0), (120.0, 60.0, 9), (120.0, 60.0, -3)):
        i = c.left(x, y, o, rng.integers(0, 256, 32, dtype=np.uint8))
        c.expect.append((i, "invalid_record", {}))
    for x, y, o in ((np.nan, TY, 0), (100.0, np.inf, 0), (120.0, TY, 9), (1.0e9, TY, 0), (0.0, 0.0, 0)):
        c.right(x, y, o, rng.integers(0, 256, 32, dtype=np.uint8))
    i, _ = _pair(c, rng, 30.0, TY + 12, -2.0)                   # round(uR0) = -2: the left end of the strip
    c.expect.append((i, "iniu_negative", {}))
    c.host_ok = False
    add(c)

    # ---- candidate scan ----
    c, rng = _case("no_candidate", 103)
    i, _ = _pair(c, rng, 200, TY, 150)                          # 50 px left: below minU = 160
    c.expect.append((i, "no_candidate", {}))
    i, _ = _pair(c, rng, 120, TY, 121)                          # right of the left keypoint: above maxU
    c.expect.append((i, "no_candidate", {}))
    i, _ = _pair(c, rng, 200, TY + 12, 193, octR=2)             # in range, octave 2 against 0
    c.expect.append((i, "no_candidate", {}))
    add(c)

    c, rng = _case("hamming_thresholds", 104)
    for k, (dist, ex) in enumerate(((74, "accepted"), (75, "hamming_above_th"), (99, "hamming_above_th"),
                                    (100, "hamming_above_th"), (0, "accepted"))):
        i, iR = _pair(c, rng, 80 + 50 * k, TY + (k % 2) * 12, 73 + 50 * k, dist)
        # a distance of 100 is in range but never becomes bestDist (strict < against TH_HIGH)
        c.expect.append((i, ex, dict(bestDist=min(dist, 100), bestIdxR=iR if dist < 100 else -1)))
    add(c)

    c, rng = _case("hamming_tie_first_wins", 105)
    # two right keypoints at the same distance; only the first in right-index order sits on the true match
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    i = c.left(200, TY, 0, base)
    good = c.right(193, TY, 0, flip_bits(base, 30, rng))
    c.right(175, TY, 0, flip_bits(base, 30, rng))
    c.right(186, TY + 1, 0, flip_bits(base, 31, rng))
    c.expect.append((i, "accepted", dict(bestIdxR=good, bestDist=30)))
    # and the other way round: the first is 18 px off the match, the true one comes second and must lose
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    i = c.left(120, TY + 12, 0, base)
    bad = c.right(95, TY + 12, 0, flip_bits(base, 30, rng))
    c.right(113, TY + 12, 0, flip_bits(base, 30, rng))
    c.expect.append((i, None, dict(bestIdxR=bad, bestDist=30)))
    add(c)

    c, rng = _case("u_range_ends_inclusive", 106)
    # maxU: uR == uL exactly, in the zero-disparity V zone (also the clamp); minU: uR == uL - 40 exactly in the
    # 38-px zone with the vertex at +2 (disparity 38 < maxD); one float below minU is out
    row, xl0, xr0 = V_ZONES["v0"]
    i, _ = _pair(c, rng, xl0 + 10, row, xr0 + 10)
    c.expect.append((i, "accepted", dict(clamped=True, bestincR=0)))
    row, xl0, xr0 = V_ZONES["v38"]
    i, _ = _pair(c, rng, xl0 + 12, row, xr0 + 10)
    assert xl0 + 12 - 40 == xr0 + 10
    c.expect.append((i, "accepted", dict(bestincR=2)))
    row, xl0, xr0 = V_ZONES["v42"]
    i, _ = _pair(c, rng, xl0 + 8, row, np.nextafter(F(xr0 + 10), F(-1e9)))
    assert xl0 + 8 - 40 == xr0 + 10
    c.expect.append((i, "no_candidate", {}))
    add(c)

    c, rng = _case("octave_difference", 107)
    sf = scale_factors()
    k = 0
    for octL, octR, ok in ((0, 1, True), (0, 2, False), (1, 0, True), (2, 0, False), (7, 6, True), (7, 5, False),
                           (6, 7, True), (5, 7, False)):
        s = float(sf[octL])
        # level coordinates (24 + 5 j, 16 + ...) keep every patch inside level 7 (89 x 56) as well
        xl, yl = (40 + 9 * (k % 4)), (18 + 5 * (k // 4) if octL >= 5 else int(TY / s) + 3 * (k % 2))
        x, y = xl * s, yl * s
        i, _ = _pair(c, rng, x, y, F(x) - F(DISP), octL=octL, octR=octR)
        # (a rejected twin leaves no candidate of its own; a neighbour's right keypoint may still be in range)
        c.expect.append((i, "accepted", {}) if ok else (i, None, dict(bestIdxR=-1)))
        k += 1
    add(c)

    c, rng = _case("row_band_ends", 108)
    # right keypoint at y = 112.3, octave 0: rows floor(110.3) = 110 .. ceil(114.3) = 115; octave 1 (r = 2.4) at
    # y = 112: rows floor(109.6) = 109 .. ceil(114.4) = 115.  Left keypoints on the last row inside and the first outside
    for k, (vL, inside) in enumerate(((110.0, True), (109.9, False), (115.9, True), (116.0, False))):
        i, _ = _pair(c, rng, 70 + 60 * k, vL, 63 + 60 * k, vR=112.3)
        c.expect.append((i, "accepted" if inside else "empty_row", {}))
    add(c)
    c, rng = _case("row_band_ends_octave1", 109)
    for k, (vL, inside) in enumerate(((109.0, True), (108.9, False), (115.5, True), (116.0, False))):
        i, _ = _pair(c, rng, 70 + 60 * k, vL, 63 + 60 * k, vR=112.0, octR=1)
        c.expect.append((i, "accepted" if inside else "empty_row", {}))
    add(c)

    # ---- strip and patch guards ----
    c, rng = _case("strip_and_patch_guards", 110)
    for uL, v, uR, ex in ((318, TY, 310, "endu_past_cols"),     # round(uR0) + 11 = 321 >= 320
                          (312, TY + 12, 309, "endu_past_cols"),  # 320 >= 320: the end is exclusive
                          (316, TY + 24, 308, "guard_cxl_high"),  # endu = 319 passes; the left patch needs column 321
                          (314, TY - 12, 308, "accepted"),        # columns 309..319: the last legal place
                          (30, 3, 23, "guard_cy_low"), (60, 4.4, 53, "guard_cy_low"), (90, 4.6, 83, "accepted"),
                          (280, 195, 273, "guard_cy_high"), (250, 194.4, 243, "accepted"),
                          (3, 30, 1, "guard_cxl_low"), (4.4, 42, 2, "guard_cxl_low"),
                          (12, 54, 4, "guard_cxr_low"), (16, 66, 9.4, "guard_cxr_low"), (17, 78, 10, "accepted")):
        i, _ = _pair(c, rng, uL, v, uR)
        c.expect.append((i, ex, {}))
    add(c)

    # ---- SAD strip ----
    c, rng = _case("sad_minimum_at_strip_ends", 111)
    row, xl0, xr0 = V_ZONES["v6"]
    for tL, inc, ex in ((5, -5, "bestinc_low_end"), (6, -4, "accepted"), (14, 4, "accepted"), (15, 5, "bestinc_high_end")):
        i, _ = _pair(c, rng, xl0 + tL, row, xr0 + 10)
        fit = {} if ex != "accepted" else dict(fit=(330.0, 0.0, 330.0))
        c.expect.append((i, ex, dict(bestincR=inc, bestD=0, **fit)))
    row, x0, x1 = CONST_ZONE
    i, _ = _pair(c, rng, 26, row, 22)                           # constant patches: eleven zeros, the first wins
    c.expect.append((i, "bestinc_low_end", dict(dists=[0] * 11)))
    add(c)

    c, rng = _case("sad_equal_minima_first_wins", 112)
    row, x0, x1 = PERIOD_ZONE
    for k, (uR_off, inc, ex) in enumerate(((3, -3, "accepted"), (2, -4, "accepted"), (1, -5, "bestinc_low_end"))):
        # identical period-3 content: SAD 0 at every shift = uR_off (mod 3), three or four of the eleven; the first one
        # is kept (a later equal value is not < the int best), and when that is -5 the keypoint is dropped
        uL = x0 + 22 + k
        i, _ = _pair(c, rng, uL, row, uL - uR_off)
        c.expect.append((i, ex, dict(bestincR=inc, bestD=0)))
    add(c)

    c, rng = _case("disparity_ends_and_clamp", 113)
    row, xl0, xr0 = V_ZONES["v0"]
    i, _ = _pair(c, rng, xl0 + 14, row, xr0 + 10)               # vertex at +4, disparity exactly 0 -> 0.01
    c.expect.append((i, "accepted", dict(clamped=True, bestincR=4, deltaR=F(0))))
    row, xl0, xr0 = V_ZONES["vm2"]
    i, _ = _pair(c, rng, xl0 + 12, row, xr0 + 10)               # uR0 == uL, vertex at +2: disparity -2
    assert xl0 + 12 == xr0 + 10
    c.expect.append((i, "disparity_out_of_range", dict(bestincR=2)))
    row, xl0, xr0 = V_ZONES["v42"]
    i, _ = _pair(c, rng, xl0 + 8, row, xr0 + 10)                # uR0 == minU, vertex at -2: disparity 42 >= maxD
    c.expect.append((i, "disparity_out_of_range", dict(bestincR=-2)))
    row, xl0, xr0 = V_ZONES["v38"]
    i, _ = _pair(c, rng, xl0 + 13, row, xr0 + 11)               # uR0 == minU again, vertex at +2: disparity 38, inside
    c.expect.append((i, "accepted", dict(bestincR=2)))
    add(c)

    # ---- median cut: the bestD values are the cell deltas, in left-index order ----
    c15 = F(F(1.5) * F(1.4))
    exact = [m for m in range(1, 400) if float(F(c15 * F(m))).is_integer()]
    assert exact, "no median whose threshold is an integer"
    m = exact[0]
    th = int(F(c15 * F(m)))
    median_cases = {
        "median_odd": ([40, 10, 100, 30, 20], [2]),
        "median_even_upper_middle": ([100, 10, 50, 20], []),    # sorted[4 // 2] = 50, th 105; the lower middle would cut 50 and 100
        "median_even_cut": ([30, 100, 10, 20], [1]),
        "median_single": ([40], []),
        "median_zero": ([0, 5, 0, 0], [0, 1, 2, 3]),            # th = 0 and 0 < 0 is false: everything goes
        "median_run_at_threshold": ([m, th, m, th - 1, th, m, m], [1, 4]),   # th is an integer: == is cut, th - 1 stays
        "median_equal_run": ([10, 21, 10, 21, 10, 21, 20, 22], None),
        "median_above_one_byte": ([250, 600, 255, 257, 256, 1300, 2640], None),
        "median_all_equal": ([77] * 9, []),
    }
    for name, (deltas, removed) in median_cases.items():
        c = Case(name, ("cells", tuple(deltas)))
        rng = np.random.default_rng(len(cases))
        for k, dlt in enumerate(deltas):
            uL, uR, y = cell_xy(k)
            i, _ = _pair(c, rng, uL, y, uR)
            c.expect.append((i, "accepted", dict(bestD=dlt, bestincR=0,
                                                 **({} if removed is None else dict(median_removed=k in removed)))))
        add(c)
    # a realistic population: 150 cells, deltas drawn around 300 with a tail
    rng = np.random.default_rng(114)
    deltas = [int(v) for v in np.clip(rng.gamma(3.0, 110.0, 150), 0, 2640)]
    c = Case("median_population_150", ("cells", tuple(deltas)))
    for k, dlt in enumerate(deltas):
        uL, uR, y = cell_xy(k)
        i, _ = _pair(c, rng, uL, y, uR)
        c.expect.append((i, "accepted", dict(bestD=dlt)))
    add(c)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


# the stereo kernels' launch shape (csrc/k_match.hip): k_stereo_match gives a left keypoint the 16 lanes of a DPP row, so
# 4 keypoints per wavefront and 16 per 256-thread workgroup; the candidate scan strides the row band's records 16 at a
# time; k_stereo_median_cut walks the keypoints 256 at a time
LANES_PER_KEYPOINT, KEYPOINTS_PER_WAVE, KEYPOINTS_PER_WORKGROUP, MEDIAN_CUT_THREADS = 16, 4, 16, 256
SEAM_SIZES = (0, 1, KEYPOINTS_PER_WAVE - 1, KEYPOINTS_PER_WAVE, KEYPOINTS_PER_WAVE + 1, KEYPOINTS_PER_WORKGROUP - 1,
              KEYPOINTS_PER_WORKGROUP, KEYPOINTS_PER_WORKGROUP + 1, 63, 64, 65, MEDIAN_CUT_THREADS - 1,
              MEDIAN_CUT_THREADS, MEDIAN_CUT_THREADS + 1)


def seam_cases():
    """sizes at the kernels' seams: N (with Nr = N), Nr = 0, N = 0 against a full right side, one crowded row"""
    cases = []
    for n in SEAM_SIZES:
        c = Case(f"n_{n}", ("A",))
        _plain(c, np.random.default_rng(300 + n), n, ymax=136)
        cases.append(c)
    c = Case("nr_0", ("A",))
    _plain(c, np.random.default_rng(401), 20)
    c.kpR, c.dR = [], []
    cases.append(c)
    c = Case("n_0_nr_40", ("A",))
    _plain(c, np.random.default_rng(402), 40)
    c.kpL, c.dL = [], []
    cases.append(c)
    # one row band with 3 * 16 + 5 right keypoints in range of one left keypoint: more than the scan takes per pass.
    # All at distance 60 but three at 30: record 20 (on the true match), 37 and 52 (off it); and a second left keypoint
    # whose only good candidate is the very last record
    c, rng = _case("crowded_row", 403)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    base2 = rng.integers(0, 256, 32, dtype=np.uint8)
    i = c.left(200, 112, 0, base)
    i2 = c.left(200, 113, 0, base2)
    first = len(c.kpR)
    n = 3 * LANES_PER_KEYPOINT + 5
    xs = [161 + (k * 17) % 39 for k in range(n)]              # all inside [160, 200], none at 193
    for k in range(n):
        tie = k in (20, 37, 52)
        x = 193 if k in (20, n - 1) else (xs[k] if xs[k] != 193 else 192)
        d = flip_bits(base, 30 if tie else 60, rng) if k != n - 1 else flip_bits(base2, 10, rng)
        c.right(x, 112 + (k % 3) - 1, 0, d)
    c.expect.append((i, "accepted", dict(bestIdxR=first + 20, bestDist=30)))
    c.expect.append((i2, "accepted", dict(bestIdxR=first + n - 1, bestDist=10)))
    cases.append(c)
    return cases


RANDOM_SEEDS = tuple(range(7000, 7200))


def random_case(seed):
    """1..130 keypoints per side over canvas A: matching pairs at any octave, unrelated records, and positions whose
    patches leave the level (legal to pass, "no stereo").  Every fourth seed also plants the record classes
    orbfe_compute_stereo_matches rejects and the device form answers with "no stereo" (host_ok False)."""
    rng = np.random.default_rng(seed)
    sf = scale_factors()
    c = Case(f"random_{seed}", ("A",))
    nL, nR = int(rng.integers(1, 131)), int(rng.integers(1, 131))
    bad = seed % 4 == 0
    c.host_ok = not bad
    while len(c.kpL) < nL or len(c.kpR) < nR:
        kind = rng.random()
        o = int(rng.integers(0, NLEVELS))
        s = float(sf[o])
        lw, lh = int(round(W / s)), int(round(H / s))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        if kind < 0.55:      # a pair that may match: any disparity 0..45, octave difference -2..2, distance 0..110
            x = float(rng.integers(6, lw - 6)) * s
            y = float(rng.integers(6, lh - 6)) * s
            disp = float(rng.choice([DISP, DISP, DISP, rng.integers(0, 46), rng.random() * 45]))
            kl, kr = (x, y, o), (max(x - disp, 0.0), min(max(y + float(rng.integers(-3, 4)) * (rng.random() < 0.3), 0.0), H - 1.0),
                                 int(np.clip(o + rng.choice([0, 0, 0, 1, -1, 2, -2]), 0, NLEVELS - 1)))
            dr = flip_bits(base, int(rng.choice([0, 10, 40, 74, 75, 99, 100, 110, int(rng.integers(0, 111))])), rng)
        elif kind < 0.8:     # unrelated records anywhere in the image, fractional positions
            kl = (rng.random() * (W - 1), rng.random() * (H - 1), o)
            kr = (rng.random() * (W - 1), rng.random() * (H - 1), int(rng.integers(0, NLEVELS)))
            dr = rng.integers(0, 256, 32, dtype=np.uint8)
        else:                # a matching pair a few pixels from an edge of its level: the guards
            edge = int(rng.integers(0, 4))
            xl = [int(rng.integers(0, 12)), lw - 1 - int(rng.integers(0, 14)), int(rng.integers(12, lw - 12)), int(rng.integers(12, lw - 12))][edge]
            yl = [int(rng.integers(6, lh - 6)), int(rng.integers(6, lh - 6)), int(rng.integers(0, 8)), lh - 1 - int(rng.integers(0, 8))][edge]
            x, y = min(xl * s, W - 1.0), min(yl * s, H - 1.0)
            kl, kr = (x, y, o), (max(x - float(rng.integers(0, 9)), 0.0), y, o)
            dr = flip_bits(base, int(rng.integers(0, 20)), rng)
        if len(c.kpL) < nL:
            c.left(*kl, desc=base)
        if len(c.kpR) < nR:
            c.right(*kr, desc=dr)
    if bad:
        poison = [dict(x=0.0, y=0.0, octave=0), dict(x=np.nan, y=50.0, octave=1), dict(x=100.0, y=np.inf, octave=0),
                  dict(x=120.0, y=60.0, octave=9), dict(x=120.0, y=60.0, octave=-3), dict(x=1.0e9, y=60.0, octave=0),
                  dict(x=200.0, y=-40.0, octave=2), dict(x=300.0, y=1.0e6, octave=0)]
        for side in (c.kpL, c.kpR):
            for k in rng.choice(len(side), size=min(len(side), 3), replace=False):
                p = poison[int(rng.integers(1, len(poison)))]
                side[int(k)] = make_kp(p["x"], p["y"], p["octave"])
        side = c.kpL if rng.random() < 0.5 else c.kpR
        side[int(rng.integers(0, len(side)))] = make_kp(np.nan, 50.0, 1)   # at least one record the host form rejects
    return c


def random_cases():
    return [random_case(s) for s in RANDOM_SEEDS]


def image_pair(key):
    return canvas_a() if key[0] == "A" else canvas_cells(key[1])


class Pyramids:
    """oracle pyramids of the image pairs, computed once per key (the pyramid is the extractor's, not the matcher's)"""

    def __init__(self):
        self.o = orc.Oracle(1000, SCALE, NLEVELS, 20, 7)
        self._c = {}

    def get(self, key):
        if key not in self._c:
            left, right = image_pair(key)
            pL = self.o.extract(left, want_pyramid=True)[2]
            pR = self.o.extract(right, want_pyramid=True)[2]
            self._c[key] = (left, right, pL, pR)
        return self._c[key]

    def oracle(self, case: Case):
        _, _, pL, pR = self.get(case.images)
        kL, dL, kR, dR = case.arrays()
        return self.o.stereo(W, H, kL, dL, kR, dR, pL, pR, case.mbf, case.mb)

    def restatement(self, case: Case):
        _, _, pL, pR = self.get(case.images)
        kL, dL, kR, dR = case.arrays()
        return stereo_numpy(self.o.scale_factors(), self.o.inv_scale_factors(), kL, dL, kR, dR,
                            self.o.split_pyramid(pL, W, H), self.o.split_pyramid(pR, W, H), case.mbf, case.mb)
