"""The REFERENCE's own code as recorded results.  Test infrastructure only.

DBoW2 FeatureVector / BowVector (Thirdparty/DBoW2/DBoW2/{FeatureVector,BowVector}.cpp): tests/golden/dbow2_ref.npz
holds what the two containers return for every input the tests hand them, keyed by the input's bytes.

ORBextractor (src/ORBextractor.cc compiled untouched against the OpenCV double of oracle/ref_cv/, see
oracle/orbextractor_ref_shim.cpp for what that executes and what stays the oracle's): tests/golden/orbextractor_ref.npz
holds what it returns for CASES and for the candidate sets of octree_sets() -- the second half of this file.

tools/gen_ref_golden.py records both through oracle/_ref/*.so (`make -C oracle ref REF=<reference tree>`: the
sources compiled in place, nothing copied)."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "oracle" / "_ref" / "libdbow2_ref.so"
GOLDEN = ROOT / "tests" / "golden" / "dbow2_ref.npz"
_lib = None
_golden = None
recording = None  # {name: array} while tools/gen_ref_golden.py records: calls go to the library and are kept here


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(SO))
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _recorded(kind, inputs, compute):
    """compute() through the library while recording, else the recorded result for these exact inputs."""
    global _golden
    h = hashlib.sha1(kind.encode())
    for a in inputs:
        h.update(repr((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    key = f"{kind}_{h.hexdigest()[:24]}"
    if recording is not None:
        out = compute()
        for i, a in enumerate(out):
            recording[f"{key}_{i}"] = a
        return out
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = dict(z)
    if f"{key}_0" not in _golden:
        raise KeyError(f"{GOLDEN.name} has no reference result for this input ({key}); regenerate it with tools/gen_ref_golden.py")
    n = sum(1 for k in _golden if k.startswith(key + "_"))
    return tuple(_golden[f"{key}_{i}"] for i in range(n))


def featvec(node_of_feature):
    """(node_ids, offsets, indices) of the reference's FeatureVector after addFeature(node[i], i), i = 0..n-1."""
    nof = np.ascontiguousarray(node_of_feature, dtype=np.uint32)

    def compute():
        n = len(nof)
        nodes = np.zeros(max(n, 1), np.uint32)
        offs = np.zeros(n + 1, np.int32)
        idx = np.zeros(max(n, 1), np.uint32)
        k = lib().ref_featvec_build(_p(nof), n, _p(nodes), _p(offs), _p(idx))
        return nodes[:k].copy(), offs[:k + 1].copy(), idx[:n].copy()

    return _recorded("featvec", [nof], compute)


def bowvec(word, weight, l1_normalize=True):
    word = np.ascontiguousarray(word, dtype=np.uint32)
    weight = np.ascontiguousarray(weight, dtype=np.float64)

    def compute():
        n = len(word)
        ids = np.zeros(max(n, 1), np.uint32)
        val = np.zeros(max(n, 1), np.float64)
        k = lib().ref_bowvec_build(_p(word), _p(weight), n, int(bool(l1_normalize)), _p(ids), _p(val))
        return ids[:k].copy(), val[:k].copy()

    return _recorded("bowvec", [word, weight, np.array([bool(l1_normalize)])], compute)


# ---------------------------------------------------------------------------------------------------------------
# ORBextractor: the reference's src/ORBextractor.cc through oracle/_ref/liborbextractor_ref.so
# ---------------------------------------------------------------------------------------------------------------
REF_TREE = Path(os.environ.get("REF", "/root/reference"))  # as oracle/Makefile's REF
SO_X = ROOT / "oracle" / "_ref" / "liborbextractor_ref.so"
GOLDEN_X = ROOT / "tests" / "golden" / "orbextractor_ref.npz"
FULL_ARRAYS_UP_TO = 320  # keypoints: above it the recording keeps per-level counts and SHA-256 digests only
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
_libx = None
_golden_x = None


def reference_present() -> bool:
    return (REF_TREE / "src" / "ORBextractor.cc").is_file() and (REF_TREE / "include" / "ORBextractor.h").is_file()


def build_ref():
    """`make -C oracle ref` against REF_TREE; raises when the build fails.  Call only when reference_present()."""
    global _libx
    r = subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref", f"REF={REF_TREE}"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"make -C oracle ref failed:\n{r.stdout}\n{r.stderr}")
    if _libx is None:
        _libx = C.CDLL(str(SO_X))
    return _libx


def golden_x():
    global _golden_x
    if _golden_x is None:
        with np.load(GOLDEN_X) as z:
            _golden_x = dict(z)
    return _golden_x


def sha(a) -> np.ndarray:
    """SHA-256 of an array's bytes as 32 uint8 (npz holds numbers only)."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def _textured(seed, w, h):
    from orb_slam2_annotate_amd import synth
    return synth.render_frame(seed, w, h)


def _low_contrast(seed, w, h):
    """the textured scene squeezed to 128 +- 9: no contrast reaches FAST's 20, its corners pass at 7"""
    img = _textured(seed, w, h).astype(np.int32)
    return (128 + ((img - 128) * 9 + 64) // 128).astype(np.uint8)


def _adversarial(kind):
    def gen(seed, w, h):
        from orb_slam2_annotate_amd import synth
        return synth.adversarial(kind, w, h, seed=seed)
    return gen


# (name, image generator, seed, width, height, (nfeatures, scale, levels, iniTh, minTh), blur spec)
CASES = [
    ("smoke_320x240", _textured, 1, 320, 240, (500, 1.2, 8, 20, 7), 0),
    ("workload_640x480", _textured, 2, 640, 480, (1000, 1.2, 8, 20, 7), 0),
    ("odd_333x217", _textured, 3, 333, 217, (300, 1.2, 6, 20, 7), 0),
    ("flat_600x70", _textured, 4, 600, 70, (200, 1.2, 2, 20, 7), 0),
    ("noise_128x96", _adversarial("noise"), 5, 128, 96, (400, 1.3, 3, 20, 7), 0),
    ("lowcontrast_200x150", _low_contrast, 6, 200, 150, (300, 1.2, 4, 20, 7), 0),
    ("checker_160x120", _adversarial("checker"), 0, 160, 120, (300, 1.2, 4, 20, 7), 0),
    ("constant_160x120", _adversarial("constant"), 0, 160, 120, (300, 1.2, 4, 20, 7), 0),
    ("scale2_320x240", _textured, 9, 320, 240, (500, 2.0, 3, 20, 7), 0),
    ("scale105_320x240", _textured, 9, 320, 240, (500, 1.05, 8, 40, 24), 0),
    ("smoke_blur1", _textured, 1, 320, 240, (500, 1.2, 8, 20, 7), 1),
    ("smoke_blur2", _textured, 1, 320, 240, (500, 1.2, 8, 20, 7), 2),
]
CASE_NAMES = [c[0] for c in CASES]


def case(name):
    return CASES[CASE_NAMES.index(name)]


def case_image(name) -> np.ndarray:
    _, gen, seed, w, h, _, _ = case(name)
    img = np.ascontiguousarray(gen(seed, w, h), dtype=np.uint8)
    assert img.shape == (h, w)
    return img


def level_sizes(w, h, params):
    import oracle_lib as orc
    return orc.Oracle(*params).level_sizes(w, h)


def check_domain(w, h, params):
    """The reference computes nCols = width/30, nRows = height/30 (division by zero below one cell) and
    nIni = round(w/h) of the distribution area (0 initial nodes below 0.5) without any check: a case whose top level
    is narrower than 56 px in either direction, or whose distribution area has w/h < 0.5, is OUTSIDE ITS DOMAIN.
    Such a case is refused here rather than recorded as a crash; add none."""
    for lw, lh in level_sizes(w, h, params):
        if lw < 56 or lh < 56:
            raise ValueError(f"level {lw}x{lh} is narrower than 56 px: outside the reference's domain")
        if (lw - 32) / (lh - 32) < 0.5:
            raise ValueError(f"distribution area of level {lw}x{lh} has w/h < 0.5: outside the reference's domain")


def check_octree_domain(minX, maxX, minY, maxY):
    if maxX - minX <= 0 or maxY - minY <= 0 or (maxX - minX) / (maxY - minY) < 0.5:
        raise ValueError("distribution area with w/h < 0.5: outside the reference's domain")


def ref_extract(name, border=0):
    """(keypoint records, descriptors, pyramid levels, FAST statistics) of the reference build for one case.
    border > 0 returns the levels with that many pixels of ComputePyramid's surrounding buffer."""
    L = build_ref()
    _, _, _, w, h, params, blur = case(name)
    check_domain(w, h, params)
    img = case_image(name)
    cap = 4 * params[0] + 256
    kps = np.zeros(cap, KP_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int(0)
    rc = L.ref_extract(int(params[0]), C.c_float(params[1]), int(params[2]), int(params[3]), int(params[4]), _p(img), w, h,
                       img.strides[0], int(blur), _p(kps), _p(desc), cap, C.byref(n))
    assert rc == 0, rc
    levels = []
    for l in range(params[2]):
        lw, lh = C.c_int(0), C.c_int(0)
        assert L.ref_pyramid_level(l, 0, None, 0, C.byref(lw), C.byref(lh)) == 0
        out = np.zeros((lh.value + 2 * border, lw.value + 2 * border), np.uint8)
        assert L.ref_pyramid_level(l, border, _p(out), out.strides[0], C.byref(lw), C.byref(lh)) == 0
        levels.append(out)
    stats = np.zeros(4, np.int32)
    L.ref_fast_stats(_p(stats))
    return kps[:n.value].copy(), desc[:n.value].copy(), levels, stats


def ref_tables(params):
    """(mnFeaturesPerLevel, mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2, umax) of the reference"""
    L = build_ref()
    nl = params[2]
    q, um = np.zeros(nl, np.int32), np.zeros(16, np.int32)
    f = [np.zeros(nl, np.float32) for _ in range(4)]
    got = L.ref_tables(int(params[0]), C.c_float(params[1]), nl, int(params[3]), int(params[4]), _p(q), *[_p(a) for a in f],
                       _p(um))
    assert got == nl
    return (q, *f, um)


def oracle_tables(params):
    import oracle_lib as orc
    o = orc.Oracle(*params)
    return (np.array(o.features_per_level(), np.int32), o.scale_factors(), o.inv_scale_factors(), o.level_sigma2(),
            o.inv_level_sigma2(), np.array(o.umax(), np.int32))


TABLE_NAMES = ("quota", "scale", "inv_scale", "sigma2", "inv_sigma2", "umax")


def oracle_extract(name):
    import oracle_lib as orc
    _, _, _, w, h, params, blur = case(name)
    o = orc.Oracle(*params, blur_spec=blur)
    kps, desc, pyr = o.extract(case_image(name), capacity=4 * params[0] + 256, want_pyramid=True)
    return kps, desc, [np.ascontiguousarray(l) for l in o.split_pyramid(pyr, w, h)]


def case_record(name, kps, desc, levels, tables):
    """what the recording keeps of one case's results ({key: array})"""
    nl = case(name)[5][2]
    rec = {"image_sha": sha(case_image(name)),
           "counts": np.bincount(kps["octave"], minlength=nl).astype(np.int32),
           "kps_sha": sha(kps), "desc_sha": sha(desc),
           "pyr_sha": np.stack([sha(l) for l in levels]),
           "pyr_size": np.array([l.shape[::-1] for l in levels], np.int32)}
    if len(kps) <= FULL_ARRAYS_UP_TO:
        rec["kps"], rec["desc"] = kps, desc
    for tn, t in zip(TABLE_NAMES, tables):
        rec["tab_" + tn] = t
    return {f"{name}/{k}": v for k, v in rec.items()}


def recorded_case(name):
    g = golden_x()
    return {k.split("/", 1)[1]: v for k, v in g.items() if k.startswith(name + "/")}


def assert_case_equals_record(name, kps, desc, levels, tables, rec=None):
    """records, descriptors, every pyramid level and the tables against the recording of the reference's results"""
    rec = recorded_case(name) if rec is None else rec
    assert rec, f"{GOLDEN_X.name} holds no case {name}; regenerate it with tools/gen_ref_golden.py"
    assert np.array_equal(rec["image_sha"], sha(case_image(name))), "the image generator drifted from the recording"
    nl = case(name)[5][2]
    assert np.array_equal(np.bincount(kps["octave"], minlength=nl), rec["counts"])
    if "kps" in rec:
        assert kps.tobytes() == rec["kps"].tobytes()
        assert np.array_equal(desc, rec["desc"].reshape(-1, 32))
    assert np.array_equal(sha(kps), rec["kps_sha"]) and np.array_equal(sha(desc), rec["desc_sha"])
    assert [l.shape[::-1] for l in levels] == [tuple(s) for s in rec["pyr_size"]]
    for l, lev in enumerate(levels):
        assert np.array_equal(sha(lev), rec["pyr_sha"][l]), f"pyramid level {l}"
    for tn, t in zip(TABLE_NAMES, tables):
        assert np.asarray(t).tobytes() == rec["tab_" + tn].tobytes(), tn


# ---- DistributeOctTree on candidate sets: integer coordinates and 8-bit responses (the product's entry) ----
def octree_sets():
    """[(name, xs, ys, responses, minX, maxX, minY, maxY, N)]: 200 seeded random sets, then the engineered ones."""
    sets = []
    areas = [(640, 480), (1241, 376), (300, 100), (333, 217), (200, 150), (2000, 150)]
    for seed in range(200):
        rng = np.random.default_rng([0x0C7EE, seed])
        w, h = areas[seed % len(areas)]
        W, H = w - 32, h - 32
        n = int(rng.integers(1, 500))
        N = int(rng.integers(1, 120))
        if seed % 2:  # clustered: deep splits and many equal counts
            cx, cy = rng.integers(0, W, 5), rng.integers(0, H, 5)
            k = rng.integers(0, 5, n)
            xs = np.clip(cx[k] + rng.integers(-20, 20, n), 0, W - 1)
            ys = np.clip(cy[k] + rng.integers(-20, 20, n), 0, H - 1)
        else:
            xs, ys = rng.integers(0, W, n), rng.integers(0, H, n)
        if seed % 5:  # distinct pixels in raster order, as the FAST grid emits them; every fifth set keeps duplicates
            p = np.unique(np.stack([ys, xs], 1), axis=0)
            ys, xs = p[:, 0], p[:, 1]
        rs = rng.integers(7, 40, len(xs))  # few distinct responses: ties inside nodes
        sets.append((f"random{seed:03d}", xs, ys, rs, 16, w - 16, 16, h - 16, N))

    def add(name, xs, ys, rs, w, h, N):
        xs, ys = np.asarray(xs), np.asarray(ys)
        rs = np.full(len(xs), rs) if np.isscalar(rs) else np.asarray(rs)
        sets.append((name, xs, ys, rs, 16, w - 16, 16, h - 16, N))

    rng = np.random.default_rng(0x0C7EE)
    gx, gy = np.meshgrid(np.arange(3, 600, 11), np.arange(5, 440, 13))
    add("equal_responses", gx.ravel(), gy.ravel(), 20, 640, 480, 150)
    add("coincident_points", np.repeat([10, 10, 300, 301, 590], 4), np.repeat([10, 10, 200, 200, 430], 4),
        [9, 30, 30, 9, 12, 40, 40, 12, 7, 7, 7, 7, 50, 20, 50, 20, 8, 9, 10, 11], 640, 480, 40)
    # area 608 x 448, one root: halfX = 304, halfY = 224, then 152 / 112 ...; points on and next to each line
    lx = np.array([303, 304, 305, 151, 152, 153, 455, 456, 457, 75, 76, 77, 10, 600])
    add("on_split_line_x", np.tile(lx, 3), np.repeat([50, 224, 400], len(lx)), rng.integers(7, 60, 3 * len(lx)), 640, 480, 30)
    ly = np.array([223, 224, 225, 111, 112, 113, 335, 336, 337, 55, 56, 57, 5, 440])
    add("on_split_line_y", np.repeat([100, 304, 500], len(ly)), np.tile(ly, 3), rng.integers(7, 60, 3 * len(ly)), 640, 480, 30)
    xs, ys = rng.integers(0, 608, 900), rng.integers(0, 448, 900)
    for N in (17, 23, 41, 77):  # uniform points: the pass that crosses N has far more nodes to split than N needs
        add(f"early_break_N{N}", xs, ys, rng.integers(7, 200, 900), 640, 480, N)
    add("N_above_points", xs[:60], ys[:60], rng.integers(7, 200, 60), 640, 480, 500)
    add("N_is_1", xs[:300], ys[:300], rng.integers(7, 200, 300), 640, 480, 1)
    add("one_point", [77], [33], [25], 640, 480, 100)
    xs, ys = rng.integers(0, 1241 - 32, 1500), rng.integers(0, 376 - 32, 1500)
    add("kitti_1241x376_nIni4", xs, ys, rng.integers(7, 120, 1500), 1241, 376, 300)  # round(1209 / 344) = 4
    add("kitti_like_nIni3", xs[xs < 1000 - 32], ys[xs < 1000 - 32], rng.integers(7, 120, int((xs < 968).sum())), 1000, 376, 200)
    xs, ys = rng.integers(0, 2000 - 32, 1200), rng.integers(0, 150 - 32, 1200)
    add("wide_nIni17", xs, ys, rng.integers(7, 120, 1200), 2000, 150, 250)
    add("flat_nIni8", xs[xs < 336], ys[xs < 336] % 42, rng.integers(7, 120, int((xs < 336).sum())), 368, 74, 60)
    # 4 x 4 blocks of 3 x 3 points: after two passes 16 nodes of 9 points each, N = 20 ends inside the largest-first pass
    bx, by = np.meshgrid(np.arange(4) * 152 + 60, np.arange(4) * 112 + 40)
    ox, oy = np.meshgrid([0, 9, 18], [0, 9, 18])
    add("equal_sized_nodes", (bx.ravel()[:, None] + ox.ravel()[None, :]).ravel(), (by.ravel()[:, None] + oy.ravel()[None, :]).ravel(),
        rng.integers(7, 200, 144), 640, 480, 20)
    return sets


def ref_octree(xs, ys, rs, minX, maxX, minY, maxY, N, level=0):
    """indices into the input of the keypoints the reference's DistributeOctTree returns, in the order of its result"""
    L = build_ref()
    check_octree_domain(minX, maxX, minY, maxY)
    xs, ys, rs = (np.ascontiguousarray(a, np.float32) for a in (xs, ys, rs))
    out = np.zeros(len(xs) + 8, np.int32)
    k = L.ref_distribute_octtree(_p(xs), _p(ys), _p(rs), len(xs), minX, maxX, minY, maxY, N, level, _p(out), len(out))
    return out[:k].copy()


def octree_inputs_sha(s):
    _, xs, ys, rs, *rest = s
    return sha(np.concatenate([np.asarray(a, np.int64).ravel() for a in (xs, ys, rs, rest)]))


def octree_record(results):
    """{key: array} for the index lists `results` of octree_sets(), in its order"""
    sets = octree_sets()
    assert len(results) == len(sets)
    return {"octree/inputs_sha": np.stack([octree_inputs_sha(s) for s in sets]),
            "octree/count": np.array([len(r) for r in results], np.int32),
            "octree/idx": np.concatenate(results).astype(np.uint16)}


def recorded_octree():
    """the recorded index list of every set of octree_sets(), after checking that the sets are the recorded ones"""
    g = golden_x()
    sets = octree_sets()
    assert np.array_equal(g["octree/inputs_sha"], np.stack([octree_inputs_sha(s) for s in sets])), \
        "the candidate-set generator drifted from the recording"
    ends = np.cumsum(g["octree/count"])
    return [g["octree/idx"][e - c:e].astype(np.int32) for c, e in zip(g["octree/count"], ends)]


# ---- the engineered sets of tests/octree_edges.py: recorded next to the sets above, under keys of their own ----
_edge_sets = None


def octree_edge_sets():
    """octree_edges.edge_sets() at the node-list seam of the built library (its own LDS figures; needs no GPU)"""
    global _edge_sets
    if _edge_sets is None:
        import octree_edges as oe
        from orb_slam2_annotate_amd.extractor import debug_octree_limits
        _edge_sets = oe.edge_sets(oe.largest_lds_quota(lambda N: debug_octree_limits(*oe.AREA, N)))
    return _edge_sets


def octree_edge_sets_in_domain():
    import octree_edges as oe
    return [s for s in octree_edge_sets() if s[0] not in oe.OUT_OF_DOMAIN]


def octree_edges_record(results):
    """{key: array} for the index lists `results` of octree_edge_sets_in_domain(), in its order"""
    sets = octree_edge_sets_in_domain()
    assert len(results) == len(sets)
    return {"octree_edges/inputs_sha": np.stack([octree_inputs_sha(s) for s in sets]),
            "octree_edges/count": np.array([len(r) for r in results], np.int32),
            "octree_edges/idx": np.concatenate(results).astype(np.uint16)}


def recorded_octree_edges():
    """{name: recorded index list} of octree_edge_sets_in_domain(), after checking that the sets are the recorded ones"""
    g = golden_x()
    sets = octree_edge_sets_in_domain()
    assert np.array_equal(g["octree_edges/inputs_sha"], np.stack([octree_inputs_sha(s) for s in sets])), \
        "the engineered sets (or the library's node-list limit) drifted from the recording"
    ends = np.cumsum(g["octree_edges/count"])
    return {s[0]: g["octree_edges/idx"][e - c:e].astype(np.int32) for s, c, e in zip(sets, g["octree_edges/count"], ends)}
