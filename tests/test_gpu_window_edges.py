"""The engineered and seeded window-search cases of tests/window_edges.py through the kernels of csrc/k_window.hip
(k_grid_build, k_grid_build_count, k_window_search, k_window_search_multi, k_window_claim<>, k_window_claim_init) by every
route that reaches them, array_equal with the CPU oracle.  tests/test_window_edges.py pins the oracle itself to an
independent restatement on the same cases and shows that every named case takes the branch it names."""
import numpy as np
import pytest

import window_edges as we

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def named():
    """every named case with the oracle's answer, computed once (the padded grid forms change no answer:
    test_window_edges.py::test_filler_of_the_grid_forms_is_seen_by_no_named_case)"""
    return [(c, we.run_oracle(c)[0]) for c in we.named_cases()]


def _pad_result(c, ref, n):
    """the oracle's answer of the unpadded case as the padded frame returns it: the filler stays unmatched"""
    if c.kind in ("mappoints", "lastframe", "reloc", "sim3proj"):
        return [ref[0], ref[1] + [-1] * (n - len(ref[1]))]
    return ref


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frame"])
@pytest.mark.parametrize("form", ["sparse", "crowded", "large"])
@pytest.mark.parametrize("kind", we.KINDS)
def test_named_cases_single_call(amd, named, kind, form, resident):
    """sparse: k_grid_build_count's counting path; crowded: its bitonic fallback (70 key points in one cell); large:
    k_grid_build (n > 8192)"""
    n = 0
    for c, ref in named:
        if c.kind != kind:
            continue
        p = we.padded_case(c, form)
        got = we.run_gpu(amd, p, resident)
        assert got == _pad_result(c, ref, len(p.frame["x"])), c.name
        n += 1
    assert n > 0


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frame"])
@pytest.mark.parametrize("kind", we.KINDS)
def test_seeded_cases_single_call(amd, kind, resident):
    for seed in range(200):
        c = we.seeded_case(kind, seed)
        assert we.run_gpu(amd, c, resident) == we.run_oracle(c)[0], c.name


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frame"])
def test_fuse_multi_one_gate_edge_per_job(amd, named, resident):
    """k_window_search_multi: the seven chi-square gate cases (one float below / at / above 5.99 and 7.8, uRight == 0.0f and
    -0.0f on the stereo arm) as the seven key frames of ONE Fuse call -- the same map point, one edge per job"""
    gate = [(c, ref) for c, ref in named if c.name.startswith("gate_")]
    assert len(gate) == 7
    KFs = [we.gpu_frame(amd, c.frame, resident and k != 3) for k, (c, _) in enumerate(gate)]   # (one host-array frame in the group)
    st = lambda key: np.stack([c.args[key] for c, _ in gate])  # noqa: E731
    got = amd.ORBmatcher(0.6).FuseSearchMulti(KFs, we.SF, st("valid"), st("u"), st("v"), st("level"), gate[0][0].args["desc"], th=4.0,
                                              inv_level_sigma2=we.GATE_SIGMA, ur=st("ur"))
    assert [g.tolist() for g in got] == [ref[0] for _, ref in gate]
    assert sorted(r[0][0] for _, r in gate) == [-1, -1, -1, 0, 0, 0, 0]


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frame"])
def test_fuse_multi_seeded(amd, resident):
    """seeded Fuse cases in groups of four key frames: the queries of the first case against all four frames"""
    import oracle_lib as orc
    for s in range(0, 60, 3):
        cs = [we.seeded_case("fuse", s + 3 * k) for k in range(4)]      # (seeds of one residue share bounds and gate setting)
        a = cs[0].args
        nq = len(a["u"])
        KFs = [we.gpu_frame(amd, c.frame, resident) for c in cs]
        rep = lambda v: np.stack([v] * 4)  # noqa: E731
        got = amd.ORBmatcher(0.6).FuseSearchMulti(KFs, we.SF, rep(a["valid"]), rep(a["u"]), rep(a["v"]), rep(a["level"]), a["desc"], th=a["th"],
                                                  inv_level_sigma2=a["inv_sigma2"] if a["chi2"] else None, ur=rep(a["ur"]))
        for k, c in enumerate(cs):
            f = c.frame
            Fo = orc.Frame(f["x"], f["y"], f["octave"], f["desc"], f["bounds"], angle=f["angle"], u_right=f["u_right"])
            ref = orc.fuse_search(Fo, we.SF, a["inv_sigma2"], a["valid"], a["u"], a["v"], a["ur"], a["level"], a["desc"], a["th"], a["chi2"])
            assert got[k].tolist() == ref.tolist(), (s, k, nq)


def _reversed_queries(a):
    b = dict(a)
    for k in ("valid", "u", "v", "level", "angle", "desc"):
        b[k] = np.ascontiguousarray(a[k][::-1])
    return b


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frame"])
def test_keyframe_multi_named_and_seeded(amd, named, resident):
    """k_window_search_multi + k_window_claim<false>: every key-frame (relocalisation) case as candidate 0 and the same points
    in reverse order -- another claim order, another answer -- as candidate 1 of ONE call"""
    import dataclasses
    cases = [c for c, _ in named if c.kind == "reloc"] + [we.seeded_case("reloc", s) for s in range(40)]
    differ = 0
    for c in cases:
        rev = dataclasses.replace(c, args=_reversed_queries(c.args))
        refs = [we.run_oracle(c)[0], we.run_oracle(rev)[0]]
        differ += refs[0] != refs[1]
        cands = [dict(valid=x.args["valid"], u=x.args["u"], v=x.args["v"], level=x.args["level"], kf_angle=x.args["angle"],
                      mp_desc=x.args["desc"], th=x.args["th"], ORBdist=x.args["orb_dist"], blocked=x.args["blocked"]) for x in (c, rev)]
        cnt, got = amd.ORBmatcher(0.9, c.args["check_ori"]).SearchByProjectionKeyFrameMulti(we.gpu_frame(amd, c.frame, resident), we.SF, cands)
        for k in range(2):
            assert [int(cnt[k]), got[k].tolist()] == refs[k], (c.name, k)
    assert differ > 20
