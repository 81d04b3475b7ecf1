"""The stereo kernels (k_stereo_bucket / k_stereo_match[_batch] / k_stereo_median_cut, csrc/k_match.hip) on the engineered
and seeded cases of tests/stereo_edges.py: np.array_equal with the CPU oracle on mvuRight and mvDepth, no tolerance, no
case excused.  tests/test_stereo_edges.py (CPU) shows that every case reaches the branch it was built for and that the
oracle agrees with an independent restatement of src/Frame.cc:512-686.

Three ways in: the host-operand call (ComputeStereoMatches), the device-resident batch (stereo_match_batch_device, several
cases per launch so that empty and full frames are neighbours), and extract_stereo_frame (which extracts its own
keypoints, so it runs on the engineered images, not on the hand-placed records).  tests/kernel_variants.py has no
stereo entry and the stereo kernels read no switch, so there is no variant to run them under.

Cases flagged host_ok=False hold records the host-operand call must answer with ORBFE_ERR_INVALID (the classes of
test_compute_stereo_matches_rejects_bad_host_records); the device form answers "no stereo" for them and is compared with
the oracle like every other case."""
import numpy as np
import pytest

import oracle_lib as orc
import stereo_edges as se

pytestmark = pytest.mark.gpu

ENGINEERED = se.engineered_cases()
SEAMS = se.seam_cases()
PAIRS_PER_LAUNCH = 48


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def world():
    """case name -> (case, oracle mvuRight, oracle mvDepth): the reference, computed once and never written to"""
    P = se.Pyramids()
    out = {}
    for c in ENGINEERED + SEAMS + se.random_cases():
        u, d = P.oracle(c)
        u, d = u.copy(), d.copy()
        u.setflags(write=False)
        d.setflags(write=False)
        out[c.name] = (c, u, d)
    out["__pyramids__"] = P
    return out


class _HostForm:
    """one handle for the host-operand call: holds the pair of the image key last asked for as frames 0 / 1"""

    def __init__(self, amd):
        self.amd = amd
        self.e = amd.ORBextractor(1000, se.SCALE, se.NLEVELS, 20, 7)
        self.key = None

    def run(self, case):
        if case.images != self.key:
            left, right = se.image_pair(case.images)
            self.e.extract_batch(np.stack([left, right]))
            self.key = case.images
        kL, dL, kR, dR = case.arrays()
        return self.amd.ComputeStereoMatches(self.e, self.e, kL, dL, kR, dR, case.mbf, case.mb, frameL=0, frameR=1)


@pytest.fixture(scope="module")
def host(amd):
    return _HostForm(amd)


@pytest.fixture(scope="module")
def device_results(amd, world):
    """every case through stereo_match_batch_device, PAIRS_PER_LAUNCH cases per launch in the order engineered, seams
    (n_0, n_1, ... side by side), seeded: name -> (mvuRight[capacity], mvDepth[capacity], n_stereo)"""
    torch = pytest.importorskip("torch")
    e = amd.ORBextractor(1000, se.SCALE, se.NLEVELS, 20, 7)
    cap = e.max_keypoints()
    dev = torch.device("cuda", 0)
    cases = [world[c.name][0] for c in ENGINEERED + SEAMS] + [world[f"random_{s}"][0] for s in se.RANDOM_SEEDS]
    assert max(max(len(c.kpL), len(c.kpR)) for c in cases) <= cap
    images = {}
    out = {}
    for start in range(0, len(cases), PAIRS_PER_LAUNCH):
        chunk = cases[start: start + PAIRS_PER_LAUNCH]
        B = 2 * len(chunk)
        for c in chunk:
            if c.images not in images:
                images[c.images] = se.image_pair(c.images)
        imgs = np.stack([im for c in chunk for im in images[c.images]])
        kp = np.zeros((B, cap, 7), np.float32)
        desc = np.zeros((B, cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        for p, c in enumerate(chunk):
            for side, (k, d) in enumerate(zip(c.arrays()[0::2], c.arrays()[1::2])):
                n[2 * p + side] = len(k)
                if len(k):
                    kp[2 * p + side, :len(k)] = np.ascontiguousarray(k).view(np.float32).reshape(-1, 7)
                    desc[2 * p + side, :len(k)] = d
        mbf = (chunk[0].mbf, chunk[0].mb)
        assert all((c.mbf, c.mb) == mbf for c in chunk)
        d_img = torch.from_numpy(imgs).to(dev)
        d_kp = torch.zeros((B, cap, 7), dtype=torch.float32, device=dev)
        d_desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        d_n = torch.zeros((B,), dtype=torch.int32, device=dev)
        # outputs start as garbage-like values: every slot must be written
        d_u = torch.full((B // 2, cap), 12345.0, dtype=torch.float32, device=dev)
        d_d = torch.full((B // 2, cap), 12345.0, dtype=torch.float32, device=dev)
        d_ns = torch.full((B // 2,), -9, dtype=torch.int32, device=dev)
        e.extract_batch_device(d_img.data_ptr(), B, se.W, se.H, se.W, se.W * se.H, d_kp.data_ptr(), d_desc.data_ptr(), cap,
                               d_n.data_ptr(), wait=True)
        # the handle now holds the pyramids; the records are the cases' own
        d_kp.copy_(torch.from_numpy(kp))
        d_desc.copy_(torch.from_numpy(desc))
        d_n.copy_(torch.from_numpy(n))
        torch.cuda.synchronize()
        e.stereo_match_batch_device(B // 2, d_kp.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap, mbf[0], mbf[1],
                                    d_u.data_ptr(), d_d.data_ptr(), d_ns.data_ptr())
        e.synchronize()
        u, d, ns = d_u.cpu().numpy(), d_d.cpu().numpy(), d_ns.cpu().numpy()
        for p, c in enumerate(chunk):
            out[c.name] = (u[p], d[p], int(ns[p]))
    return out


def _check_host(host, world, name):
    from orb_slam2_annotate_amd import _lib
    c, u_ref, d_ref = world[name]
    if not c.host_ok:
        with pytest.raises(_lib.OrbfeError):
            host.run(c)
        return
    u, d = host.run(c)
    assert u.shape == u_ref.shape and d.shape == d_ref.shape, name
    assert np.array_equal(u_ref, u), (name, np.flatnonzero(u_ref != u)[:8])
    assert np.array_equal(d_ref, d), (name, np.flatnonzero(d_ref != d)[:8])


def _check_device(device_results, world, name):
    c, u_ref, d_ref = world[name]
    u, d, ns = device_results[name]
    N = len(u_ref)
    assert np.array_equal(u_ref, u[:N]), (name, np.flatnonzero(u_ref != u[:N])[:8])
    assert np.array_equal(d_ref, d[:N]), (name, np.flatnonzero(d_ref != d[:N])[:8])
    assert (u[N:] == -1).all() and (d[N:] == -1).all(), name   # slots past the frame's keypoints: "no stereo"
    assert ns == int((u_ref >= 0).sum()), name


@pytest.mark.parametrize("name", [c.name for c in ENGINEERED])
def test_engineered_case_host_operands(host, world, name):
    _check_host(host, world, name)


@pytest.mark.parametrize("name", [c.name for c in ENGINEERED])
def test_engineered_case_device_batch(device_results, world, name):
    _check_device(device_results, world, name)


@pytest.mark.parametrize("name", [c.name for c in SEAMS])
def test_size_seam_host_operands(host, world, name):
    """N = 0, 1, the wavefront's 4 and the workgroup's 16 keypoints +-1, 63 / 64 / 65, the median cut's 256 +-1, Nr = 0,
    N = 0 against 40 right keypoints, and one row band with 53 candidates (the scan takes 16 per pass)"""
    _check_host(host, world, name)


@pytest.mark.parametrize("name", [c.name for c in SEAMS])
def test_size_seam_device_batch(device_results, world, name):
    _check_device(device_results, world, name)


def test_seeded_cases_host_operands(host, world):
    rejected = 0
    for s in se.RANDOM_SEEDS:
        _check_host(host, world, f"random_{s}")
        rejected += not world[f"random_{s}"][0].host_ok
    assert rejected == 50


def test_seeded_cases_device_batch(device_results, world):
    matched = 0
    for s in se.RANDOM_SEEDS:
        _check_device(device_results, world, f"random_{s}")
        matched += device_results[f"random_{s}"][2]
    assert matched > 1000


@pytest.mark.parametrize("name", ["sad_minimum_at_strip_ends", "median_population_150"])
def test_extract_stereo_frame_on_the_engineered_images(amd, world, name):
    """extract_stereo_frame extracts its own keypoints: the engineered IMAGES (V zones, constant and periodic zones; the
    150-cell median canvas) with whatever FAST finds on them, against the oracle's two extractions + stereo matcher"""
    c = world[name][0]
    left, right = se.image_pair(c.images)
    e = amd.ORBextractor(1000, se.SCALE, se.NLEVELS, 20, 7)
    kl, dl, kr, dr, u, d = e.extract_stereo_frame(left, right, se.MBF, se.MB)
    o = orc.Oracle(1000, se.SCALE, se.NLEVELS, 20, 7)
    kL, dL, pL = o.extract(left, want_pyramid=True)
    kR, dR, pR = o.extract(right, want_pyramid=True)
    assert np.array_equal(kL, kl) and np.array_equal(kR, kr) and np.array_equal(dL, dl) and np.array_equal(dR, dr)
    u_ref, d_ref = o.stereo(se.W, se.H, kL, dL, kR, dR, pL, pR, se.MBF, se.MB)
    assert np.array_equal(u_ref, u) and np.array_equal(d_ref, d)
    assert len(kL) > 0 and len(kR) > 0
