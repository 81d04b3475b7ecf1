"""The GPU extractor against the REFERENCE's own src/ORBextractor.cc as recorded in tests/golden/orbextractor_ref.npz
(tests/test_orbextractor_ref.py and tests/ref_lib.py say how that recording is made and checked).  Reads the recording
only.  Where it keeps digests instead of arrays, the arrays are compared with the oracle and the digests with the
recording, so a mismatch can still be located."""
import numpy as np
import pytest

import ref_lib

pytestmark = pytest.mark.gpu

MODES = ("device_octree", "host_octree", "desc_tiles")


@pytest.fixture(scope="module")
def oracle_results():
    return {name: ref_lib.oracle_extract(name) for name in ref_lib.CASE_NAMES}


def _product_tables(e):
    return (e.features_per_level(), e.GetScaleFactors(), e.GetInverseScaleFactors(), e.GetScaleSigmaSquares(),
            e.GetInverseScaleSigmaSquares(), e.umax())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ref_lib.CASE_NAMES)
def test_gpu_extractor_equals_recorded_reference(oracle_results, name, mode):
    import orb_slam2_annotate_amd as amd
    _, _, _, w, h, params, blur = ref_lib.case(name)
    e = amd.ORBextractor(*params)
    e.set_blur_spec(blur)
    if mode == "host_octree":
        e.debug_host_octree(True)
    if mode == "desc_tiles":
        e.set_desc_tiles(True)
    kps, desc = e(ref_lib.case_image(name))
    levels = [e.pyramid_level(l) for l in range(params[2])]
    tables = _product_tables(e)
    for tn, t in zip(ref_lib.TABLE_NAMES, tables):
        assert t.dtype == ref_lib.recorded_case(name)["tab_" + tn].dtype, tn
    if "kps" not in ref_lib.recorded_case(name):  # digests only: locate a mismatch through the oracle first
        okps, odesc, olevels = oracle_results[name]
        assert len(kps) == len(okps) and kps.tobytes() == okps.tobytes()
        assert np.array_equal(desc, odesc)
        for l, (a, b) in enumerate(zip(levels, olevels)):
            assert np.array_equal(a, b), f"pyramid level {l}"
    ref_lib.assert_case_equals_record(name, kps, desc, levels, tables)
