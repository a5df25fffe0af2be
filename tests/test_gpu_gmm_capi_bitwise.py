"""The GMM half of the C API on every branch of its host-side dispatch, bit for bit against tests/golden/gmm_capi_bitwise.json
(tools/bitwise_fixture_gmm_capi.py): digests and launch counts written by the library before capi_gmm.hip was split into capi_ctx.hip,
capi_gmm.hip and capi_feat.hip, before gmmiv_llk_determine_top became a dispatcher over three path functions, before the two plans of
gmmiv_tv_stats became functions, and before the per-chunk likelihood stage, the walk head and the ranged output view of
capi_models.hip got one owner each.  None of that may move one bit of any result or one launch count: the kernels, their arguments
and the launch that restarts each kernel timer are the same, and so is their order on the stream (but for the offsets of a chunk's models
in gmmiv_feat_compensate_models, which are now packed after the chunk's likelihood stage, not inside it)."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_the_gmm_entry_points_are_bitwise_the_recorded_results_with_the_recorded_launch_counts(golden_dir):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bitwise_fixture_gmm_capi as bf
    ref = json.load(open(os.path.join(golden_dir, "gmm_capi_bitwise.json")))
    arrs, launches = bf.compute()
    got = bf.digests(arrs)
    assert sorted(ref["arrays"]) == sorted(got)
    assert len(ref["arrays"]) == bf.N_KEYS
    bad = [k for k in ref["arrays"] if got[k] != ref["arrays"][k]]
    assert not bad, bad
    assert sorted(ref["launches"]) == sorted(launches)
    bad = [(k, launches[k], ref["launches"][k]) for k in ref["launches"] if launches[k] != ref["launches"][k]]
    assert not bad, bad
