"""The i-vector half of the C API on every branch of its host-side dispatch, bit for bit against tests/golden/tv_capi_bitwise.json
(tools/bitwise_fixture_tv.py): digests written by the library before the batched SPD work (reserve, zero the status words, packed or
full, factor / solve / invert, read the status back) got one owner, SpdBatch in capi_tv_util.h, before capi_tv.hip was split into
capi_tv.hip, capi_iv_score.hip and capi_backend.hip, and before the host linear algebra moved to host_linalg.cpp.  None of that may
move one bit of any result: the kernels, their arguments and their order on the stream are the same."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_the_tv_scoring_and_back_end_entry_points_are_bitwise_the_recorded_results(golden_dir):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bitwise_fixture_tv as bf
    ref = json.load(open(os.path.join(golden_dir, "tv_capi_bitwise.json")))["arrays"]
    got = bf.digests(bf.compute())
    assert sorted(ref) == sorted(got)
    assert len(ref) == bf.N_KEYS
    bad = [k for k in ref if got[k] != ref[k]]
    assert not bad, bad
