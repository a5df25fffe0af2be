"""The stored-likelihood path (k_llk_mfma in WZ mode and its three readers k_stats_z, k_post_from_z, k_topc_from_z) at boundary
shapes, bit for bit against tests/golden/em_readers_bitwise.json (tools/bitwise_fixture_em.py): digests written by the library
before k_stats_z read x^2 from LDS and before the running exponents were stored four to a 16-byte word.  Neither change may move
one bit of the EM accumulator, the N / F rows, the posterior vectors or the top-C lists."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu


def test_stored_likelihood_readers_are_bitwise_the_recorded_results(golden_dir):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import bitwise_fixture_em as bf
    ref = json.load(open(os.path.join(golden_dir, "em_readers_bitwise.json")))["arrays"]
    got = bf.digests(bf.compute())
    bad = [k for k in ref if got.get(k) != ref[k]]
    assert len(ref) > 100 and sorted(ref) == sorted(got) and not bad, bad
