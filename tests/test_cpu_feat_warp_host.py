"""The host layer of NormFeat `warp true` without a GPU: liagpu::featWarpHost (the host-only twin of the per-unit loop) against the
restatement of tests/warp_ref.py, bit for bit, and the .histo reader and writer of host/io.cpp on the reference's two fixtures."""
import os

import numpy as np

import warp_ref as W
from conftest import GOLDEN

from lia_ral_amd import host_capi as h

HG = os.path.join(GOLDEN, "table_gaussN.histo")
H01 = os.path.join(GOLDEN, "01New.histo")


def test_histo_files_round_trip_through_the_host_layer(tmp_path):
    for path in (H01, HG):
        b, c = h.read_histo(path)
        rb, rc = W.read_histo(path)
        assert np.array_equal(b, rb) and np.array_equal(c, rc)
        out = str(tmp_path / "out.histo")
        h.write_histo(out, b, c)
        assert open(out).read().split() == open(path).read().split()        # token for token: the default ostream precision is the file's
    bad = str(tmp_path / "bad.histo")
    with open(bad, "w") as f:
        f.write("3\n0 1\n1 1\n")
    for path, word in ((bad, "not a histo file"), (str(tmp_path / "none.histo"), "cannot read")):
        try:
            h.read_histo(path)
            raise AssertionError("read_histo accepted %s" % path)
        except h.HostError as e:
            assert word in str(e)


def test_the_host_twin_has_the_restatements_bits():
    tb, tc = W.read_histo(HG)
    rng = np.random.default_rng(0)
    x = (rng.gamma(2.0, 1.5, (1700, 5)) - 1).astype(np.float32)
    x[100:140, 2] = 0.5                     # ties across a bound of unit 0
    x[905, 4] = np.nan
    x[1500, 1] = np.inf
    runs = np.array([(0, 400, 0), (450, 300, 0), (800, 39, 1), (900, 500, 2), (1450, 107, 3)], np.int64)
    for nb in (40, 2, 7):
        got, st = h.feat_warp_host(x, runs, 5, (tb, tc), nb)
        want, _, _, rs = W.warp_units(x, runs, 5, nb, tb, tc)
        assert np.array_equal(st, rs) and st[4].all() and st[2, 4] == 1 and st[3, 1] == 1 and (nb != 40 or st[1].all())
        assert got.tobytes() == want.tobytes()
        rows = np.concatenate([W.unit_rows(runs, u) for u in range(4)])
        assert np.delete(got, rows, 0).tobytes() == np.delete(x, rows, 0).tobytes()
    assert not st[0, 0] and got[:400, 0].tobytes() != x[:400, 0].tobytes()
