"""NormFeat `warp true` end to end through the host layer: liagpu::normFeatFiles (host_capi.norm_feat_files(warp=True)) on three written
feature files with label files against liagpu::featWarpHost, the host-only twin of the per-unit loop -- fileMode and segmentalMode,
warpAdd01Norm on and off, writeAllFeatures both ways -- the in-memory entry point, and the refusals of NormFeat.cpp:262-264.

Every host-layer call owns a context with a private stream, so this file is collected after the stream-order tests of the older files
(see tests/test_gpu_zz_feat_warp_stream.py).

The warp itself must give the twin's BYTES (both are the fp64 loops of ScoreWarp.cpp:168-206, rounded once to float32).  The 0/1 pass
after it is judged against numpy in fp64 on the twin's frames: the device's mean and std differ from numpy's by summation order
(relative 1e-13 at these lengths), so a normalised value differs by at most one float32 rounding, 2^-23 |v|, plus 1e-10 near zero."""
import math
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from conftest import GOLDEN                     # noqa: E402
from lia_ral_amd import host_capi as h          # noqa: E402

D, NBIN = 12, 40
FRAMES = (900, 1000, 800)
LABELS = (["0 8.99 speech"],
          ["0.1 4.09 speech", "4.5 5 noise", "5 9.49 speech"],
          ["0 2.99 speech", "3.2 4.09 speech", "4.2 4.9 music", "5 6.99 speech"])
_S = {}


def time_to_frame(t, fl=0.01):
    """timeToFrameIdx (SegTools.cpp:135-142)"""
    frac, whole = math.modf(t / fl)
    return int(whole) + 1 if frac > 0.99999 else int(whole)


def clusters():
    out = []
    for lab in LABELS:
        rows = [l.split() for l in lab]
        out.append([(time_to_frame(float(b)), time_to_frame(float(e)) - time_to_frame(float(b)) + 1) for b, e, name in rows if name == "speech"])
    return out


def read_prm(path):
    b = open(path, "rb").read()
    hd = struct.unpack("<4I", b[:16])
    return hd, np.frombuffer(b[16:], np.float32).reshape(hd[2], -1)


def setup(tmp):
    """three .prm / .lbl pairs in tmp -> (names, frames of all files [sum, D], first frame of every file, target)"""
    rng = np.random.default_rng(12)
    d = str(tmp) + os.sep
    xs = []
    for k, (n, lab) in enumerate(zip(FRAMES, LABELS)):
        x = (rng.gamma(2.0 + k, 1.5, (n, D)) - 1).astype(np.float32)            # skewed: the warp has work to do
        xs.append(x)
        with open(d + "f%d.prm" % k, "wb") as f:
            f.write(struct.pack("<4I", 2, D, n, 0) + x.tobytes())
        with open(d + "f%d.lbl" % k, "w") as f:
            f.write("\n".join(lab) + "\n")
    if "t" not in _S:
        _S["t"] = h.read_histo(os.path.join(GOLDEN, "table_gaussN.histo"))
    return d, ["f0", "f1", "f2"], np.concatenate(xs), np.concatenate([[0], np.cumsum(FRAMES)[:-1]]), _S["t"]


def expected(x, first, target, segmental, add01):
    """the twin, then (add01) numpy's 0/1 pass per file -> (frames, bar per value, selected rows per file)"""
    runs, rows = [], []
    for f, c in enumerate(clusters()):
        rows.append(np.concatenate([np.arange(first[f] + b, first[f] + b + n) for b, n in c]))
        runs += [(first[f] + b, n, f) for b, n in c]
    runs = np.array(runs, np.int64)
    if segmental:
        runs[:, 2] = np.arange(len(runs))
    want, st = h.feat_warp_host(x, runs, int(runs[-1, 2]) + 1, target, NBIN)
    assert not st.any()
    bar = np.zeros(want.shape)
    if add01:
        for r in rows:
            v = want[r].astype(np.float64)
            z = (v - v.mean(0)) / v.std(0)
            want[r] = z.astype(np.float32)
            bar[r] = 2.0 ** -23 * np.abs(z) + 1e-10
    return want, bar, rows


@pytest.mark.parametrize("write_all", [True, False])
@pytest.mark.parametrize("add01", [False, True])
@pytest.mark.parametrize("segmental", [False, True])
def test_norm_feat_files_warp_against_the_host_twin(tmp_path, segmental, add01, write_all):
    d, names, x, first, target = setup(tmp_path)
    want, bar, rows = expected(x, first, target, segmental, add01)
    h.norm_feat_files(names, feature_path=d, save_ext=".warp.prm", label_path=d, label="speech", write_all_features=write_all, segmental_mode=segmental,
                      warp=True, warp_bin_count=NBIN, warp_gauss_histo_filename=os.path.join(GOLDEN, "table_gaussN.histo"), warp_add01_norm=add01)
    mem = h.norm_feat_warp(x, clusters(), target, src_first=first, segmental_mode=segmental, warp_bin_count=NBIN, warp_add01_norm=add01)
    for f, n in enumerate(FRAMES):
        hd, got = read_prm(d + "f%d.warp.prm" % f)
        sel = rows[f] if not write_all else np.arange(first[f], first[f] + n)
        assert hd == (2, D, len(sel), 0) and got.shape == (len(sel), D)
        assert got.tobytes() == mem[sel].tobytes()                              # the files hold what the in-memory entry point gives
        if add01:
            err = np.abs(got.astype(np.float64) - want[sel])
            print("file %d: worst |files - numpy| / bar = %.3f" % (f, np.max(err[bar[sel] > 0] / bar[sel][bar[sel] > 0])))
            assert np.all(err <= bar[sel])                                      # unselected frames: bar 0, the input's bytes
        else:
            assert got.tobytes() == want[sel].tobytes()
    other = np.setdiff1d(np.arange(len(x)), np.concatenate(rows))
    assert len(other) and mem[other].tobytes() == x[other].tobytes()            # frames outside the clusters keep their values
    sel = mem[np.concatenate(rows)].astype(np.float64)
    assert abs(sel.mean()) < 0.05 and abs(sel.std() - 1) < 0.06                 # Gaussianised (40 bins squeeze the tails: std 0.96 before the 0/1 pass)


def test_the_refusals_of_the_host_layer(tmp_path):
    d, names, x, first, target = setup(tmp_path)
    histo = os.path.join(GOLDEN, "table_gaussN.histo")
    kw = dict(feature_path=d, label_path=d, label="speech", warp=True, warp_gauss_histo_filename=histo)
    for extra, word in ((dict(cms_only=True), "cmsOnly and warp are not compatible"), (dict(var_only=True), "varOnly and warp are not compatible"),
                        (dict(window_mode=True), "warp with windowMode is not built"), (dict(warp_gauss_histo_filename=""), "rand\\(\\)-made default target"),
                        (dict(warp_bin_count=0), "warpBinCount")):
        with pytest.raises(h.HostError, match=word):
            h.norm_feat_files(names, **dict(kw, **extra))
    with pytest.raises(h.HostError, match="rand\\(\\)-made default target"):
        h.norm_feat_warp(x, clusters(), None, src_first=first)
    with pytest.raises(h.HostError, match="source 1 overlap or are not in increasing order"):
        h.norm_feat_warp(x, [clusters()[0], [(500, 100), (0, 100)], clusters()[2]], target, src_first=first)
    with pytest.raises(h.HostError, match="cannot read"):
        h.norm_feat_warp(x, clusters(), str(tmp_path / "missing.histo"), src_first=first)
    # a target given as a file and as arrays: the same frames
    a = h.norm_feat_warp(x, clusters(), histo, src_first=first)
    b = h.norm_feat_warp(x, clusters(), target, src_first=first)
    assert a.tobytes() == b.tobytes() and a.tobytes() != x.tobytes()
    # a constant column of one file: copied through, its neighbours warped
    xc = x.copy()
    xc[first[1]:first[2], 3] = 1.25
    c = h.norm_feat_warp(xc, clusters(), target, src_first=first)
    assert c[first[1]:first[2], 3].tobytes() == xc[first[1]:first[2], 3].tobytes() and c[:, 4].tobytes() == b[:, 4].tobytes()
