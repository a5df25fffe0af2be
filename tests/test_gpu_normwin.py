"""NormFeat's windowMode on resident frames (include/gmmiv_feat_window.h: gmmiv_plan_norm_windows, gmmiv_feat_norm_window; liagpu::normFeat
with windowMode).

  * bit for bit against the per-step composition of gmmiv_frame_moments_groups (a zeroed accumulator, one group of the window's
    uncut runs), gmmiv_frame_moments_stats, the blend on the host (normwin_ref.blend) and gmmiv_feat_norm_apply, run on a copy;
  * the planner exactly against the restatement of the reference's loop (normwin_ref.plan): offsets, steps, alpha bit for bit;
  * against the long-double restatement under the derived bar of tests/normwin_ref.py (nothing in it is fitted to an output);
  * a file's bits do not depend on the list, on its place in it, or on what the context did before;
  * device tables whose content arrives late on the context's stream;
  * the host layer on the reference's test1.prm.
Worst |difference| / bar measured on an MI355X (profiles/r27/feat_norm_window_errors_gpu.json, rewritten by every run): frames 0.10,
step statistics 0.08, global statistics 0.10.  The bar is derived, not fitted: a ratio above 1 fails the test."""
import itertools
import json
import math
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normwin_ref as nr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFILES = 37
WINDOWS, COMPS, FLAGS = (0.0, 0.05, 0.5, 5.0), (1.0, 0.5), ({}, dict(cms_only=True), dict(var_only=True))
COMBOS = list(itertools.product(WINDOWS, COMPS, FLAGS))            # 24: a shape runs six of them, four consecutive shapes run them all
SHAPES = [(D, pad, f64) for D in (1, 3, 33, 60, 65) for pad in (0, 5) for f64 in (0, 1)]
_STATE = {}


def ctx():
    """one context for the module, on torch's current stream"""
    if "ctx" not in _STATE:
        import torch
        from lia_ral_amd import capi
        _STATE["ctx"] = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    return _STATE["ctx"]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def table():
    """37 files: none and one run, the run lengths 1, 15, 16, 17, 33 and 700, a run of 20 500 frames (a window by itself, whatever the
    duration), then random ones; guard frames between the runs and between the files -> (runs, file_first, T)"""
    if "table" not in _STATE:
        rng = np.random.default_rng(37)
        files = [[], [17], [1, 15, 16, 17, 33, 700], [700, 20500, 33, 16]]
        while len(files) < NFILES:
            files.append([int(v) for v in rng.choice((1, 2, 7, 15, 16, 17, 30, 33, 120), int(rng.integers(0, 13)))])
        runs, first, pos = [], [], 2
        for f, lens in enumerate(files):
            first.append(pos)
            p = pos + (3 if f % 3 == 1 else 0)
            for n in lens:
                runs.append((p, n, f))
                p += n + int(rng.choice((0, 1, 5, 40)))
            pos = p + 2
        _STATE["table"] = (np.array(runs, np.int64), np.array(first, np.int64), pos)
    return _STATE["table"]


def frames(D, f64, pad):
    key = ("x", D, f64, pad)
    if key not in _STATE:
        runs, first, T = table()
        rng = np.random.default_rng(1000 * D + 10 * pad + f64)
        x = np.full((T, D + pad), 1e30, np.float64 if f64 else np.float32)
        drift = np.linspace(0, 2, T)[:, None] * rng.uniform(-1, 1, D)       # a window's statistics differ from the file's
        x[:, :D] = rng.normal(rng.uniform(-3, 3, D), rng.uniform(0.5, 2, D), (T, D)) + drift
        _STATE[key] = x
    return _STATE[key]


def plans(wd, comp):
    key = ("plan", wd, comp)
    if key not in _STATE:
        from lia_ral_amd import capi
        runs, first, T = table()
        _STATE[key] = capi.plan_norm_windows(runs, NFILES, first, wd, comp, 0.01)
    return _STATE[key]


def same_bits(a, b):
    """bit for bit; two NaNs count as equal whatever their payload"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype
    iv = {4: np.int32, 8: np.int64}[a.itemsize]
    return bool(((a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))).all())


def compose(c, xc, D, runs, off, st, al, cms_only=False, var_only=False):
    """the per-step composition of the existing entry points, in place on the device matrix xc[:, :D] -> (gstat, step_stat)"""
    import torch
    view = xc[:, :D]

    def stats(lo, hi):
        g = runs[lo:hi].copy()
        g[:, 2] = 0
        acc = torch.zeros((1, 2 * D + 1), dtype=torch.float64, device="cuda")
        if len(g):
            c.frame_moments_groups(view, g, 1, acc)
        m, s = c.frame_moments_stats(acc, D)
        return m.cpu().numpy()[0], s.cpu().numpy()[0]
    gstat, sstat = np.zeros((NFILES, 2 * D)), np.zeros((len(al), 2 * D))
    for f in range(NFILES):
        idx = np.nonzero(runs[:, 2] == f)[0]
        gm, gs = stats(int(idx[0]), int(idx[-1]) + 1) if len(idx) else stats(0, 0)
        gstat[f] = np.concatenate([gm, gs])
        for s in range(int(off[f]), int(off[f + 1])):
            wlo, whi, alo, ahi = [int(v) for v in st[s]]
            m, sd = stats(wlo, whi)
            mp, sp = nr.blend(m, sd, gm, gs, float(al[s]))
            if cms_only:
                sp = np.ones(D)
            if var_only:
                mp = np.zeros(D)
            sstat[s] = np.concatenate([mp, sp])
            g = runs[alo:ahi].copy()
            g[:, 2] = 0
            c.feat_norm_apply(view, g, mp[None], sp[None], out=view)
    return gstat, sstat


# ---------------------------------------------------------------------------------------------------------------- the planner
def test_the_planner_equals_the_restatement_of_the_loop_on_every_window_and_comp():
    """gmmiv_plan_norm_windows hands back doubles (alpha), so tests/test_cpu_judged_inventory.py lists it as judged, here: the offsets
    and the steps equal those of normwin_ref.plan -- the loop of NormFeat.cpp:384-446 restated on lists -- and alpha has its bits, for
    every (window, comp) the module runs.  Pure host: no device is touched"""
    from lia_ral_amd import capi
    runs, first, T = table()
    seen = 0
    for wd, comp in itertools.product(WINDOWS, COMPS):
        off, st, al = capi.plan_norm_windows(runs, NFILES, first, wd, comp, 0.01)
        woff, wst, wal = nr.plan(runs, NFILES, first, wd, comp, 0.01)
        assert off.dtype == np.int64 and st.dtype == np.int64 and al.dtype == np.float64
        assert off.tolist() == woff.tolist(), (wd, comp)
        assert st.shape == wst.shape and st.tolist() == wst.tolist(), (wd, comp)
        assert al.shape == wal.shape and al.tobytes() == wal.tobytes(), (wd, comp, al[al != wal][:5], wal[al != wal][:5])
        assert np.isfinite(al).all() and (al > 0).all() and (al <= comp).all() and off[-1] == len(al) and off[1] == off[0] == 0
        seen += len(al)
    assert seen > 8 * 37


# ---------------------------------------------------------------------------------------------------------------- bitwise
def _bitwise(x, col0, D, combos):
    import torch
    c = ctx()
    runs, first, T = table()
    rows = np.concatenate([np.arange(b, b + n) for b, n, f in runs])
    guard = np.setdiff1d(np.arange(T), rows)
    cols = np.ones(x.shape[1], bool)
    cols[col0:col0 + D] = False
    steps_seen = 0
    for wd, comp, flags in combos:
        off, st, al = plans(wd, comp)
        xd, xc = dev(x), dev(x)
        gstat, sstat = c.feat_norm_window(xd[:, col0:col0 + D], runs, NFILES, off, st, al, **flags)
        g2, s2 = compose(c, xc[:, col0:], D, runs, off, st, al, **flags)
        torch.cuda.synchronize()
        got, want = xd.cpu().numpy(), xc.cpu().numpy()
        assert same_bits(gstat, g2), (wd, comp, flags)
        assert same_bits(sstat, s2), (wd, comp, flags)
        for f in range(NFILES):                                                      # every file
            r = np.concatenate([np.arange(b, b + n) for b, n, ff in runs if ff == f] or [np.zeros(0, np.int64)])
            assert same_bits(got[r], want[r]), (wd, comp, flags, f)
        assert got[guard].tobytes() == x[guard].tobytes()                            # guard frames between the runs and the files
        assert got[:, cols].tobytes() == x[:, cols].tobytes()                        # columns outside the slice
        assert np.isnan(gstat[0]).all() and off[1] == off[0]                         # the file without runs
        changed = np.any(got[rows][:, col0:col0 + D] != x[rows][:, col0:col0 + D], axis=1)
        assert changed.mean() > 0.9
        steps_seen += len(al)
    assert steps_seen > 100


@pytest.mark.parametrize("k", range(len(SHAPES)), ids=["D%d_pad%d_%s" % (D, p, "f64" if f else "f32") for D, p, f in SHAPES])
def test_every_file_equals_the_per_step_composition_bit_for_bit(k):
    D, pad, f64 = SHAPES[k]
    _bitwise(frames(D, f64, pad), 0, D, COMBOS[k % 4::4])


@pytest.mark.parametrize("f64", [0, 1])
def test_the_energy_column_slice(f64):
    """x + 16, D = 1, ldx = 34: the other 33 columns keep their bytes"""
    _bitwise(frames(34, f64, 0), 16, 1, [COMBOS[i] for i in (3 + 12 * f64, 7, 14, 18 + f64)])


def test_the_long_window_is_there():
    runs, first, T = table()
    off, st, al = plans(5.0, 1.0)
    span = max(int(runs[whi - 1, 0] + runs[whi - 1, 1] - runs[wlo, 0]) for wlo, whi, alo, ahi in st)
    assert span > 20000
    assert sorted(set(runs[runs[:, 2] == 2][:, 1])) == [1, 15, 16, 17, 33, 700] and (runs[:, 2] == 0).sum() == 0 and (runs[:, 2] == 1).sum() == 1


# ---------------------------------------------------------------------------------------------------------------- long double
def test_frames_and_step_statistics_stay_under_the_bar_of_the_long_double_restatement():
    import torch
    c = ctx()
    runs, first, T = table()
    worst = dict(frames=0.0, step_stat=0.0, gstat=0.0)
    D = 3
    rows = np.concatenate([np.arange(b, b + n) for b, n, f in runs])
    for f64 in (0, 1):
        x = frames(D, f64, 0)
        for wd, comp, flags in ((0.5, 1.0, {}), (5.0, 0.5, {}), (5.0, 1.0, dict(cms_only=True)), (0.5, 0.5, dict(var_only=True))):
            off, st, al = plans(wd, comp)
            key = ("ld", f64, wd, comp, tuple(flags))
            if key not in _STATE:
                _STATE[key] = nr.longdouble(x, runs, NFILES, off, st, al, cms=bool(flags.get("cms_only")), var=bool(flags.get("var_only")))
            l = _STATE[key]
            xd = dev(x)
            gstat, sstat = c.feat_norm_window(xd, runs, NFILES, off, st, al, **flags)
            torch.cuda.synchronize()
            got = xd.cpu().numpy()
            # a bar exists wherever the restatement's statistics are usable: not for a window that is one frame (its std is 0)
            fin = np.isfinite(l["bar"][rows]) & np.isfinite(l["out"][rows])
            assert fin.mean() > 0.99
            assert (np.isfinite(got[rows]) | ~fin).all()
            r = dict(frames=nr.worst_ratio(got[rows][fin], l["out"][rows][fin], l["bar"][rows][fin]),
                     step_stat=nr.worst_ratio(sstat, l["step_stat"], l["sbar"]), gstat=nr.worst_ratio(gstat[1:], l["gstat"][1:], l["gbar"][1:]))
            print("f64 %d window %g comp %g %s: %s" % (f64, wd, comp, flags, r))
            for k in worst:
                worst[k] = max(worst[k], r[k])
            sfin = np.isfinite(l["sbar"])
            assert (np.abs(sstat - l["step_stat"])[sfin] <= l["sbar"][sfin]).all()
            assert (np.abs(got[rows].astype(np.float64) - l["out"][rows].astype(np.float64))[fin] <= l["bar"][rows][fin]).all()
    assert max(worst.values()) <= 1.0 and worst["step_stat"] > 0.0, worst
    try:
        os.makedirs(os.path.join(ROOT, "profiles", "r27"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "r27", "feat_norm_window_errors_gpu.json"), "w") as f:
            json.dump(dict(what="gmmiv_feat_norm_window against the long-double restatement: worst |difference| / derived bar (37 files, D = 3, f32 and f64)",
                           worst_ratio=worst), f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass


# ---------------------------------------------------------------------------------------------------------------- independence
def _run(c, x, runs, nfiles, first, wd=0.5, comp=1.0, device_tables=False):
    """-> (frames, gstat, step_stat, step_off) of one call on a fresh copy of x"""
    import torch
    from lia_ral_amd import capi
    off, st, al = capi.plan_norm_windows(runs, nfiles, first, wd, comp, 0.01)
    xd = dev(x)
    D = x.shape[1] - 5
    gstat, sstat = c.feat_norm_window(xd[:, :D], runs, nfiles, off, st, al)
    torch.cuda.synchronize()
    return xd.cpu().numpy(), gstat, sstat, off


def _file_rows(runs, f):
    return np.concatenate([np.arange(b, b + n) for b, n, ff in runs if ff == f] or [np.zeros(0, np.int64)])


def test_a_file_does_not_depend_on_the_list_or_on_the_history_of_the_context():
    import torch
    from lia_ral_amd import capi
    import ws_history as wh
    runs, first, T = table()
    x = frames(33, 0, 5)
    fresh = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    base, g0, s0, off0 = _run(fresh, x, runs, NFILES, first)
    fresh.close()
    c = ctx()
    # the list reversed: file f becomes file 36 - f, the frames stay where they are
    rev = np.concatenate([runs[runs[:, 2] == f] for f in range(NFILES - 1, -1, -1)])
    rev[:, 2] = NFILES - 1 - rev[:, 2]
    got, g1, s1, off1 = _run(c, x, rev, NFILES, first[::-1].copy())
    assert same_bits(got, base) and same_bits(g1[::-1], g0)
    for f in range(NFILES):
        assert same_bits(s1[off1[NFILES - 1 - f]:off1[NFILES - f]], s0[off0[f]:off0[f + 1]]), f
    # a file alone
    for f in (1, 2, 3, 17, 36):
        alone = runs[runs[:, 2] == f].copy()
        alone[:, 2] = 0
        got, g1, s1, off1 = _run(c, x, alone, 1, first[f:f + 1])
        r = _file_rows(runs, f)
        assert same_bits(got[r], base[r]) and same_bits(g1[0], g0[f]) and same_bits(s1, s0[off0[f]:off0[f + 1]]), f
        rest = np.setdiff1d(np.arange(T), r)
        assert got[rest].tobytes() == x[rest].tobytes()
    # a context that has served large NaN-laden calls: every shared workspace slot is dirty (the fresh-context rule of ws_history)
    used = capi.Context(0, torch.cuda.current_stream().cuda_stream)
    assert all(wh.nan_calls(used).values())
    big = np.array([[i * 3000 + k * 300, 290, i] for i in range(40) for k in range(10)], np.int64)   # more runs, steps and columns than the case below
    xb = torch.full((40 * 3000, 70), float("nan"), dtype=torch.float64, device="cuda")
    ob, sb, ab = capi.plan_norm_windows(big, 40, big[::10, 0].copy(), 5.0, 1.0, 0.01)
    assert len(ab) > len(runs)
    gb, stb = used.feat_norm_window(xb, big, 40, ob, sb, np.full(len(ab), np.nan))
    assert np.isnan(gb).all() and np.isnan(stb).all()
    ws_before = used.workspace_bytes()
    got, g1, s1, off1 = _run(used, x, runs, NFILES, first)
    assert used.workspace_bytes() == ws_before                                       # every slot was reused as it was
    assert same_bits(got, base) and same_bits(g1, g0) and same_bits(s1, s0)
    used.close()


def test_device_tables_written_late_on_the_stream():
    """every array a device pointer: the call only enqueues, and reads its inputs in stream order -- they hold poison when the call is
    made and become right behind a spin kernel on the context's stream (the helpers of tests/stream_order.py)"""
    import torch
    from lia_ral_amd import capi
    import stream_order as so
    runs, first, T = table()
    x = frames(33, 0, 5)
    D = 33
    off, st, al = plans(0.5, 1.0)
    c = capi.Context(0)                                                              # a private stream
    be = so.TorchBackend(capi.lib, c)
    true = [dev(x), dev(runs), dev(off), dev(st), dev(al)]
    # the reference: the same call with everything in place
    xr = true[0].clone()
    gr = torch.zeros((NFILES, 2 * D), dtype=torch.float64, device="cuda")
    sr = torch.zeros((len(al), 2 * D), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    c.feat_norm_window(xr[:, :D], true[1], NFILES, true[2], true[3], true[4], gstat=gr, step_stat=sr)
    c.sync()
    live = [t.clone() for t in true]
    gl, sl = torch.full_like(gr, -7.0), torch.full_like(sr, -7.0)
    torch.cuda.synchronize()
    for t, src in zip(live, true):                                                   # poison: -(a) - 1 for the floats, zeros for the tables
        be.write_now(t, so.poison(src))
    be.spin(so.SPIN_CYCLES)
    for t, src in zip(live, true):
        be.enqueue_copy(t, src)
    ev = be.mark()
    assert be.probe(live[4]) == so.poison(true[4]).flatten()[0].item()               # the restoring copies wait behind the spin
    c.feat_norm_window(live[0][:, :D], live[1], NFILES, live[2], live[3], live[4], gstat=gl, step_stat=sl)
    busy = be.busy(ev)
    c.sync()
    torch.cuda.synchronize()
    assert busy, "the call returned after the stream had drained: it did not only enqueue"
    assert same_bits(live[0].cpu().numpy(), xr.cpu().numpy()) and same_bits(gl.cpu().numpy(), gr.cpu().numpy()) and same_bits(sl.cpu().numpy(), sr.cpu().numpy())
    # and the device tables give the bits of the host tables
    base, g0, s0, _ = _run(ctx(), x, runs, NFILES, first)
    assert same_bits(xr.cpu().numpy(), base) and same_bits(gr.cpu().numpy(), g0) and same_bits(sr.cpu().numpy(), s0)
    c.close()


# ---------------------------------------------------------------------------------------------------------------- host layer
def read_prm(path):
    b = open(path, "rb").read()
    h = struct.unpack("<4I", b[:16])
    return h, np.frombuffer(b[16:], np.float32).reshape(h[2], -1)


def time_to_frame(t, fl=0.01):
    """timeToFrameIdx (SegTools.cpp:135-142)"""
    frac, whole = math.modf(t / fl)
    return int(whole) + 1 if frac > 0.99999 else int(whole)


def test_the_host_layer_on_test1_prm(golden_dir, tmp_path):
    from lia_ral_amd import capi, host_capi as h
    hdr, x = read_prm(os.path.join(golden_dir, "ref_files", "test1.prm"))
    lab = [l.split() for l in open(os.path.join(golden_dir, "normwin_test1.lbl")).read().splitlines()]
    cluster = [(time_to_frame(float(b)), time_to_frame(float(e)) - time_to_frame(float(b)) + 1) for b, e, name in lab if name == "speech"]
    assert cluster == [(0, 4), (5, 7), (14, 7), (25, 6), (33, 9), (43, 7)] and x.shape == (50, 34)
    runs = np.array([(b, n, 0) for b, n in cluster], np.int64)
    rows = _file_rows(runs, 0)
    rest = np.setdiff1d(np.arange(50), rows)
    for wd, comp, kw in ((0.1, 1.0, {}), (0.2, 0.5, dict(cms_only=True)), (0.05, 1.0, dict(var_only=True))):
        out = h.norm_feat_window(x, [cluster], window_duration=wd, window_comp=comp, **kw)
        off, st, al = nr.plan(runs, 1, [0], wd, comp, 0.01)                          # the restatement's own schedule
        assert len(al) > 1
        l = nr.longdouble(x, runs, 1, off, st, al, cms=bool(kw.get("cms_only")), var=bool(kw.get("var_only")))
        assert np.isfinite(l["bar"][rows]).all()
        assert (np.abs(out[rows].astype(np.float64) - l["out"][rows].astype(np.float64)) <= l["bar"][rows]).all()
        assert out[rest].tobytes() == x[rest].tobytes()
    # through files, with the file pass behind it
    d = str(tmp_path) + os.sep
    for name, src in (("test1.prm", os.path.join(golden_dir, "ref_files", "test1.prm")), ("test1.lbl", os.path.join(golden_dir, "normwin_test1.lbl"))):
        with open(d + name, "wb") as f:
            f.write(open(src, "rb").read())
    mem = h.norm_feat_window(x, [cluster], window_duration=0.1)
    h.norm_feat_files(["test1"], feature_path=d, save_ext=".win.prm", label_path=d, label="speech", window_mode=True, window_duration=0.1)
    hdr_o, got = read_prm(d + "test1.win.prm")
    assert hdr_o == hdr and got.tobytes() == mem.tobytes()
    both = h.norm_feat_window(x, [cluster], window_duration=0.1, file_mode=True)
    assert both.tobytes() == h.norm_feat(mem, [cluster]).tobytes() and both.tobytes() != mem.tobytes()
    h.norm_feat_files(["test1"], feature_path=d, save_ext=".both.prm", label_path=d, label="speech", window_mode=True, window_duration=0.1, file_mode=True)
    assert read_prm(d + "test1.both.prm")[1].tobytes() == both.tobytes()
    # refusals: segmental with window mode, a cluster out of order (the message names the source / the file)
    with pytest.raises(h.HostError, match="Incompatible modes"):
        h.norm_feat_files(["test1"], feature_path=d, label_path=d, label="speech", window_mode=True, segmental_mode=True)
    with pytest.raises(h.HostError, match="source 0"):
        h.norm_feat_window(x, [[(5, 7), (0, 4)]])
    with pytest.raises(h.HostError, match="source 0"):
        h.norm_feat_window(x, [[(0, 6), (5, 7)]])
    with open(d + "bad.lbl", "w") as f:
        f.write("0.2 0.3 speech\n0 0.1 speech\n")
    with open(d + "bad.prm", "wb") as f:
        f.write(open(d + "test1.prm", "rb").read())
    with pytest.raises(h.HostError, match=r"\[bad\]"):
        h.norm_feat_files(["bad"], feature_path=d, label_path=d, label="speech", window_mode=True)
    # the default mode is what it was: no window keyword, the file pass
    assert h.norm_feat(x, [cluster]).tobytes() != mem.tobytes()
    del capi


# ---------------------------------------------------------------------------------------------------------------- inventory
def test_every_prototype_of_the_header_is_exercised_here_or_is_the_planner():
    from test_cpu_ws_history import binding_calls
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "gmmiv_feat_window.h")).read(), flags=re.S)
    protos = set(re.findall(r"\b(gmmiv_[a-z0-9_]+)\s*\(", hdr))
    assert protos == {"gmmiv_plan_norm_windows", "gmmiv_feat_norm_window"}
    wrappers = {}
    for fn, libs in binding_calls().items():
        for l in libs:
            wrappers.setdefault(l, set()).add(fn)
    me = open(os.path.abspath(__file__)).read()
    for p in protos:
        assert p in wrappers, p
        if p == "gmmiv_plan_norm_windows":
            continue
        assert any(re.search(r"\.%s\(" % w, me) for w in wrappers[p]), p
