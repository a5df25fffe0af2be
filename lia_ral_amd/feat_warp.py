"""ctypes bindings of include/ext/gmmiv_feat_warp.h: NormFeat's `warp true` on the resident frames.

A module of its own, not part of capi.py: tests/test_cpu_judged_inventory.py and tests/test_cpu_ws_history.py parse capi.py by source
against tables that do not name these two entry points yet (the header's first comment says the same)."""
import ctypes as ct

import numpy as np

from . import capi
from .capi import F32, F64, _chk, _feat_view, _is_torch, _ptr, _vptr, lib

WARP_DEGENERATE = 1    # status of a (unit, column): copied through
WARP_FORCE_SELECT = 1  # flags of warp_hist: every unit through the radix select
WARP_MAX_BINS = 2048
WARP_SORT_CAP = {F32: 32768, F64: 16384}  # values of a unit's column the LDS sort takes

_i64, _int = ct.c_int64, ct.c_int
lib.gmmiv_feat_warp_hist.restype = ct.c_int
lib.gmmiv_feat_warp_hist.argtypes = [ct.c_void_p, ct.c_void_p, _int, _i64, _int, ct.c_void_p, _i64, _i64, _int, _int, ct.c_void_p, ct.c_void_p, ct.c_void_p]
lib.gmmiv_feat_warp_apply.restype = ct.c_int
lib.gmmiv_feat_warp_apply.argtypes = [ct.c_void_p, ct.c_void_p, _int, _i64, ct.c_void_p, _int, _i64, _int, ct.c_void_p, _i64, _i64, _int, ct.c_void_p,
                                      ct.c_void_p, ct.c_void_p, _int, ct.c_void_p, ct.c_void_p]


def _tab(a, dtype):
    if a is None or _is_torch(a):
        return a
    return np.ascontiguousarray(a, dtype)


def read_histo(path):
    """A Histo::save file -> (bounds [nbin + 1], count [nbin]): a line nbin, nbin lines `lowerBound count`, the last upper bound."""
    tok = open(path).read().split()
    nb = int(tok[0])
    if nb < 1 or len(tok) != 2 * nb + 2:
        raise ValueError("%s is not a .histo file: %d tokens for %d bins" % (path, len(tok), nb))
    return (np.array([float(t) for t in tok[1:1 + 2 * nb:2]] + [float(tok[-1])]), np.array([float(t) for t in tok[2:2 + 2 * nb:2]]))


def write_histo(path, bounds, count):
    with open(path, "w") as f:
        f.write("%d\n" % len(count))
        for b, c in zip(bounds[:-1], count):
            f.write("%g\t%g\n" % (b, c))
        f.write("%g\n" % bounds[-1])


def warp_hist(ctx, x, runs, nunits, nbin=40, force_select=False, bounds=None, count=None, status=None):
    """gmmiv_feat_warp_hist on x (a torch device frame matrix, column slices allowed): runs [nrun, 3] int64 (first frame, length, unit),
    host or device -> (bounds [nunits, D, nbin + 1], count [nunits, D, nbin], status [nunits, D] int32): numpy unless torch device arrays
    are passed (with a device run table the call then only enqueues)."""
    x, dt, T, ldx = _feat_view(x)
    D = x.shape[1]
    r = _tab(runs, np.int64)
    nrun = 0 if r is None else r.shape[0]
    if bounds is None:
        bounds = np.zeros((nunits, D, nbin + 1))
    if count is None:
        count = np.zeros((nunits, D, nbin))
    if status is None:
        status = np.zeros((nunits, D), np.int32)
    _chk(lib.gmmiv_feat_warp_hist(ctx._h, _vptr(x), dt, ldx, D, _ptr(r), nrun, nunits, nbin, WARP_FORCE_SELECT if force_select else 0,
                                  _ptr(bounds), _ptr(count), _ptr(status)))
    return bounds, count, status


def warp_apply(ctx, x, runs, nunits, bounds, count, status, tbounds, tcount, out=None):
    """gmmiv_feat_warp_apply: the frames of the runs of x warped onto the target (tbounds [nbin_t + 1], tcount [nbin_t]) through the
    histograms warp_hist returned for the same x and runs; tables host or device.  out=None: in place on x; else a torch device frame
    matrix of any float dtype and stride (frames outside the runs keep what it held).  -> out"""
    x, dt, T, ldx = _feat_view(x)
    D = x.shape[1]
    if out is None:
        out = x
    o, odt, To, ldo = _feat_view(out)
    r = _tab(runs, np.int64)
    nrun = 0 if r is None else r.shape[0]
    b, c, s = _tab(bounds, np.float64), _tab(count, np.float64), _tab(status, np.int32)
    tb, tc = _tab(tbounds, np.float64), _tab(tcount, np.float64)
    nbin = int(c.shape[-1])
    _chk(lib.gmmiv_feat_warp_apply(ctx._h, _vptr(x), dt, ldx, _vptr(o), odt, ldo, D, _ptr(r), nrun, nunits, nbin, _ptr(b), _ptr(c), _ptr(s),
                                   int(tc.shape[0]), _ptr(tb), _ptr(tc)))
    return out


def feat_warp(ctx, x, runs, nunits, tbounds, tcount, nbin=40, out=None, add01=False, add01_runs=None, add01_groups=None):
    """NormFeat `warp true` on resident frames: per unit and column the histogram, then the warp (NormFeat.cpp:362-368, 465-471); with
    add01 (warpAdd01Norm, :475-483) the mean / std normalisation afterwards, by the moments / apply pair the default mode uses.  The
    reference takes those moments over a FILE's selected frames whatever the unit was: in segmentalMode pass the file-wise table as
    add01_runs [., 3] = (first, length, file) with add01_groups files; the default is the units themselves (fileMode).  runs on the
    host.  -> (out, status [nunits, D])"""
    import torch
    D = x.shape[1]
    dev = x.device
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    b = torch.empty((nunits, D, nbin + 1), dtype=torch.float64, device=dev)
    c = torch.empty((nunits, D, nbin), dtype=torch.float64, device=dev)
    s = torch.empty((nunits, D), dtype=torch.int32, device=dev)
    with ctx.ordered():
        warp_hist(ctx, x, r, nunits, nbin, bounds=b, count=c, status=s)
        out = warp_apply(ctx, x, r, nunits, b, c, s, tbounds, tcount, out=out)
        if add01:
            ar = r if add01_runs is None else np.ascontiguousarray(add01_runs, np.int64).reshape(-1, 3)
            ng = nunits if add01_runs is None else int(add01_groups)
            acc = torch.zeros((ng, 2 * D + 1), dtype=torch.float64, device=dev)
            ctx.frame_moments_groups(out, ar, ng, acc)
            mean, std = ctx.frame_moments_stats(acc, D)
            ctx.feat_norm_apply(out, ar, mean, std, out=out)
    return out, s.cpu().numpy()
