"""ctypes binding of host/libliatools_gpu.so -- the C++ mirror of the LIA_SpkTools hot-path drivers
(trainModelStream, ComputeTest's LLR loop, IvExtractor, TotalVariability) over libgmmiv."""
import ctypes as ct
import os

import numpy as np

from . import capi  # noqa: F401  (loads torch's HIP runtime first, then libgmmiv.so)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "host", "libliatools_gpu.so")


class HostError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise HostError("libliatools_gpu.so is not built (%s); run __graft_entry__.build()" % LIB_PATH)
    lib = ct.CDLL(LIB_PATH)
    lib.liagpu_last_error.restype = ct.c_char_p
    return lib


lib = _load()
_dp = ct.POINTER(ct.c_double)
_lp = ct.POINTER(ct.c_long)
_fp = ct.POINTER(ct.c_float)


def _chk(rc):
    if rc != 0:
        raise HostError(lib.liagpu_last_error().decode())


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _segs(seg_begin, seg_len):
    b = np.ascontiguousarray(seg_begin, np.int64); l = np.ascontiguousarray(seg_len, np.int64)
    return b, l, b.ctypes.data_as(_lp), l.ctypes.data_as(_lp)


def train_world(x, seg_begin, seg_len, w, mean, cov, nb_it, bagged_p=1.0, init_floor=0.0, final_floor=0.0,
                init_ceil=10.0, final_ceil=10.0, init_rand=0, device=0):
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w = np.array(w, np.float64); mean = np.array(mean, np.float64); cov = np.array(cov, np.float64)
    C = len(w)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    gm = np.empty(D); gc = np.empty(D); llk = np.empty(nb_it); it_ms = np.empty(nb_it)
    _chk(lib.liagpu_train_world_timed(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, _d(w), _d(mean),
                                      _d(cov), nb_it, ct.c_double(bagged_p), ct.c_double(init_floor), ct.c_double(final_floor),
                                      ct.c_double(init_ceil), ct.c_double(final_ceil), ct.c_long(init_rand), _d(gm), _d(gc), _d(llk), _d(it_ms)))
    return dict(w=w, mean=mean, cov=cov, global_mean=gm, global_cov=gc, llk=llk, it_ms=it_ms)


def train_world_streams(xs, seg_begins, seg_lens, w, mean, cov, nb_it, weights=None, bagged_p=1.0, init_floor=0.0, final_floor=0.0,
                        init_ceil=10.0, final_ceil=10.0, init_rand=0, component_reduction=False, target_distrib_count=0,
                        normalize_model=False, normalize_mean_only=False, normalize_nb_it=1, device=0):
    """TrainWorld over several input streams (liagpu_train_world_streams): xs / seg_begins / seg_lens are lists, one entry per stream."""
    ns = len(xs)
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    D = xs[0].shape[1]
    w = np.array(w, np.float64); mean = np.array(mean, np.float64); cov = np.array(cov, np.float64)
    C = len(w)
    segs = [_segs(b, l) for b, l in zip(seg_begins, seg_lens)]
    xp = (_fp * ns)(*[x.ctypes.data_as(_fp) for x in xs])
    Tp = (ct.c_long * ns)(*[x.shape[0] for x in xs])
    bp = (_lp * ns)(*[s[2] for s in segs]); lp = (_lp * ns)(*[s[3] for s in segs])
    np_ = (ct.c_long * ns)(*[len(s[0]) for s in segs])
    wt = None if weights is None else np.ascontiguousarray(weights, np.float64)
    opts = (ct.c_long * 5)(int(component_reduction), int(target_distrib_count), int(normalize_model), int(normalize_mean_only), int(normalize_nb_it))
    gm = np.empty(D); gc = np.empty(D); llk = np.empty(nb_it); cout = ct.c_long(0)
    _chk(lib.liagpu_train_world_streams(device, ns, xp, Tp, D, bp, lp, np_, _d(wt), C, _d(w), _d(mean), _d(cov), nb_it, ct.c_double(bagged_p),
                                        ct.c_double(init_floor), ct.c_double(final_floor), ct.c_double(init_ceil), ct.c_double(final_ceil),
                                        ct.c_long(init_rand), opts, ct.byref(cout), _d(gm), _d(gc), _d(llk)))
    Co = cout.value
    return dict(w=w[:Co].copy(), mean=mean[:Co].copy(), cov=cov[:Co].copy(), global_mean=gm, global_cov=gc, llk=llk)


def mixture_init_streams(xs, seg_begins, seg_lens, C, global_cov, weights=None, nb_frame_to_select=50.0, min_len=3, max_len=7, device=0):
    """mixtureInit over several input streams (liagpu_mixture_init_streams) -> dict(w, mean, cov, counts)."""
    ns = len(xs)
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    D = xs[0].shape[1]
    segs = [_segs(b, l) for b, l in zip(seg_begins, seg_lens)]
    xp = (_fp * ns)(*[x.ctypes.data_as(_fp) for x in xs])
    Tp = (ct.c_long * ns)(*[x.shape[0] for x in xs])
    bp = (_lp * ns)(*[s[2] for s in segs]); lp = (_lp * ns)(*[s[3] for s in segs])
    np_ = (ct.c_long * ns)(*[len(s[0]) for s in segs])
    wt = None if weights is None else np.ascontiguousarray(weights, np.float64)
    gc = np.ascontiguousarray(global_cov, np.float64)
    w = np.empty(C); mean = np.empty((C, D)); cov = np.empty((C, D)); cnt = np.zeros(C, np.int64)
    _chk(lib.liagpu_mixture_init_streams(device, ns, xp, Tp, D, bp, lp, np_, _d(wt), C, _d(gc), ct.c_double(nb_frame_to_select), ct.c_long(min_len),
                                         ct.c_long(max_len), _d(w), _d(mean), _d(cov), cnt.ctypes.data_as(_lp)))
    return dict(w=w, mean=mean, cov=cov, counts=cnt)


def model_reduce_normalize(w, mean, cov, nb_top=0, normalize=False, mean_only=False, nb_it=1):
    """selectComponent(nbTop) + reduceModel + normalizeWeights, then normalizeMixture to N(0,1) (TrainTools.cpp:1078-1098); host only.
    Returns (w, mean, cov, order) with order = TabWeight's heaviest-first component order of the INPUT model."""
    w = np.array(w, np.float64); mean = np.array(mean, np.float64); cov = np.array(cov, np.float64)
    C, D = mean.shape
    order = np.empty(C, np.int64)
    _chk(lib.liagpu_model_reduce_normalize(C, D, _d(w), _d(mean), _d(cov), ct.c_long(nb_top), int(normalize), int(mean_only), ct.c_long(nb_it),
                                           order.ctypes.data_as(_lp)))
    Co = nb_top if 0 < nb_top < C else C
    return w[:Co].copy(), mean[:Co].copy(), cov[:Co].copy(), order


def train_world_scratch(x, seg_begin, seg_len, C, nb_it, nb_frame_to_select=50.0, use01=False, bagged_p=1.0, init_floor=0.0, final_floor=0.0,
                        init_ceil=10.0, final_ceil=10.0, init_rand=0, device=0):
    """TrainWorld with no initial model: computeMeanCov (or use01), mixtureInit, trainModelStream (liagpu_train_world_scratch)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    b, l, bp, lp = _segs(seg_begin, seg_len)
    w = np.empty(C); mean = np.empty((C, D)); cov = np.empty((C, D)); gc = np.empty(D); llk = np.empty(nb_it)
    _chk(lib.liagpu_train_world_scratch(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, ct.c_double(nb_frame_to_select),
                                        int(use01), _d(w), _d(mean), _d(cov), nb_it, ct.c_double(bagged_p), ct.c_double(init_floor),
                                        ct.c_double(final_floor), ct.c_double(init_ceil), ct.c_double(final_ceil), ct.c_long(init_rand), _d(gc), _d(llk)))
    return dict(w=w, mean=mean, cov=cov, global_cov=gc, llk=llk)


def mixture_init(x, seg_begin, seg_len, C, global_cov, nb_frame_to_select=50.0, stream_weight=1.0, single_stream_proba=None, min_len=3,
                 max_len=7, device=0):
    """mixtureInit: TrainWorld's start-from-scratch model (multi-stream form with one stream; single_stream_proba = the
    baggedFrameProbabilityInit of the single-stream form).  Returns dict(w, mean, cov, counts)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    b, l, bp, lp = _segs(seg_begin, seg_len)
    gc = np.ascontiguousarray(global_cov, np.float64)
    w = np.empty(C); mean = np.empty((C, D)); cov = np.empty((C, D)); cnt = np.zeros(C, np.int64)
    single = single_stream_proba is not None
    _chk(lib.liagpu_mixture_init(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, int(single),
                                 ct.c_double(single_stream_proba if single else nb_frame_to_select), ct.c_double(stream_weight),
                                 ct.c_long(min_len), ct.c_long(max_len), _d(gc), _d(w), _d(mean), _d(cov), cnt.ctypes.data_as(_lp)))
    return dict(w=w, mean=mean, cov=cov, counts=cnt)


def tv_verify_emlk(x, file_begin, row_of_file, ubm, Tmat, W, max_llk_computed=None, min_llk=-200.0, max_llk=200.0, device=0):
    """TVAcc::verifyEMLK: per-file mean log-likelihood under the speaker model m + T^T w_row; returns (llk [nfiles], total, supervectors)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C = len(w)
    fb = np.ascontiguousarray(file_begin, np.int64); rows = np.ascontiguousarray(row_of_file, np.int64)
    nf = len(fb) - 1
    Tm = np.ascontiguousarray(Tmat, np.float64); Wm = np.ascontiguousarray(W, np.float64)
    n = nf if max_llk_computed is None else min(nf, max_llk_computed)
    llk = np.zeros(nf); total = ct.c_double(0.0); sv = np.empty((nf, C * D))
    _chk(lib.liagpu_tv_verify_emlk(device, x.ctypes.data_as(_fp), ct.c_long(T), D, fb.ctypes.data_as(_lp), ct.c_long(nf), rows.ctypes.data_as(_lp),
                                   C, _d(w), _d(mean), _d(cov), Tm.shape[0], _d(Tm), ct.c_long(Wm.shape[0]), _d(Wm), ct.c_long(n),
                                   ct.c_double(min_llk), ct.c_double(max_llk), _d(llk), ct.byref(total), _d(sv)))
    return llk[:n], total.value, sv


def mean_llk(x, seg_begin, seg_len, model, min_llk=-200.0, max_llk=200.0, device=0):
    """accumulateStatLLK: mean clamped log-likelihood of the selected frames."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in model]
    b, l, bp, lp = _segs(seg_begin, seg_len)
    out = ct.c_double(0.0)
    _chk(lib.liagpu_mean_llk(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), len(w), _d(w), _d(mean), _d(cov),
                             ct.c_double(min_llk), ct.c_double(max_llk), ct.byref(out)))
    return out.value


def mean_llk_streams(xs, seg_begins, seg_lens, model, decision=None, min_llk=-200.0, max_llk=200.0, device=0):
    """meanLikelihood over several feature servers, optionally weighted by one decision value per server (GeneralTools.cpp:599-624)."""
    ns = len(xs)
    xs = [np.ascontiguousarray(x, np.float32) for x in xs]
    D = xs[0].shape[1]
    w, m, c = [np.ascontiguousarray(a, np.float64) for a in model]
    segs = [_segs(b, l) for b, l in zip(seg_begins, seg_lens)]
    xp = (_fp * ns)(*[x.ctypes.data_as(_fp) for x in xs])
    Tp = (ct.c_long * ns)(*[x.shape[0] for x in xs])
    bp = (_lp * ns)(*[s[2] for s in segs]); lp = (_lp * ns)(*[s[3] for s in segs])
    np_ = (ct.c_long * ns)(*[len(s[0]) for s in segs])
    dec = None if decision is None else np.ascontiguousarray(decision, np.float64)
    out = ct.c_double(0.0)
    _chk(lib.liagpu_mean_llk_streams(device, ns, xp, Tp, D, bp, lp, np_, _d(dec), len(w), _d(w), _d(m), _d(c), ct.c_double(min_llk),
                                     ct.c_double(max_llk), ct.byref(out)))
    return out.value


def train_target(x, seg_begin, seg_len, world, nb_it=1, mean_reg=16.0, device=0):
    """TrainTarget: mean-only MAPOccDep adaptation of the world model; returns (w, mean, cov)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in world]
    C = len(w)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    wo = np.empty(C); mo = np.empty((C, D)); co = np.empty((C, D))
    _chk(lib.liagpu_train_target(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, _d(w), _d(mean),
                                 _d(cov), nb_it, ct.c_double(mean_reg), _d(wo), _d(mo), _d(co)))
    return wo, mo, co


def _map_flags(mean, var, weight, batch_variances=False):
    return int(mean) | (int(var) << 1) | (int(weight) << 2) | (int(batch_variances) << 3)


def train_target_ex(x, seg_begin, seg_len, world, method="MAPOccDep", nb_it=1, bagged_p=1.0, mean=True, var=False, weight=False,
                    reg=(16.0, 16.0, 16.0), alpha_mean=0.75, normalize=False, normalize_mean_only=False, normalize_nb_it=1, device=0):
    """TrainTarget (adaptModel, TrainTools.cpp:871-904) with every MAPCfg parameter -> (w, mean, cov)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, m, c = [np.ascontiguousarray(a, np.float64) for a in world]
    C = len(w)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    r = np.ascontiguousarray(reg, np.float64)
    norm = (ct.c_long * 3)(int(normalize), int(normalize_mean_only), int(normalize_nb_it))
    wo = np.empty(C); mo = np.empty((C, D)); co = np.empty((C, D))
    _chk(lib.liagpu_train_target_ex(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, _d(w), _d(m), _d(c), method.encode(),
                                    nb_it, ct.c_double(bagged_p), _map_flags(mean, var, weight), _d(r), ct.c_double(alpha_mean), norm, _d(wo), _d(mo), _d(co)))
    return wo, mo, co


def train_target_batch(x, client_begin, seg_begin, seg_len, world, method="MAPOccDep", nb_it=1, bagged_p=1.0, mean=True, var=False, weight=False,
                       reg=(16.0, 16.0, 16.0), alpha_mean=0.75, normalize=False, normalize_mean_only=False, normalize_nb_it=1, device=0,
                       return_mllr=False, batch_variances=False):
    """TrainTarget for many clients at once (adaptModelBatch): client i owns the segments client_begin[i] .. client_begin[i + 1] of the
    seg_begin / seg_len lists and starts from `world` -> (w [G, C], mean [G, C, D], cov [G, C, D]); row i is what train_target_ex gives
    for client i when the clients are adapted one after the other in this order (var / normalize: it runs exactly that loop, unless
    batch_variances=True -- MAPCfg::batchVariances -- which keeps those configurations on the device too: second-order statistics per client,
    the variance branch of computeMAP and normalizeMixture as kernels).
    method="MLLR": one global affine transform of the world means per client (computeMLLR); return_mllr=True appends the last
    iteration's transforms W [G, D, D + 1] to the result."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, m, c = [np.ascontiguousarray(a, np.float64) for a in world]
    C = len(w)
    cb = np.ascontiguousarray(client_begin, np.int64); b = np.ascontiguousarray(seg_begin, np.int64); l = np.ascontiguousarray(seg_len, np.int64)
    G = len(cb) - 1
    assert len(b) == len(l) and cb[0] == 0 and cb[-1] == len(b)
    lp = lambda a: a.ctypes.data_as(ct.POINTER(ct.c_long))
    r = np.ascontiguousarray(reg, np.float64)
    norm = (ct.c_long * 3)(int(normalize), int(normalize_mean_only), int(normalize_nb_it))
    wo = np.empty((G, C)); mo = np.empty((G, C, D)); co = np.empty((G, C, D))
    Wm = np.zeros((G, D, D + 1)) if return_mllr else None
    _chk(lib.liagpu_train_target_batch_w(device, x.ctypes.data_as(_fp), ct.c_long(T), D, lp(cb), ct.c_long(G), lp(b), lp(l), C, _d(w), _d(m), _d(c),
                                         method.encode(), nb_it, ct.c_double(bagged_p), _map_flags(mean, var, weight, batch_variances), _d(r),
                                         ct.c_double(alpha_mean), norm, _d(wo), _d(mo), _d(co), _d(Wm)))
    return (wo, mo, co, Wm) if return_mllr else (wo, mo, co)


def compute_map(method, init, client, frame_count, mean=True, var=False, weight=False, reg=(16.0, 16.0, 16.0), alpha_mean=0.75):
    """computeMAP (TrainTools.cpp:543-556) on its own, host arithmetic only: init / client = (w, mean, cov) -> adapted (w, mean, cov)."""
    w0, m0, c0 = [np.ascontiguousarray(a, np.float64) for a in init]
    w, m, c = [np.array(a, np.float64, order="C", copy=True) for a in client]
    C, D = m0.shape
    r = np.ascontiguousarray(reg, np.float64)
    _chk(lib.liagpu_compute_map(C, D, _d(w0), _d(m0), _d(c0), _d(w), _d(m), _d(c), ct.c_double(frame_count), method.encode(),
                                _map_flags(mean, var, weight), _d(r), ct.c_double(alpha_mean)))
    return w, m, c


def compute_mllr(init, client, frame_count, return_covinv=False):
    """computeMLLR (TrainTools.cpp:788-866) on its own, host arithmetic only: init = (w, mean, cov) of the a-priori model, client =
    (w, mean[, cov]) the ML estimate -> (W [D, D + 1], (w, mean, cov)) with the adapted means and the a-priori weights and variances;
    return_covinv=True appends the covInv the model holds after its computeAll()."""
    w0, m0, c0 = [np.ascontiguousarray(a, np.float64) for a in init[:3]]
    w, m = [np.array(a, np.float64, order="C", copy=True) for a in client[:2]]
    C, D = m0.shape
    c = np.empty((C, D)); ci = np.empty((C, D)); W = np.empty((D, D + 1))
    _chk(lib.liagpu_compute_mllr(C, D, _d(w0), _d(m0), _d(c0), _d(w), _d(m), _d(c), _d(ci), ct.c_double(frame_count), _d(W)))
    return (W, (w, m, c), ci) if return_covinv else (W, (w, m, c))


def topgauss(x, seg_begin, seg_len, ubm, top_gauss, path, top_distribs_count=64, model2_mean=None, complete=True, min_llk=-200.0,
             max_llk=200.0, device=0):
    """TopGauss::compute -> write(path) -> read(path) -> get (liagpu_topgauss).  Returns dict(llk_compute, llk_get, llk_get_model2,
    capped, nbg [T], idx (flat), snsw, snsl)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C = len(w)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    n = int(l.sum())
    cap = min(top_distribs_count, C)
    out = np.zeros(4); cnt = np.zeros(n, np.int64); idx = np.zeros(n * cap, np.int64); sw = np.zeros(n); sl = np.zeros(n); tot = ct.c_long(0)
    m2 = None if model2_mean is None else np.ascontiguousarray(model2_mean, np.float64)
    _chk(lib.liagpu_topgauss(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, _d(w), _d(mean), _d(cov), _d(m2),
                             ct.c_double(top_gauss), int(top_distribs_count), int(complete), ct.c_double(min_llk), ct.c_double(max_llk),
                             path.encode(), _d(out), cnt.ctypes.data_as(_lp), idx.ctypes.data_as(_lp), _d(sw), _d(sl), ct.byref(tot)))
    return dict(llk_compute=out[0], llk_get=out[1], llk_get_model2=out[2], capped=int(out[3]), nbg=cnt, idx=idx[:tot.value].copy(), snsw=sw, snsl=sl)


def compute_test(x, seg_begin, seg_len, world, clients, top_c=10, complete=True, min_llk=-200.0, max_llk=200.0,
                 segmental=False, device=0, reps=0):
    """world = (w, mean, cov); clients = list of (w, mean, cov).  Returns LLR[n_seg_or_1, n_clients]; with reps > 0 the LLR loop
    is run that many times on the resident features and (llr, ms[reps]) is returned."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    ww, mw, cw = [np.ascontiguousarray(a, np.float64) for a in world]
    C = len(ww)
    wc = np.ascontiguousarray(np.stack([c[0] for c in clients]), np.float64)
    mc = np.ascontiguousarray(np.stack([c[1] for c in clients]), np.float64)
    cc = np.ascontiguousarray(np.stack([c[2] for c in clients]), np.float64)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    nout = (len(b) if segmental else 1) * len(clients)
    out = np.empty(nout)
    ms = np.zeros(max(reps, 1))
    _chk(lib.liagpu_compute_test_timed(device, x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)), C, _d(ww), _d(mw),
                                       _d(cw), len(clients), _d(wc), _d(mc), _d(cc), top_c, int(complete), ct.c_double(min_llk),
                                       ct.c_double(max_llk), int(segmental), _d(out), max(reps, 1), _d(ms)))
    out = out.reshape(-1, len(clients))
    return (out, ms) if reps > 0 else out


def compute_test_ex(x, seg_begin, seg_len, world, clients, top_c=10, complete=True, min_llk=-200.0, max_llk=200.0, segmental=False,
                    world_decime=1, window_size=0, window_dec=0, device=0):
    """ComputeTest frame loop with worldDecime and the WindowLLR mode.  -> (llr [nseg or 1, nClients], windows [n, 2 + nClients])."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    sb = np.ascontiguousarray(seg_begin, np.int64); sl = np.ascontiguousarray(seg_len, np.int64)
    ww, wm, wc = [np.ascontiguousarray(a, np.float64) for a in world]
    C = len(ww)
    cw = np.ascontiguousarray(np.stack([c[0] for c in clients]), np.float64)
    cm = np.ascontiguousarray(np.stack([c[1] for c in clients]), np.float64)
    cc = np.ascontiguousarray(np.stack([c[2] for c in clients]), np.float64)
    nC = len(clients)
    nseg = len(sb) if segmental else 1
    out = np.empty((nseg, nC))
    max_win = int(sl.sum()) + 1
    win = np.zeros((max_win, 2 + nC)); nw = ct.c_long(0)
    _chk(lib.liagpu_compute_test_ex(device, x.ctypes.data_as(_fp), ct.c_long(T), D, sb.ctypes.data_as(_lp), sl.ctypes.data_as(_lp),
                                    ct.c_long(len(sb)), C, _d(ww), _d(wm), _d(wc), nC, _d(cw), _d(cm), _d(cc), top_c, int(complete),
                                    ct.c_double(min_llk), ct.c_double(max_llk), int(segmental), ct.c_long(world_decime),
                                    ct.c_long(window_size), ct.c_long(window_dec), _d(out), _d(win), ct.c_long(max_win), ct.byref(nw)))
    return out, win[:nw.value]


def iv_extract(x, utt_begin, ubm, Tmat, device=0, return_stats=False, reps=0):
    """IvExtractor.  reps > 0: the extraction is run that many times on the resident features; the wall times
    ms[reps, 4] = (statistics, substractM, estimateTETt [first run only], estimateW) are appended to the result."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C = len(w)
    Tm = np.ascontiguousarray(Tmat, np.float64)
    R = Tm.shape[0]
    ub = np.ascontiguousarray(utt_begin, np.int64)
    U = len(ub) - 1
    W = np.empty((U, R))
    N = np.empty((U, C)) if return_stats else None
    F = np.empty((U, C * D)) if return_stats else None
    ms = np.zeros((max(reps, 1), 4))
    _chk(lib.liagpu_iv_extract_timed(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ub.ctypes.data_as(_lp), ct.c_long(U), C, _d(w),
                                     _d(mean), _d(cov), R, _d(Tm), _d(W), _d(N), _d(F), max(reps, 1), _d(ms)))
    res = (W, N, F) if return_stats else W
    if reps > 0:
        return res + (ms,) if return_stats else (W, ms)
    return res


def iv_extract_approx(x, utt_begin, ubm, Tmat, mode, device=0):
    """IvExtractor --mode ubmWeight (mode=1) / eigenDecomposition (mode=2).  -> dict(W, Wcov, Q, D)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C = len(w)
    Tm = np.ascontiguousarray(Tmat, np.float64)
    R = Tm.shape[0]
    ub = np.ascontiguousarray(utt_begin, np.int64)
    U = len(ub) - 1
    W = np.empty((U, R)); Wc = np.empty((R, R)); Q = np.zeros((R, R)); Dm = np.zeros((C, R))
    _chk(lib.liagpu_iv_extract_approx(device, int(mode), x.ctypes.data_as(_fp), ct.c_long(T), D, ub.ctypes.data_as(_lp), ct.c_long(U), C,
                                      _d(w), _d(mean), _d(cov), R, _d(Tm), _d(W), _d(Wc), _d(Q), _d(Dm)))
    return dict(W=W, Wcov=Wc, Q=Q, D=Dm)


def backend_train(X, sps, nb_it=2, sph_norm=False, lda_rank=0, device=0):
    """PldaDev EFR / sphNorm training (+ WCCN, Mahalanobis, LDA on the normalised set). X[dim, n] -> dict."""
    X = np.array(X, np.float64, order="C", copy=True)
    dim, n = X.shape
    sps = np.ascontiguousarray(sps, np.int64)
    mats = np.empty((nb_it, dim, dim)); means = np.empty((nb_it, dim)); wccn = np.empty((dim, dim)); mah = np.empty((dim, dim))
    lda = np.empty((max(lda_rank, 1), dim))
    _chk(lib.liagpu_backend_train(device, dim, ct.c_long(n), _d(X), ct.c_long(len(sps)), sps.ctypes.data_as(_lp), int(sph_norm), nb_it,
                                  _d(mats), _d(means), _d(wccn), _d(mah), lda_rank, _d(lda)))
    return dict(X=X, mats=mats, means=means, wccn=wccn, mahalanobis=mah, lda=lda[:lda_rank])


def plda_train(X, sps, F, G, Sigma, nb_it, device=0):
    """PLDA.cpp training loop: nb_it x PldaModel::em_iteration.  -> dict(X, F, G, Sigma, Delta, original_mean)."""
    X = np.array(X, np.float64, order="C", copy=True); F = np.array(F, np.float64, order="C", copy=True)
    G = np.array(G, np.float64, order="C", copy=True); Sigma = np.array(Sigma, np.float64, order="C", copy=True)
    dim, n = X.shape
    sps = np.ascontiguousarray(sps, np.int64)
    Delta = np.zeros(dim); om = np.zeros(dim)
    _chk(lib.liagpu_plda_train(device, dim, ct.c_long(n), _d(X), ct.c_long(len(sps)), sps.ctypes.data_as(_lp), F.shape[1], G.shape[1], nb_it,
                               _d(F), _d(G), _d(Sigma), _d(Delta), _d(om)))
    return dict(X=X, F=F, G=G, Sigma=Sigma, Delta=Delta, original_mean=om)


_SCORING = {"cosine": 0, "mahalanobis": 1, "2cov": 2, "plda": 3}
_PLDA_SCORING = {"native": 0, "enrollMean": 1}


def _iv_test_cfg(scoring, iv_norm, iv_norm_it, sph_norm, lda_rank, wccn, plda, plda_it, plda_scoring):
    """-> (the configuration arguments shared by the IvTest exports, the arrays they point to)"""
    if plda_scoring not in _PLDA_SCORING:
        raise HostError("pldaScoring must be: native OR enrollMean")
    if plda is not None:
        F, G, S = [np.ascontiguousarray(a, np.float64) for a in plda]
        rf, rg = F.shape[1], G.shape[1]
    else:
        F = G = S = np.zeros(1); rf = rg = 0
    args = (int(iv_norm), int(iv_norm_it), int(sph_norm), int(lda_rank > 0), int(lda_rank), int(wccn), _SCORING[scoring], rf, rg, int(plda_it),
            _d(F), _d(G), _d(S), _PLDA_SCORING[plda_scoring])
    return args, (F, G, S)


def iv_test(dev, sps, enrol, enrol_per_model, test, scoring="cosine", iv_norm=False, iv_norm_it=1, sph_norm=False, lda_rank=0,
            wccn=False, plda=None, plda_it=0, device=0, plda_scoring="native"):
    """IvTest end to end.  plda = (F, G, Sigma) initial matrices in the normalised space; plda_scoring "native" (the sum of a model's
    vectors with its session count) or "enrollMean" (their mean as one session).  -> scores [nModels, nTest]."""
    return iv_test_trials(dev, sps, enrol, enrol_per_model, test, None, None, scoring, iv_norm, iv_norm_it, sph_norm, lda_rank, wccn, plda, plda_it,
                          device, plda_scoring)


def iv_test_trials(dev, sps, enrol, enrol_per_model, test, trial_model, trial_seg, scoring="cosine", iv_norm=False, iv_norm_it=1, sph_norm=False,
                   lda_rank=0, wccn=False, plda=None, plda_it=0, device=0, plda_scoring="native"):
    """IvTest on a list of trials (liagpu::ivTestTrials): trial i is model trial_model[i] against test vector trial_seg[i].
    -> scores [ntrial] in list order.  trial_model = None: the dense matrix [nModels, nTest] (liagpu::ivTest)."""
    dev = np.ascontiguousarray(dev, np.float64); enrol = np.ascontiguousarray(enrol, np.float64); test = np.ascontiguousarray(test, np.float64)
    dim, n_dev = dev.shape
    sps = np.ascontiguousarray(sps, np.int64); epm = np.ascontiguousarray(enrol_per_model, np.int64)
    cfg, keep = _iv_test_cfg(scoring, iv_norm, iv_norm_it, sph_norm, lda_rank, wccn, plda, plda_it, plda_scoring)
    head = (device, dim, ct.c_long(n_dev), _d(dev), ct.c_long(len(sps)), sps.ctypes.data_as(_lp), ct.c_long(len(epm)), epm.ctypes.data_as(_lp),
            _d(enrol), ct.c_long(test.shape[1]), _d(test))
    if trial_model is None:
        out = np.empty((len(epm), test.shape[1]))
        if plda_scoring == "native":
            _chk(lib.liagpu_iv_test(*head, *cfg[:-1], _d(out)))
        else:
            _chk(lib.liagpu_iv_test_trials(*head, *cfg, ct.c_long(0), None, None, _d(out)))
        return out
    tm = np.ascontiguousarray(trial_model, np.int32); ts = np.ascontiguousarray(trial_seg, np.int32)
    assert tm.shape == ts.shape and tm.ndim == 1
    out = np.empty(len(tm))
    _chk(lib.liagpu_iv_test_trials(*head, *cfg, ct.c_long(len(tm)), ct.c_void_p(tm.ctypes.data), ct.c_void_p(ts.ctypes.data), _d(out)))
    return out


def load_iv_test_ndx(ndx_path, target_id_list=None):
    """liagpu::loadIvTestNdx (host only, needs no GPU) -> dict(models, sessions, segs, trial_model, trial_seg, dropped, max_sessions)"""
    dims = (ct.c_long * 6)()
    tl = None if not target_id_list else str(target_id_list).encode()
    _chk(lib.liagpu_iv_test_ndx_load(str(ndx_path).encode(), tl, dims, None, ct.c_long(0)))
    cap = os.path.getsize(ndx_path) + (os.path.getsize(target_id_list) if target_id_list else 0) + 32 * (dims[0] + dims[1] + dims[2]) + 64
    buf = ct.create_string_buffer(cap)
    _chk(lib.liagpu_iv_test_ndx_load(str(ndx_path).encode(), tl, dims, buf, ct.c_long(cap)))
    models, sessions, segs, tm, ts = [], [], [], [], []
    for line in buf.value.decode().splitlines():
        f = line.split()
        if f[0] == "M":
            models.append(f[1]); sessions.append(f[2:])
        elif f[0] == "S":
            segs.append(f[1])
        else:
            tm.append(int(f[1])); ts.append(int(f[2]))
    return dict(models=models, sessions=sessions, segs=segs, trial_model=np.array(tm, np.int32), trial_seg=np.array(ts, np.int32),
                dropped=int(dims[3]), max_sessions=int(dims[5]))


def iv_test_ndx(dev, sps, ndx_path, vector_path, out_path, target_id_list=None, vector_ext=".y", fmt="DB", gender="M", threshold=0.0,
                scoring="cosine", iv_norm=False, iv_norm_it=1, sph_norm=False, lda_rank=0, wccn=False, plda=None, plda_it=0, device=0,
                plda_scoring="native"):
    """IvTest from files on an ndx (liagpu::ivTestFiles): writes the result lines to out_path (segment-major, model index ascending).
    -> dict(line_model, line_seg, scores) of the lines, in file order."""
    dev = np.ascontiguousarray(dev, np.float64)
    dim, n_dev = dev.shape
    sps = np.ascontiguousarray(sps, np.int64)
    cfg, keep = _iv_test_cfg(scoring, iv_norm, iv_norm_it, sph_norm, lda_rank, wccn, plda, plda_it, plda_scoring)
    nx = load_iv_test_ndx(ndx_path, target_id_list)
    n = len(nx["trial_model"])
    lm = np.zeros(max(n, 1), np.int32); ls = np.zeros(max(n, 1), np.int32); sc = np.zeros(max(n, 1)); cnt = ct.c_long(0)
    tl = None if not target_id_list else str(target_id_list).encode()
    _chk(lib.liagpu_iv_test_ndx(device, dim, ct.c_long(n_dev), _d(dev), ct.c_long(len(sps)), sps.ctypes.data_as(_lp), str(ndx_path).encode(), tl,
                                str(vector_path).encode(), vector_ext.encode(), fmt.encode(), str(out_path).encode(), gender.encode(),
                                ct.c_double(threshold), *cfg, ct.c_long(n), ct.c_void_p(lm.ctypes.data), ct.c_void_p(ls.ctypes.data), _d(sc),
                                ct.byref(cnt)))
    k = cnt.value
    return dict(line_model=lm[:k], line_seg=ls[:k], scores=sc[:k], ndx=nx)


def tv_train(N, F, ubm, Tmat, nb_it, min_div=True, device=0):
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    N = np.ascontiguousarray(N, np.float64); F = np.ascontiguousarray(F, np.float64)
    Tm = np.array(Tmat, np.float64)
    R = Tm.shape[0]
    means = np.empty(C * D)
    _chk(lib.liagpu_tv_train(device, ct.c_long(N.shape[0]), C, D, _d(w), _d(mean), _d(cov), R, _d(N), _d(F), _d(Tm), nb_it,
                             int(min_div), _d(means)))
    return Tm, means


def io_xml(xml_in, xml_out, raw_out=""):
    dims = np.zeros(2, np.int64); first = np.zeros(3)
    _chk(lib.liagpu_io_xml(xml_in.encode(), xml_out.encode(), raw_out.encode(), dims.ctypes.data_as(_lp), _d(first)))
    return dims, first


def io_db_header_bytes(nbytes=0):
    """Width (4 | 8) of the rows / cols extents writeMatrixDB writes; returns the previous width (0 only queries)."""
    return int(lib.liagpu_io_db_header_bytes(int(nbytes)))


def io_matrix_convert(path_in, fmt_in, path_out, fmt_out):
    dims = np.zeros(2, np.int64)
    _chk(lib.liagpu_io_matrix_convert(path_in.encode(), fmt_in.encode(), path_out.encode(), fmt_out.encode(), dims.ctypes.data_as(_lp)))
    return tuple(int(v) for v in dims)


def io_vectors(directory, ids, ext, fmt, W):
    W = np.ascontiguousarray(W, np.float64)
    n, rank = W.shape
    arr = (ct.c_char_p * n)(*[i.encode() for i in ids])
    back = np.empty((rank, n))
    _chk(lib.liagpu_io_vectors(directory.encode(), n, arr, ext.encode(), fmt.encode(), rank, _d(W), _d(back)))
    return back


def tv_init_t(ubm, R, seed=1, device=0):
    """TVAcc::initT, randomInitLaw normal (glibc rand() Box-Muller chain); seed 1 = a process that never called srand."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    Tm = np.empty((R, C * D))
    _chk(lib.liagpu_tv_init_t(device, C, D, _d(w), _d(mean), _d(cov), R, ct.c_uint(seed), _d(Tm)))
    return Tm


def tv_stats_lines(x, file_begin, lines, ubm, device=0):
    """Baum-Welch statistics per ndx line through liagpu::TVAcc (a file may be listed on several lines)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C = len(w)
    fb = np.ascontiguousarray(file_begin, np.int64)
    off = np.zeros(len(lines) + 1, np.int64); off[1:] = np.cumsum([len(l) for l in lines])
    files = np.ascontiguousarray([f for l in lines for f in l] or [0], np.int64)
    N = np.empty((len(lines), C)); F = np.empty((len(lines), C * D))
    _chk(lib.liagpu_tv_stats_lines(device, x.ctypes.data_as(_fp), ct.c_long(T), D, fb.ctypes.data_as(_lp), ct.c_long(len(fb) - 1),
                                   ct.c_long(len(lines)), off.ctypes.data_as(_lp), files.ctypes.data_as(_lp), C, _d(w), _d(mean), _d(cov),
                                   _d(N), _d(F)))
    return N, F


def tv_train_dist(N, F, ubm, Tmat, nb_it, world=1, rank=0, id_file="", n_total=None, min_div=True, device=0, overlap=False):
    """One rank of a multi-GPU TotalVariability run (liagpu_tv_train_dist2); returns (T, means, times_ms [nb_it x 4]).
    overlap: TVAcc::setOverlap -- the reduce-scatter of A starts inside estimateAandC, the all-gather of T is joined inside minDivergence."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    N = np.ascontiguousarray(N, np.float64); F = np.ascontiguousarray(F, np.float64)
    Tm = np.array(Tmat, np.float64)
    R = Tm.shape[0]
    means = np.empty(C * D); times = np.zeros((nb_it, 4))
    _chk(lib.liagpu_tv_train_dist2(device, world, rank, id_file.encode(), ct.c_long(N.shape[0]), ct.c_long(n_total or N.shape[0]), C, D, _d(w),
                                   _d(mean), _d(cov), R, _d(N), _d(F), _d(Tm), nb_it, int(min_div), int(overlap), _d(means), _d(times)))
    return Tm, means, times


def train_world_dist(x, seg_begin, seg_len, w, mean, cov, nb_it, global_cov, world=1, rank=0, id_file="", init_floor=0.0, final_floor=0.0,
                     init_ceil=10.0, final_ceil=10.0, device=0):
    """One rank of a multi-GPU TrainWorld run (liagpu_train_world_dist)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    w = np.array(w, np.float64); mean = np.array(mean, np.float64); cov = np.array(cov, np.float64)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    llk = np.empty(nb_it); gc = np.ascontiguousarray(global_cov, np.float64)
    _chk(lib.liagpu_train_world_dist(device, world, rank, id_file.encode(), x.ctypes.data_as(_fp), ct.c_long(T), D, bp, lp, ct.c_long(len(b)),
                                     len(w), _d(w), _d(mean), _d(cov), nb_it, ct.c_double(init_floor), ct.c_double(final_floor),
                                     ct.c_double(init_ceil), ct.c_double(final_ceil), _d(gc), _d(llk)))
    return dict(w=w, mean=mean, cov=cov, llk=llk)


def jfa_train(task, sess_per_spk, ubm, N, N_h, F_X, F_X_h, V, U, Dm, nb_it, Z0=None, ortho_v=False, device=0):
    """EigenVoice (task 0) / EigenChannel (1) / EstimateDMatrix (2) on given statistics; returns dict(V, U, D, Y, X, Z)."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    sps = np.ascontiguousarray(sess_per_spk, np.int64)
    nspk, nsess = len(sps), int(sps.sum())
    N, N_h, F_X, F_X_h = [np.ascontiguousarray(a, np.float64) for a in (N, N_h, F_X, F_X_h)]
    V = np.array(V, np.float64); U = np.array(U, np.float64); Dm = np.array(Dm, np.float64)
    Y = np.zeros((nspk, V.shape[0])); X = np.zeros((nsess, U.shape[0])); Z = np.zeros((nspk, C * D))
    z0 = None if Z0 is None else np.ascontiguousarray(Z0, np.float64)
    _chk(lib.liagpu_jfa_train(device, task, ct.c_long(nspk), sps.ctypes.data_as(_lp), C, D, _d(w), _d(mean), _d(cov), V.shape[0], U.shape[0],
                              _d(N), _d(N_h), _d(F_X), _d(F_X_h), _d(V), _d(U), _d(Dm), None if z0 is None else _d(z0), nb_it, int(ortho_v),
                              _d(Y), _d(X), _d(Z)))
    return dict(V=V, U=U, D=Dm, Y=Y, X=X, Z=Z)


def jfa_dot_product(ubm, N, F, V, U, Dm, client_sv, device=0):
    """ComputeTest dot-product scoring in the JFA framework: scores[nTest, nClients]."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    N, F, V, U, Dm, client_sv = [np.ascontiguousarray(a, np.float64) for a in (N, F, V, U, Dm, client_sv)]
    sc = np.empty((N.shape[0], client_sv.shape[0]))
    _chk(lib.liagpu_jfa_dot_product(device, ct.c_long(N.shape[0]), C, D, _d(w), _d(mean), _d(cov), V.shape[0], U.shape[0], _d(N), _d(F), _d(V),
                                    _d(U), _d(Dm), ct.c_long(client_sv.shape[0]), _d(client_sv), _d(sc)))
    return sc

def tv_stats_cross_server(x_own, x, utt_begin, ubm, device=0):
    """N / F of a TVAcc on one GpuServer from the frames of a FeatureBuffer on ANOTHER server; the accumulator's server holds
    the (clean) buffer x_own.  -> N, F, (unusable frames of x_own, of x), assume_finite of the accumulator's context afterwards."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    x_own = np.ascontiguousarray(x_own, np.float32); x = np.ascontiguousarray(x, np.float32)
    ub = np.ascontiguousarray(utt_begin, np.int64)
    U = len(ub) - 1
    N = np.empty((U, C)); F = np.empty((U, C * D))
    bad = (ct.c_long * 2)(); af = ct.c_long(-7)
    _chk(lib.liagpu_tv_stats_cross_server(device, x_own.ctypes.data_as(_fp), ct.c_long(x_own.shape[0]), x.ctypes.data_as(_fp), ct.c_long(x.shape[0]), D,
                                          ub.ctypes.data_as(_lp), ct.c_long(U), C, _d(w), _d(mean), _d(cov), _d(N), _d(F), bad, ct.byref(af)))
    return N, F, (bad[0], bad[1]), af.value


def jfa_stats(x, sess_begin, sess_per_spk, ubm, device=0):
    """JFAAcc::computeAndAccumulateJFAStat on float32 frames: returns N, N_h, F_X, F_X_h."""
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    x = np.ascontiguousarray(x, np.float32)
    sb = np.ascontiguousarray(sess_begin, np.int64); sps = np.ascontiguousarray(sess_per_spk, np.int64)
    nspk, nsess = len(sps), len(sb) - 1
    N = np.empty((nspk, C)); Nh = np.empty((nsess, C)); FX = np.empty((nspk, C * D)); FXh = np.empty((nsess, C * D))
    _chk(lib.liagpu_jfa_stats(device, x.ctypes.data_as(ct.POINTER(ct.c_float)), ct.c_long(x.shape[0]), D, sb.ctypes.data_as(_lp), ct.c_long(nspk),
                              sps.ctypes.data_as(_lp), C, _d(w), _d(mean), _d(cov), _d(N), _d(Nh), _d(FX), _d(FXh)))
    return N, Nh, FX, FXh

def jfa_session_model_host(means, V, y, Dm, z, U, x):
    """getUX / getSpeakerModel host arithmetic of one session (no device): -> (ux [SV], m + V y + D z + U x [SV])."""
    means, V, y, Dm, z, U, x = [np.ascontiguousarray(a, np.float64) for a in (means, V, y, Dm, z, U, x)]
    SV = means.size
    ux = np.empty(SV); sp = np.empty(SV)
    _chk(lib.liagpu_jfa_session_model_host(ct.c_long(SV), V.shape[0], U.shape[0], _d(means), _d(V), _d(y), _d(Dm), _d(z), _d(U), _d(x), _d(ux), _d(sp)))
    return ux, sp


def _clusters(clusters):
    """list (one per session) of lists of (begin, length) -> offsets, begins, lengths as int64 arrays"""
    off = np.zeros(len(clusters) + 1, np.int64)
    for h, c in enumerate(clusters):
        off[h + 1] = off[h] + len(c)
    b = np.ascontiguousarray([s[0] for c in clusters for s in c], np.int64)
    l = np.ascontiguousarray([s[1] for c in clusters for s in c], np.int64)
    return off, b, l


def jfa_normalize_features(x, sess_per_spk, clusters, ubm, V, U, Dm, Y, X, Z, device=0, batched=None):
    """JFAAcc::normalizeFeatures on float32 frames: -> (compensated frames, ux [nsess, SV], session model means [nsess, SV]).
    batched=True: JFAAcc::normalizeFeaturesBatch (all sessions in one device pass), batched=False: the per-session loop; either
    returns the compensated frames alone.  None: the loop, with the two tables (the call as it always was)."""
    if batched is not None:
        w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
        C, D = mean.shape
        x = np.array(x, np.float32)
        sps = np.ascontiguousarray(sess_per_spk, np.int64)
        off, b, l = _clusters(clusters)
        V, U, Dm, Y, X, Z = [np.ascontiguousarray(a, np.float64) for a in (V, U, Dm, Y, X, Z)]
        _chk(lib.liagpu_jfa_normalize_features_batch(device, x.ctypes.data_as(_fp), ct.c_long(x.shape[0]), D, ct.c_long(len(sps)), sps.ctypes.data_as(_lp),
                                                     off.ctypes.data_as(_lp), b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), C, _d(w), _d(mean), _d(cov),
                                                     V.shape[0], U.shape[0], _d(V), _d(U), _d(Dm), _d(Y), _d(X), _d(Z), int(bool(batched))))
        return x
    w, mean, cov = [np.ascontiguousarray(a, np.float64) for a in ubm]
    C, D = mean.shape
    x = np.array(x, np.float32)
    sps = np.ascontiguousarray(sess_per_spk, np.int64)
    off, b, l = _clusters(clusters)
    V, U, Dm, Y, X, Z = [np.ascontiguousarray(a, np.float64) for a in (V, U, Dm, Y, X, Z)]
    nsess = int(sps.sum())
    ux = np.empty((nsess, C * D)); models = np.empty((nsess, C * D))
    _chk(lib.liagpu_jfa_normalize_features(device, x.ctypes.data_as(_fp), ct.c_long(x.shape[0]), D, ct.c_long(len(sps)), sps.ctypes.data_as(_lp),
                                           off.ctypes.data_as(_lp), b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), C, _d(w), _d(mean), _d(cov),
                                           V.shape[0], U.shape[0], _d(V), _d(U), _d(Dm), _d(Y), _d(X), _d(Z), _d(ux), _d(models)))
    return x, ux, models


def feature_mapping(x, cluster, cd, ci, device=0):
    """liagpu::featureMapping on float32 frames over one cluster [(begin, length), ...]; cd / ci = (w, mean, cov) -> mapped frames."""
    x = np.array(x, np.float32)
    wd, md, vd = [np.ascontiguousarray(a, np.float64) for a in cd]
    wi, mi, vi = [np.ascontiguousarray(a, np.float64) for a in ci]
    C, D = md.shape
    _, b, l = _clusters([cluster])
    _chk(lib.liagpu_feature_mapping(device, x.ctypes.data_as(_fp), ct.c_long(x.shape[0]), D, b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), ct.c_long(len(b)),
                                    C, _d(wd), _d(md), _d(vd), _d(wi), _d(mi), _d(vi)))
    return x


def _sources(src_first, T):
    sf = np.ascontiguousarray([0] if src_first is None else src_first, np.int64)
    return np.ascontiguousarray(np.append(sf, T), np.int64)


def norm_feat(x, clusters, src_first=None, segmental_mode=False, file_mode=False, cms_only=False, var_only=False, ext_mean=None,
              ext_std=None, first_col=0, ncols=0, device=0):
    """liagpu::normFeat (NormFeat's default mode) on float32 frames [T, D]: clusters = one list of (begin, length) per source (begins
    counted from the source's first frame), src_first = first frame of every source (None: one source) -> the normalised frames."""
    x = np.array(x, np.float32)
    T, D = x.shape
    sf = _sources(src_first, T)
    off, b, l = _clusters(clusters)
    em = None if ext_mean is None else np.ascontiguousarray(ext_mean, np.float64)
    es = None if ext_std is None else np.ascontiguousarray(ext_std, np.float64)
    _chk(lib.liagpu_norm_feat(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(len(sf) - 1), sf.ctypes.data_as(_lp), off.ctypes.data_as(_lp),
                              b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), int(segmental_mode), int(file_mode), int(cms_only), int(var_only),
                              None if em is None else _d(em), None if es is None else _d(es), int(first_col), int(ncols)))
    return x


def norm_feat_online(x, src_first=None, window_duration=300, init_with_delay=0, device=0):
    """liagpu::normFeatOnlineMode (NormFeatWindowMode) on float32 frames [T, D], every source on its own -> the normalised frames."""
    x = np.array(x, np.float32)
    T, D = x.shape
    sf = _sources(src_first, T)
    _chk(lib.liagpu_norm_feat_online(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(len(sf) - 1), sf.ctypes.data_as(_lp),
                                     ct.c_long(window_duration), ct.c_long(init_with_delay)))
    return x


def norm_feat_window(x, clusters, src_first=None, window_duration=5.0, window_comp=1.0, frame_length=0.01, file_mode=False, cms_only=False,
                     var_only=False, first_col=0, ncols=0, device=0):
    """liagpu::normFeat with windowMode (NormFeat.cpp:372-447) on float32 frames [T, D]: clusters and src_first as norm_feat takes them;
    the segments of a cluster in increasing order and not overlapping.  file_mode: the file pass afterwards -> the normalised frames."""
    x = np.array(x, np.float32)
    T, D = x.shape
    sf = _sources(src_first, T)
    off, b, l = _clusters(clusters)
    _chk(lib.liagpu_norm_feat_window(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(len(sf) - 1), sf.ctypes.data_as(_lp), off.ctypes.data_as(_lp),
                                     b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), ct.c_double(window_duration), ct.c_double(window_comp),
                                     ct.c_double(frame_length), int(file_mode), int(cms_only), int(var_only), int(first_col), int(ncols)))
    return x


def read_histo(path):
    """liagpu::readHistoFile (a Histo::save file) -> (bounds [nbin + 1], count [nbin])"""
    lib.liagpu_histo_bins.restype = ct.c_long
    nb = lib.liagpu_histo_bins(path.encode())
    if nb < 0:
        raise HostError(lib.liagpu_last_error().decode())
    b, c = np.zeros(nb + 1), np.zeros(nb)
    _chk(lib.liagpu_histo_read(path.encode(), _d(b), _d(c)))
    return b, c


def write_histo(path, bounds, count):
    """liagpu::writeHistoFile: the layout and the precision (%g) of Histo::save"""
    b, c = np.ascontiguousarray(bounds, np.float64), np.ascontiguousarray(count, np.float64)
    _chk(lib.liagpu_histo_write(path.encode(), len(c), _d(b), _d(c)))


def _target(target):
    if target is None:
        return 0, None, None, None
    if isinstance(target, str):
        return 0, None, None, target.encode()
    b, c = np.ascontiguousarray(target[0], np.float64), np.ascontiguousarray(target[1], np.float64)
    return len(c), b, c, None


def norm_feat_warp(x, clusters, target, src_first=None, segmental_mode=False, file_mode=False, warp_bin_count=40, warp_add01_norm=False,
                   window_mode=False, cms_only=False, var_only=False, first_col=0, ncols=0, device=0):
    """liagpu::normFeat with warp (NormFeat.cpp:362-368, 465-483) on float32 frames [T, D]: clusters and src_first as norm_feat takes
    them, the segments of a cluster in increasing order; target = (bounds, count) or the path of a .histo file (warpGaussHistoFilename;
    None: refused, the rand()-made default target is not built).  window_mode, cms_only, var_only are refused with it -> the frames."""
    x = np.array(x, np.float32)
    T, D = x.shape
    sf = _sources(src_first, T)
    off, b, l = _clusters(clusters)
    nt, tb, tc, path = _target(target)
    _chk(lib.liagpu_norm_feat_warp(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(len(sf) - 1), sf.ctypes.data_as(_lp), off.ctypes.data_as(_lp),
                                   b.ctypes.data_as(_lp), l.ctypes.data_as(_lp), int(segmental_mode), int(file_mode), int(window_mode), int(cms_only),
                                   int(var_only), ct.c_long(warp_bin_count), int(warp_add01_norm), nt, None if tb is None else _d(tb),
                                   None if tc is None else _d(tc), path, int(first_col), int(ncols)))
    return x


def feat_warp_host(x, runs, nunits, target, warp_bin_count=40):
    """liagpu::featWarpHost, the host-only twin of warp's per-unit loop (no device): float32 frames [T, D], runs [nrun, 3] = (first frame,
    length, unit), target = (bounds, count) -> (the warped frames, status [nunits, D])"""
    x = np.array(x, np.float32)
    T, D = x.shape
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    tb, tc = np.ascontiguousarray(target[0], np.float64), np.ascontiguousarray(target[1], np.float64)
    st = np.zeros((nunits, D), np.int32)
    _chk(lib.liagpu_feat_warp_host(x.ctypes.data_as(_fp), ct.c_long(D), D, r.ctypes.data_as(_lp), ct.c_long(len(r)), ct.c_long(nunits),
                                   ct.c_long(warp_bin_count), len(tc), _d(tb), _d(tc), st.ctypes.data_as(ct.POINTER(ct.c_int))))
    return x, st


def norm_feat_files(names, feature_path="", load_ext=".prm", save_ext=".norm.prm", label_path="", label_ext=".lbl", label="speech",
                    frame_length=0.01, mask="", write_all_features=True, save_path="", segmental_mode=False, file_mode=False, cms_only=False,
                    var_only=False, device=0, window_mode=False, window_duration=5.0, window_comp=1.0, warp=False, warp_bin_count=40,
                    warp_gauss_histo_filename="", warp_add01_norm=False):
    """liagpu::normFeatFiles: <feature_path><name><load_ext> -> <save_path or feature_path><name><save_ext> for every name, one batch.
    window_mode: NormFeat's windowMode with window_duration / window_comp (segmental_mode with it is refused, file_mode follows it).
    warp: feature warping onto the table of warp_gauss_histo_filename (needed), warp_bin_count bins per histogram, warp_add01_norm the
    mean / std pass afterwards; window_mode, cms_only and var_only with it are refused."""
    arr = (ct.c_char_p * len(names))(*[n.encode() for n in names])
    if warp:
        _chk(lib.liagpu_norm_feat_files_warp(device, len(names), arr, feature_path.encode(), load_ext.encode(), save_path.encode(), save_ext.encode(),
                                             label_path.encode(), label_ext.encode(), label.encode(), ct.c_double(frame_length), mask.encode(),
                                             int(write_all_features), int(segmental_mode), int(file_mode), int(window_mode), int(cms_only),
                                             int(var_only), ct.c_long(warp_bin_count), int(warp_add01_norm), warp_gauss_histo_filename.encode()))
        return
    if window_mode:
        if segmental_mode:
            raise HostError(" Incompatible modes (segmental/windowMode)")
        _chk(lib.liagpu_norm_feat_files_window(device, len(names), arr, feature_path.encode(), load_ext.encode(), save_path.encode(), save_ext.encode(),
                                               label_path.encode(), label_ext.encode(), label.encode(), ct.c_double(frame_length), mask.encode(),
                                               int(write_all_features), int(file_mode), int(cms_only), int(var_only), ct.c_double(window_duration),
                                               ct.c_double(window_comp)))
        return
    _chk(lib.liagpu_norm_feat_files(device, len(names), arr, feature_path.encode(), load_ext.encode(), save_path.encode(), save_ext.encode(),
                                    label_path.encode(), label_ext.encode(), label.encode(), ct.c_double(frame_length), mask.encode(),
                                    int(write_all_features), int(segmental_mode), int(file_mode), int(cms_only), int(var_only)))


def compute_test_files(world_path, client_paths, client_names, prm_path, lbl_path, mask="", label="male", frame_length=0.01,
                       top_c=10, complete=True, min_llk=-200.0, max_llk=200.0, gender="M", test_name="test", threshold=0.0,
                       device=0):
    """ComputeTest (segmental mode) driven from RAW model / .prm / .lbl files; returns (LLR[nseg, nclients], text)."""
    n = len(client_paths)
    cp = (ct.c_char_p * n)(*[p.encode() for p in client_paths])
    cn = (ct.c_char_p * n)(*[p.encode() for p in client_names])
    llr = np.empty(4096)
    text = ct.create_string_buffer(1 << 16)
    _chk(lib.liagpu_compute_test_files(device, world_path.encode(), n, cp, cn, prm_path.encode(), lbl_path.encode(), mask.encode(),
                                       label.encode(), ct.c_double(frame_length), top_c, int(complete), ct.c_double(min_llk),
                                       ct.c_double(max_llk), gender.encode(), test_name.encode(), ct.c_double(threshold),
                                       llr.ctypes.data_as(_dp), ct.c_long(len(llr)), text, ct.c_long(len(text))))
    lines = text.value.decode().strip().split("\n")
    return llr[:len(lines)].reshape(-1, n), lines


def _lines(seg_begin_per_line, seg_len_per_line, clients_per_line, n_models):
    """flat tables of a trial list (liagpu_compute_test_batch); raises HostError for what needs no device to be refused"""
    if not (len(seg_begin_per_line) == len(seg_len_per_line) == len(clients_per_line)):
        raise HostError("compute_test_batch: one segment list and one client list per line are needed")
    so = [0]; co = [0]; sb = []; sl = []; cl = []
    for l, (b, n, c) in enumerate(zip(seg_begin_per_line, seg_len_per_line, clients_per_line)):
        if len(b) != len(n):
            raise HostError("compute_test_batch: line %d has %d segment begins and %d lengths" % (l, len(b), len(n)))
        for g in c:
            if not 0 <= int(g) < n_models:
                raise HostError("compute_test_batch: line %d names client %d of %d" % (l, int(g), n_models))
        sb += [int(v) for v in b]; sl += [int(v) for v in n]; cl += [int(g) for g in c]
        so.append(len(sb)); co.append(len(cl))
    return [np.ascontiguousarray(a, np.int64) for a in (so, sb, sl, co, cl)]


def compute_test_batch(x, seg_begin_per_line, seg_len_per_line, world, models, clients_per_line, top_c=10, complete=True, min_llk=-200.0,
                       max_llk=200.0, segmental=False, loop=False, device=0):
    """ComputeTest for a whole trial list in one device pass (liagpu::computeTestBatch): line l scores the segments
    (seg_begin_per_line[l], seg_len_per_line[l]) of x against the models clients_per_line[l] (indices into `models`, a list of
    (w, mean, cov) like compute_test's clients; the Gaussian counts may differ -- such a list runs the per-line loop).  loop=True: the
    computeTestLLR loop line by line.  -> list of LLR[n_seg_or_1, n_clients_of_the_line]."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    ww, mw, cw = [np.ascontiguousarray(a, np.float64) for a in world]
    so, sb, sl, co, cl = _lines(seg_begin_per_line, seg_len_per_line, clients_per_line, len(models))
    mC = np.ascontiguousarray([len(m[0]) for m in models], np.int32)
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(m[k], np.float64).ravel() for m in models]) if models else np.zeros(0))
    wc, mc, cc = cat(0), cat(1), cat(2)
    nl = len(so) - 1
    per = [(int(so[l + 1] - so[l]) if segmental else 1, int(co[l + 1] - co[l])) for l in range(nl)]
    out = np.empty(max(1, sum(a * b for a, b in per)))
    n = ct.c_long(0)
    p = lambda a: a.ctypes.data_as(_lp)
    _chk(lib.liagpu_compute_test_batch(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(nl), p(so), p(sb), p(sl), len(ww), _d(ww), _d(mw), _d(cw),
                                       len(models), mC.ctypes.data_as(ct.POINTER(ct.c_int)), _d(wc), _d(mc), _d(cc), p(co), p(cl), int(top_c),
                                       int(complete), ct.c_double(min_llk), ct.c_double(max_llk), int(segmental), int(bool(loop)), _d(out),
                                       ct.c_long(len(out)), ct.byref(n)))
    res, k = [], 0
    for a, b in per:
        res.append(out[k:k + a * b].reshape(a, b).copy())
        k += a * b
    return res


def compute_test_jfa(x, seg_begin_per_line, seg_len_per_line, world, U, models, clients_per_line, top_c=10, complete=True, min_llk=-200.0,
                     max_llk=200.0, compose=False, device=0):
    """ComputeTestJFA for a whole trial list (liagpu::computeTestJFABatch): per line the channel factor of the test file from its
    selected frames, those frames compensated, then the LLR of every client of the line (one per line and client, worldDecime 1).
    world = (w, mean, cov); U [rankEC, C*D]; models: (w, mean, cov) of the world's shape.  compose=True: the same through the existing
    calls (JFAAcc steps, the normalizeFeatures loop on a copy of x, computeTestBatch).  x is not rewritten.
    -> (list of LLR[n_clients], compensated frames [sum of the selections, D] float32 line after line, channel factors [nlines, rankEC])."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    ww, mw, cw = [np.ascontiguousarray(a, np.float64) for a in world]
    U = np.ascontiguousarray(U, np.float64)
    so, sb, sl, co, cl = _lines(seg_begin_per_line, seg_len_per_line, clients_per_line, len(models))
    for m in models:
        if np.shape(m[1]) != mw.shape:
            raise HostError("compute_test_jfa: every client model must have the world's shape")
    if U.ndim != 2 or U.shape[1] != mw.size:
        raise HostError("compute_test_jfa: U must be [rankEC, C*D]")
    cat = lambda k: np.ascontiguousarray(np.concatenate([np.asarray(m[k], np.float64).ravel() for m in models]) if models else np.zeros(0))
    wc, mc, cc = cat(0), cat(1), cat(2)
    nl = len(so) - 1
    out = np.empty(max(1, int(co[-1])))
    comp = np.empty((int(sl.sum()), D), np.float32)
    xf = np.zeros((nl, U.shape[0]))
    n = ct.c_long(0)
    p = lambda a: a.ctypes.data_as(_lp)
    _chk(lib.liagpu_compute_test_jfa(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(nl), p(so), p(sb), p(sl), len(ww), _d(ww), _d(mw), _d(cw),
                                     U.shape[0], _d(U), len(models), _d(wc), _d(mc), _d(cc), p(co), p(cl), int(top_c), int(complete),
                                     ct.c_double(min_llk), ct.c_double(max_llk), int(bool(compose)), _d(out), ct.c_long(len(out)), ct.byref(n),
                                     comp.ctypes.data_as(_fp), _d(xf)))
    return [out[int(co[l]):int(co[l + 1])].copy() for l in range(nl)], comp, xf


def compute_test_ndx(world_path, ndx_path, model_path, feature_path, label_path, model_ext=".gmm", feature_ext=".prm", label_ext=".lbl", mask="",
                     label="male", frame_length=0.01, top_c=10, complete=True, min_llk=-200.0, max_llk=200.0, gender="M", threshold=0.0, device=0):
    """ComputeTest (segmental mode) for a whole ndx -- every line a test file name followed by its client ids -- in one device pass.  Files:
    <feature_path><test><feature_ext>, <label_path><test><label_ext>, <model_path><id><model_ext> (RAW).  -> (LLR [flat, line after line,
    each [segment][client]], result lines in the format of compute_test_files)."""
    n = ct.c_long(0); nbytes = ct.c_long(0)                     # sizes from the ndx and the label files (host only)
    _chk(lib.liagpu_compute_test_ndx_count(ndx_path.encode(), label_path.encode(), label_ext.encode(), label.encode(), ct.c_double(frame_length),
                                           gender.encode(), ct.byref(n), ct.byref(nbytes)))
    llr = np.empty(max(n.value, 1))
    text = ct.create_string_buffer(max(nbytes.value, 1))
    _chk(lib.liagpu_compute_test_ndx(device, world_path.encode(), ndx_path.encode(), model_path.encode(), model_ext.encode(), feature_path.encode(),
                                     feature_ext.encode(), label_path.encode(), label_ext.encode(), mask.encode(), label.encode(),
                                     ct.c_double(frame_length), int(top_c), int(complete), ct.c_double(min_llk), ct.c_double(max_llk), gender.encode(),
                                     ct.c_double(threshold), llr.ctypes.data_as(_dp), ct.c_long(len(llr)), ct.byref(n), text, ct.c_long(len(text))))
    t = text.value.decode().strip()
    return llr[:n.value].copy(), (t.split("\n") if t else [])


def bench_computetest(x, world, mean_cl, line_clients, frames_per_line, top_c=10, complete=True, which=0, reps=3, trial_piece=0, device=0):
    """liagpu_bench_computetest (tools/bench_computetest.py): len(line_clients) lines of frames_per_line frames of x, line l against the
    models line_clients[l] (rows of mean_cl [n_models, C*D]; weights and variances the world's); which = 0: computeTestBatch on resident
    models, 1: the computeTestLLR loop on resident models, 2: computeTestBatch from host models -> dict(ms [reps], kernel_ms, llr)."""
    x = np.ascontiguousarray(x, np.float32)
    T, D = x.shape
    ww, mw, cw = [np.ascontiguousarray(a, np.float64) for a in world]
    mean_cl = np.ascontiguousarray(mean_cl, np.float64).reshape(-1, len(ww) * D)
    lc = np.ascontiguousarray(line_clients, np.int64)
    nl, per = lc.shape
    ms = np.zeros(max(reps, 1)); km = np.zeros(5); llr = np.empty((nl, per))
    _chk(lib.liagpu_bench_computetest(device, x.ctypes.data_as(_fp), ct.c_long(T), D, ct.c_long(nl), ct.c_long(frames_per_line), len(ww), _d(ww), _d(mw),
                                      _d(cw), len(mean_cl), _d(mean_cl), ct.c_long(per), lc.ctypes.data_as(_lp), int(top_c), int(complete), int(which),
                                      int(reps), ct.c_long(trial_piece), _d(ms), _d(km), _d(llr)))
    return dict(ms=ms[:reps], kernel_ms=dict(k_llk_mfma=km[0], k_topc_rank=km[1], k_topc_use=km[2], k_trial_reduce=km[3]), piece=int(km[4]), llr=llr)


def energy_detector(energy, seg_begin, seg_len, C=2, nb_train_it=10, variance_flooring=0.5, variance_ceiling=10.0, alpha=0.25, device=0):
    """EnergyDetector (meanStd mode) on one energy column -> dict(begin, length, w, mean, cov, threshold)."""
    e = np.ascontiguousarray(energy, np.float32)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    ob = np.zeros(4096, np.int64); ol = np.zeros(4096, np.int64); n = ct.c_long(0)
    model = np.zeros(3 * C); th = ct.c_double(0.0)
    _chk(lib.liagpu_energy_detector(device, e.ctypes.data_as(_fp), ct.c_long(len(e)), bp, lp, ct.c_long(len(b)), int(C), int(nb_train_it),
                                    ct.c_double(variance_flooring), ct.c_double(variance_ceiling), ct.c_double(alpha),
                                    ob.ctypes.data_as(_lp), ol.ctypes.data_as(_lp), ct.c_long(len(ob)), ct.byref(n), _d(model), ct.byref(th)))
    return dict(begin=ob[:n.value].copy(), length=ol[:n.value].copy(), w=model[:C].copy(), mean=model[C:2 * C].copy(), cov=model[2 * C:].copy(),
                threshold=th.value)


def energy_detector_batch(energies, segments, C=2, nb_train_it=10, variance_flooring=0.5, variance_ceiling=10.0, alpha=0.25, device=0):
    """EnergyDetector (meanStd mode) on a LIST of energy columns in one device pass (liagpu::energyDetectorBatch): energies[f] a float32
    column, segments[f] = (seg_begin, seg_len) of its input label segments -> one dict(begin, length, w, mean, cov, threshold, status) per
    file.  The output arrays are sized from the frame counts: a file has at most one segment per two frames plus one per input segment."""
    es = [np.ascontiguousarray(e, np.float32).reshape(-1) for e in energies]
    nf = len(es)
    fb = np.zeros(nf + 1, np.int64)
    fb[1:] = np.cumsum([len(e) for e in es])
    x = np.concatenate(es) if nf and fb[-1] else np.zeros(0, np.float32)
    sb = [np.ascontiguousarray(s[0], np.int64).reshape(-1) for s in segments]
    sl = [np.ascontiguousarray(s[1], np.int64).reshape(-1) for s in segments]
    assert len(sb) == nf
    so = np.zeros(nf + 1, np.int64)
    so[1:] = np.cumsum([len(b) for b in sb])
    sbc = np.concatenate(sb + [np.zeros(1, np.int64)]); slc = np.concatenate(sl + [np.zeros(1, np.int64)])
    room = int(sum(int(l.sum()) // 2 + 1 + len(l) for l in sl)) + 1
    oo = np.zeros(nf + 1, np.int64); ob = np.zeros(room, np.int64); ol = np.zeros(room, np.int64)
    model = np.zeros((max(nf, 1), 3 * C)); th = np.zeros(max(nf, 1)); st = np.zeros(max(nf, 1), np.int32)
    _chk(lib.liagpu_energy_detector_batch(device, x.ctypes.data_as(_fp), ct.c_long(len(x)), fb.ctypes.data_as(_lp), ct.c_long(nf), so.ctypes.data_as(_lp),
                                          sbc.ctypes.data_as(_lp), slc.ctypes.data_as(_lp), int(C), int(nb_train_it), ct.c_double(variance_flooring),
                                          ct.c_double(variance_ceiling), ct.c_double(alpha), oo.ctypes.data_as(_lp), ob.ctypes.data_as(_lp),
                                          ol.ctypes.data_as(_lp), ct.c_long(room), _d(model), _d(th), st.ctypes.data_as(ct.POINTER(ct.c_int))))
    return [dict(begin=ob[oo[f]:oo[f + 1]].copy(), length=ol[oo[f]:oo[f + 1]].copy(), w=model[f, :C].copy(), mean=model[f, C:2 * C].copy(),
                 cov=model[f, 2 * C:].copy(), threshold=float(th[f]), status=int(st[f])) for f in range(nf)]


def energy_detector_files(names, feature_path="", load_ext=".prm", label_path="", label_ext=".lbl", label="speech", save_path="", save_ext=".enr.lbl",
                          label_out="speech", mask="", frame_length=0.01, C=2, nb_train_it=10, variance_flooring=0.5, variance_ceiling=10.0, alpha=0.25,
                          device=0):
    """liagpu::energyDetectorFiles: the list's feature files (mask picks the energy column) and label files in one batch; one output label
    file <save_path><name><save_ext> per name -> (thresholds [n], status [n])."""
    names = list(names)
    arr = (ct.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    th = np.zeros(max(len(names), 1)); st = np.zeros(max(len(names), 1), np.int32)
    _chk(lib.liagpu_energy_detector_files(device, len(names), arr, feature_path.encode(), load_ext.encode(), label_path.encode(), label_ext.encode(),
                                          label.encode(), save_path.encode(), save_ext.encode(), label_out.encode(), mask.encode(), ct.c_double(frame_length),
                                          int(C), int(nb_train_it), ct.c_double(variance_flooring), ct.c_double(variance_ceiling), ct.c_double(alpha), _d(th),
                                          st.ctypes.data_as(ct.POINTER(ct.c_int))))
    return th[:len(names)].copy(), st[:len(names)].copy()


def turn_detection_batch(frames, segments, crit="DGLR", win_size=50, win_step=5, alpha=0.7, min_llk=-200.0, max_llk=200.0, twin=False, device=0):
    """TurnDetection on a LIST of files in one device pass (liagpu::turnDetectionBatch), or -- twin=True -- the host-only loop twin
    liagpu::turnDetection file by file (no GPU): frames[f] a float32 matrix [T_f, D], segments[f] = (seg_begin, seg_len) of its input
    segments (frames of the file) -> one dict per file: begin, length (the output segments, frames of the file) and curves, one dict(value,
    smoothed, dec, mean, std) per input segment (empty arrays for a segment that is copied through).  crit DELTABIC is refused."""
    xs = [np.ascontiguousarray(x, np.float32) for x in frames]
    nf = len(xs)
    D = xs[0].shape[1] if nf else 1
    assert all(x.ndim == 2 and x.shape[1] == D for x in xs)
    fb = np.zeros(nf + 1, np.int64)
    fb[1:] = np.cumsum([len(x) for x in xs])
    x = np.concatenate(xs) if nf and fb[-1] else np.zeros((0, D), np.float32)
    sb = [np.ascontiguousarray(s[0], np.int64).reshape(-1) for s in segments]
    sl = [np.ascontiguousarray(s[1], np.int64).reshape(-1) for s in segments]
    assert len(sb) == nf
    so = np.zeros(nf + 1, np.int64)
    so[1:] = np.cumsum([len(b) for b in sb])
    sbc = np.concatenate(sb + [np.zeros(1, np.int64)]); slc = np.concatenate(sl + [np.zeros(1, np.int64)])
    npos = int(sum(int(np.maximum(0, -(-(l - 2 * win_size) // win_step)).sum()) for l in sl))
    room = npos + int(so[-1]) + 1
    oo = np.zeros(nf + 1, np.int64); ob = np.zeros(room, np.int64); ol = np.zeros(room, np.int64)
    co = np.zeros(int(so[-1]) + 1, np.int64); val = np.zeros(npos + 1); sm = np.zeros(npos + 1); dec = np.zeros(npos + 1, np.uint8)
    stats = np.zeros((int(so[-1]) + 1, 2))
    _chk(lib.liagpu_turn_detection_batch(device, int(bool(twin)), x.ctypes.data_as(_fp), ct.c_long(len(x)), int(D), fb.ctypes.data_as(_lp), ct.c_long(nf),
                                         so.ctypes.data_as(_lp), sbc.ctypes.data_as(_lp), slc.ctypes.data_as(_lp), crit.encode(), ct.c_long(win_size),
                                         ct.c_long(win_step), ct.c_double(alpha), ct.c_double(min_llk), ct.c_double(max_llk), oo.ctypes.data_as(_lp),
                                         ob.ctypes.data_as(_lp), ol.ctypes.data_as(_lp), ct.c_long(room), co.ctypes.data_as(_lp), _d(val), _d(sm),
                                         dec.ctypes.data_as(ct.c_void_p), _d(stats), ct.c_long(npos + 1)))
    out = []
    for f in range(nf):
        curves = [dict(value=val[co[q]:co[q + 1]].copy(), smoothed=sm[co[q]:co[q + 1]].copy(), dec=dec[co[q]:co[q + 1]].copy(), mean=float(stats[q, 0]),
                       std=float(stats[q, 1])) for q in range(int(so[f]), int(so[f + 1]))]
        out.append(dict(begin=ob[oo[f]:oo[f + 1]].copy(), length=ol[oo[f]:oo[f + 1]].copy(), curves=curves))
    return out


def turn_detection_files(names, feature_path="", load_ext=".prm", label_path="", label_ext=".lbl", label="speech", save_path="", save_ext=".turn.lbl",
                         mask="", frame_length=0.01, crit="DGLR", win_size=50, win_step=5, alpha=0.7, min_llk=-200.0, max_llk=200.0, max_segments=1 << 20,
                         device=0):
    """liagpu::turnDetectionFiles: the list's feature files and label files in one batch; one output label file <save_path><name><save_ext>
    per name, the input label kept on every piece -> per name (begin [], length []) of the segments written (frames of the file)."""
    names = list(names)
    arr = (ct.c_char_p * max(len(names), 1))(*[n.encode() for n in names])
    oo = np.zeros(len(names) + 1, np.int64); ob = np.zeros(max_segments, np.int64); ol = np.zeros(max_segments, np.int64)
    _chk(lib.liagpu_turn_detection_files(device, len(names), arr, feature_path.encode(), load_ext.encode(), label_path.encode(), label_ext.encode(),
                                         label.encode(), save_path.encode(), save_ext.encode(), mask.encode(), ct.c_double(frame_length), crit.encode(),
                                         ct.c_long(win_size), ct.c_long(win_step), ct.c_double(alpha), ct.c_double(min_llk), ct.c_double(max_llk),
                                         oo.ctypes.data_as(_lp), ob.ctypes.data_as(_lp), ol.ctypes.data_as(_lp), ct.c_long(max_segments)))
    return [(ob[oo[k]:oo[k + 1]].copy(), ol[oo[k]:oo[k + 1]].copy()) for k in range(len(names))]


def select_frames(energy, threshold, seg_begin, seg_len):
    """selectFrames (EnergyDetector.cpp:118-157) on the host: -> (begin[], length[], frames above the threshold)."""
    e = np.ascontiguousarray(energy, np.float32)
    b, l, bp, lp = _segs(seg_begin, seg_len)
    ob = np.zeros(max(16, len(e) + 1), np.int64); ol = np.zeros_like(ob); n = ct.c_long(0); cnt = ct.c_long(0)
    _chk(lib.liagpu_select_frames(e.ctypes.data_as(_fp), ct.c_long(len(e)), ct.c_double(threshold), bp, lp, ct.c_long(len(b)),
                                  ob.ctypes.data_as(_lp), ol.ctypes.data_as(_lp), ct.c_long(len(ob)), ct.byref(n), ct.byref(cnt)))
    return ob[:n.value].copy(), ol[:n.value].copy(), cnt.value


def gmm_tokenizer_files(world_path, prm_path, lbl_path, mask="", label="male", frame_length=0.01, top_c=1, min_llk=-200.0, max_llk=200.0,
                        matrix_path="", device=0):
    """GmmTokenizer from its files (GmmTokenizer.cpp:120-207): -> (symbols[n_selected], confusion[C, C]) with nBest = top_c."""
    dims = np.zeros(3, np.int64)
    sym = np.zeros(1 << 20, np.int64); n = ct.c_long(0)
    _chk(lib.liagpu_gmm_tokenizer_files(device, world_path.encode(), prm_path.encode(), lbl_path.encode(), mask.encode(), label.encode(),
                                        ct.c_double(frame_length), int(top_c), ct.c_double(min_llk), ct.c_double(max_llk),
                                        sym.ctypes.data_as(_lp), ct.c_long(len(sym)), ct.byref(n), None, dims.ctypes.data_as(_lp), b""))
    conf = np.zeros((int(dims[0]), int(dims[0])), np.int64)
    _chk(lib.liagpu_gmm_tokenizer_files(device, world_path.encode(), prm_path.encode(), lbl_path.encode(), mask.encode(), label.encode(),
                                        ct.c_double(frame_length), int(top_c), ct.c_double(min_llk), ct.c_double(max_llk),
                                        None, ct.c_long(0), None, conf.ctypes.data_as(_lp), dims.ctypes.data_as(_lp), matrix_path.encode()))
    return sym[:n.value].copy(), conf


def io_roundtrip(raw_in, raw_out, prm_in, prm_out, mask):
    dims = np.zeros(4, np.int64); mean0 = np.zeros(512); frame0 = np.zeros(512, np.float32)
    _chk(lib.liagpu_io_roundtrip(raw_in.encode(), raw_out.encode(), prm_in.encode(), prm_out.encode(), mask.encode(),
                                 dims.ctypes.data_as(_lp), mean0.ctypes.data_as(_dp), frame0.ctypes.data_as(_fp)))
    return dims, mean0[:dims[1]], frame0[:dims[3]]


def label_segments(lbl_path, label, frame_length=0.01):
    b = np.zeros(1024, np.int64); l = np.zeros(1024, np.int64); n = ct.c_long(0)
    _chk(lib.liagpu_label_segments(lbl_path.encode(), label.encode(), ct.c_double(frame_length), b.ctypes.data_as(_lp),
                                   l.ctypes.data_as(_lp), ct.c_long(1024), ct.byref(n)))
    return b[:n.value].copy(), l[:n.value].copy()


# ---- ComputeNorm (LIA_SpkDet/ComputeNorm): score normalisation on resident matrices and on NIST result files
NORM_TYPES = {"znorm": 0, "tnorm": 1, "ztnorm": 2, "tznorm": 3}


def _vp(a):
    """void* of a numpy array or a torch tensor (used in place), None -> NULL"""
    if a is None:
        return ct.c_void_p(0)
    if type(a).__module__.startswith("torch"):
        assert a.is_contiguous()
        return ct.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"] and a.dtype in (np.float64, np.uint8)
    return ct.c_void_p(a.ctypes.data)


def compute_norm(X, Z=None, T=None, ZT=None, norm_type="znorm", mean_mode=0, percent_h=0.0, percent_l=0.0, imp_models=None,
                 imp_segs=None, first_out=None, device=0):
    """liagpu::computeNorm: X [M, S] is normalised IN PLACE (numpy float64 or a torch CUDA tensor); Z [M, Nz], T [Nt, S],
    ZT [Nt, Nz] as the normType needs them.  first_out: None, or [M, S] for the t-normed (ztnorm) / z-normed (tznorm) scores.
    imp_models [Nt] / imp_segs [Nz]: the impostorIDList selection as bytes.  -> X"""
    M, S = X.shape
    Nt = T.shape[0] if T is not None else (ZT.shape[0] if ZT is not None else 0)
    Nz = Z.shape[1] if Z is not None else (ZT.shape[1] if ZT is not None else 0)
    im = None if imp_models is None else np.ascontiguousarray(imp_models, np.uint8)
    iz = None if imp_segs is None else np.ascontiguousarray(imp_segs, np.uint8)
    _chk(lib.liagpu_compute_norm(device, NORM_TYPES.get(norm_type, -1), int(mean_mode), ct.c_double(percent_h), ct.c_double(percent_l),
                                 ct.c_long(M), ct.c_long(S), ct.c_long(Nt), ct.c_long(Nz), _vp(X), _vp(Z), _vp(T), _vp(ZT), _vp(im), _vp(iz),
                                 _vp(first_out)))
    return X


def compute_norm_files(test_nist_file, output_base, norm_type="znorm", znorm_nist_file=None, tnorm_nist_file=None,
                       ztnorm_nist_file=None, impostor_id_list=None, mean_mode=0, percent_h=0.0, percent_l=0.0, fields=None, device=0):
    """liagpu::computeNormFiles: writes <output_base>.znorm / .tnorm / .ztnorm / .tznorm like the reference.  fields: the five
    positions (fieldGender, fieldName, fieldDecision, fieldSeg, fieldLLR), default 0 1 2 3 4."""
    e = lambda p: None if p is None else str(p).encode()
    fl = None if fields is None else (ct.c_int * 5)(*[int(v) for v in fields])
    _chk(lib.liagpu_compute_norm_files(device, norm_type.encode(), int(mean_mode), ct.c_double(percent_h), ct.c_double(percent_l),
                                       e(test_nist_file), e(znorm_nist_file), e(tnorm_nist_file), e(ztnorm_nist_file), e(impostor_id_list),
                                       e(output_base), fl))


def _ip(a):
    """void* of an index array: numpy (made contiguous by the caller) or a torch tensor, None -> NULL"""
    if a is None:
        return ct.c_void_p(0)
    if type(a).__module__.startswith("torch"):
        assert a.is_contiguous()
        return ct.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"]
    return ct.c_void_p(a.ctypes.data)


def _idx(a, dtype):
    if a is None or type(a).__module__.startswith("torch"):
        return a
    return np.ascontiguousarray(a, dtype)


def compute_norm_lists(x, line_model=None, line_seg=None, z=None, t=None, zt=None, norm_type="znorm", mean_mode=0, percent_h=0.0,
                       percent_l=0.0, first_out=None, device=0):
    """liagpu::computeNormLists: x [n] (numpy float64 or a torch CUDA tensor) is normalised IN PLACE.  line_model / line_seg [n]
    (int32) name the z / t distribution of every test line.  z, t, zt: None or a dict with "off" (host int64, ndist + 1), "scores"
    (float64), and optionally "pos" (int64, by slot) and "other" (int32, by slot: the zt distribution of the slot's second field, on z
    for ztnorm and on t for tznorm).  zt holds a distribution per impostor segment for ztnorm, per cohort model for tznorm.
    first_out: None, or [n] for the t-normed (ztnorm) / z-normed (tznorm) scores.  -> x"""
    keep = []
    nd = (ct.c_long * 3)(); ns = (ct.c_long * 3)()
    po = (ct.c_void_p * 3)(); ps = (ct.c_void_p * 3)(); pp = (ct.c_void_p * 3)(); pt = (ct.c_void_p * 3)()
    for i, l in enumerate((z, t, zt)):
        if l is None:
            continue
        off = np.ascontiguousarray(l["off"], np.int64)
        sc = l["scores"] if type(l["scores"]).__module__.startswith("torch") else np.ascontiguousarray(l["scores"], np.float64)
        pos, oth = _idx(l.get("pos"), np.int64), _idx(l.get("other"), np.int32)
        keep += [off, sc, pos, oth]
        nd[i] = len(off) - 1; ns[i] = int(sc.shape[0])
        po[i] = _ip(off).value; ps[i] = _vp(sc).value; pp[i] = _ip(pos).value; pt[i] = _ip(oth).value
    lm, ls = _idx(line_model, np.int32), _idx(line_seg, np.int32)
    _chk(lib.liagpu_compute_norm_lists(device, NORM_TYPES.get(norm_type, -1), int(mean_mode), ct.c_double(percent_h), ct.c_double(percent_l),
                                       ct.c_long(int(x.shape[0])), _vp(x), _ip(lm), _ip(ls), nd, po, ps, ns, pp, pt, _vp(first_out)))
    return x


def compute_norm_list_files(test_nist_file, output_base, norm_type="znorm", znorm_nist_file=None, tnorm_nist_file=None,
                            ztnorm_nist_file=None, impostor_id_list=None, mean_mode=0, percent_h=0.0, percent_l=0.0, fields=None, device=0):
    """liagpu::computeNormListFiles: compute_norm_files without its demand for full cross products -- sparse test lists, ragged
    cohorts, repeated pairs, as the reference's per-name DistribNorm takes them.  Writes the same files."""
    e = lambda p: None if p is None else str(p).encode()
    fl = None if fields is None else (ct.c_int * 5)(*[int(v) for v in fields])
    _chk(lib.liagpu_compute_norm_list_files(device, norm_type.encode(), int(mean_mode), ct.c_double(percent_h), ct.c_double(percent_l),
                                            e(test_nist_file), e(znorm_nist_file), e(tnorm_nist_file), e(ztnorm_nist_file),
                                            e(impostor_id_list), e(output_base), fl))


def load_compute_norm_lists(test_nist_file, norm_type="znorm", znorm_nist_file=None, tnorm_nist_file=None, ztnorm_nist_file=None,
                            impostor_id_list=None, fields=None):
    """liagpu::loadComputeNormLists (host only, opens no device) -> dict: "x", "line_model", "line_seg" (None where the normType does not
    use it) and per list "z" / "t" / "zt" a dict keys / off / scores / other (None without a first stage), ready for compute_norm_lists"""
    e = lambda p: None if p is None else str(p).encode()
    fl = None if fields is None else (ct.c_int * 5)(*[int(v) for v in fields])
    h = ct.c_void_p(0)
    _chk(lib.liagpu_norm_lists_load(norm_type.encode(), e(test_nist_file), e(znorm_nist_file), e(tnorm_nist_file), e(ztnorm_nist_file),
                                    e(impostor_id_list), fl, ct.byref(h)))
    try:
        sz = (ct.c_long * 13)()
        _chk(lib.liagpu_norm_lists_sizes(h, sz))
        out = {}
        for w, name in enumerate(("z", "t", "zt")):
            nd, nslot, has_other, nkey = [int(v) for v in sz[1 + 4 * w:5 + 4 * w]]
            off = np.zeros(nd + 1, np.int64); sc = np.zeros(nslot); oth = np.zeros(nslot, np.int32) if has_other else None
            keys = ct.create_string_buffer(max(nkey, 1))
            _chk(lib.liagpu_norm_lists_get(h, w, _ip(off) if nd else None, _ip(sc), _ip(oth), keys))
            out[name] = dict(keys=keys.raw[:nkey].decode().split("\n")[:-1], off=off, scores=sc, other=oth)
        n = int(sz[0])
        x = np.zeros(n); lm = np.zeros(n, np.int32); ls = np.zeros(n, np.int32)
        use_m, use_s = norm_type != "tnorm", norm_type != "znorm"
        _chk(lib.liagpu_norm_lists_lines(h, _ip(x), _ip(lm) if use_m else None, _ip(ls) if use_s else None))
        out.update(x=x, line_model=lm if use_m else None, line_seg=ls if use_s else None)
        return out
    finally:
        lib.liagpu_norm_lists_free(h)


def result_line(llr, client, test, gender="M", threshold=0.0, times=None, parse=None, fields=None):
    """-> (the line liagpu::resultLine writes, its fields as liagpu::parseResultLine reads them back: dict).  parse: another
    line to read instead; fields: the five field positions."""
    cap = 4096
    bufs = [ct.create_string_buffer(cap) for _ in range(4)]
    dec = ct.c_int(0); out = ct.c_double(0.0)
    fl = None if fields is None else (ct.c_int * 5)(*[int(v) for v in fields])
    st, en = times if times is not None else (0.0, 0.0)
    _chk(lib.liagpu_result_line(ct.c_double(llr), client.encode(), test.encode(), gender.encode(), ct.c_double(threshold),
                                int(times is not None), ct.c_double(st), ct.c_double(en), None if parse is None else parse.encode(), fl,
                                bufs[0], bufs[1], bufs[2], bufs[3], ct.c_long(cap), ct.byref(dec), ct.byref(out)))
    return bufs[0].value.decode(), dict(name=bufs[1].value.decode(), seg=bufs[2].value.decode(), gender=bufs[3].value.decode(),
                                        decision=dec.value, llr=out.value)
