"""The programme behind tests/test_gpu_ws_history.py: every frame-consuming entry point, the batched models and the front-end /
score calls of one context as an ordered list of named steps, run on small (judged) and large (dirtying) cases in several orders.
Plain numpy at import: the GPU is touched only inside a step.  No reference is involved -- a step returns EVERYTHING its call
produces and the test compares bits between contexts with different histories ("Results do not depend on a context's
history").

step        (ctx, handles, case, form) -> {name: array}.  form "host": numpy in and out (DevIn / DevOut / XView stage through the
            workspaces, float64 frames); form "device": torch tensors (float32 frames).  Every step ends with the deltas of the
            three counters; an output with rows the call must not touch is the whole buffer, pre-filled with a sentinel.
case        a row of SMALL or LARGE.  Data comes from the generators of the reference modules (gmm_ref.model / frames,
            mllr_ref.generate, energy_ref.energy_like); only the integer tables (segments, trials, runs) are laid out here.
sequence    an ordered list of (case, step, form) run on ONE context: see SEQUENCES.
"""
import functools
import time

import numpy as np

import energy_ref as er
import gmm_ref as gr
import mllr_ref
from elementwise_judge import SENTINEL, options
from test_gpu_gmm_elementwise import chunk_plan, layouts

SENT32 = -7.7e30                 # the sentinel of a float32 buffer
FORMS = ("host", "device")
COUNTERS = ("zero_llk_frames", "screened_frames", "topc_fallbacks")
WIDE = (-1e9, 1e9)
TORCH_SMALL_BLOCK = 2 << 20      # bytes of the block torch's caching allocator carves tensors below 1 MiB from
MLLR_MAX_DIM = 62                # mllr.hip: the augmented system must fit one 64 x 64 panel
Z_MB_530 = chunk_plan(530)[0]    # the smallest stored-likelihood scratch the library accepts at C = 530: chunks of 4096 frames

# ---------------------------------------------------------------------------------------------------------------- the cases
# name, (C, D, T, spread), segments, models, trials, ctop of determine_top / of llr_trials, utterance layouts of tv_stats, online
# files, energy files (frames), cohort length, list lengths, matrix (M, S), options of the whole case, planted frames
SMALL = (
    dict(name="s37x13x65", gcase=(37, 13, 65, 2.0), nseg=5, G=3, ntrial=6, ctops=(10, 17), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0),
    dict(name="s129x60x257", gcase=(129, 60, 257, 2.0), nseg=5, G=3, ntrial=6, ctops=(10, 17, 70), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0),
    dict(name="s40x97x66", gcase=(40, 97, 66, 0.5), nseg=5, G=3, ntrial=6, ctops=(10, 17), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0),
)
LARGE = (
    dict(name="L530x60x4300", gcase=(530, 60, 4300, 2.0), nseg=40, G=7, ntrial=60, ctops=(10, 17, 70, 100), trial_ctops=(17, 64), tv="bc",
         nfiles=3, energy=(5000, 2500, 0, 6001, 700, 9000, 1300), cohort=100003, lists=(100003, 7, 2049, 64), ms=(7, 11),
         opts={"z_scratch_mb": Z_MB_530, "timing": 1}, plant=True, online_rows=48000),
    dict(name="L96x101x700", gcase=(96, 101, 700, 0.5), nseg=40, G=7, ntrial=60, ctops=(10, 17, 64), trial_ctops=(17, 64), tv="abc", nfiles=3,
         energy=(5000, 2500, 0, 6001, 700, 9000, 1300), cohort=100003, lists=(100003, 7, 2049, 64), ms=(7, 11), opts={}, plant=True, online_rows=48000),
)
CASES = {c["name"]: c for c in SMALL + LARGE}
PLANT_HEAD = {1: np.nan, 5: np.inf, 11: -np.inf, 13: 1e30}     # row -> the value put into one of its dimensions (kind 1: screened)
PLANT_TAIL = {15: np.nan, 9: np.inf, 3: 1e30, 1: np.nan}       # rows counted back from T
FAR_HEAD, FAR_TAIL, FAR_VALUE = 7, 6, 3e17                     # whole rows of finite, absurd values (kind 2: largest logit ~ -1e37)


def planted(case):
    """-> (kind-1 rows {row: value}, kind-2 rows) of a case with plant = True, else two empty containers"""
    if not case["plant"]:
        return {}, ()
    T = case["gcase"][2]
    k1 = dict(PLANT_HEAD)
    k1.update({T - b: v for b, v in PLANT_TAIL.items()})
    return k1, (FAR_HEAD, T - FAR_TAIL)


@functools.lru_cache(maxsize=None)
def _frames(name, dtype_str):
    case = CASES[name]
    D = case["gcase"][1]
    x = gr.frames(case["gcase"], np.dtype(dtype_str).type).copy()
    k1, k2 = planted(case)
    for t, v in k1.items():
        x[t, (7 * t) % D] = v
    for t in k2:
        x[t, :] = FAR_VALUE
    x.setflags(write=False)
    return x


def frames(case, form):
    """host: float64 numpy (the staged copy in WS_X holds the raw values); device: float32"""
    return _frames(case["name"], "float64" if form == "host" else "float32")


def seg_table(case):
    """-> (seg_begin [nseg + 1], seg_model [nseg]): five segments are gmm_ref.ragged_bounds; more are equal cuts of [3, T - 1) with the
    second one emptied, so frames before the first and after the last belong to none"""
    T, nseg, G = case["gcase"][2], case["nseg"], case["G"]
    if nseg == 5:
        sb = gr.ragged_bounds(T)
    else:
        sb = 3 + (np.arange(nseg + 1, dtype=np.int64) * (T - 4)) // nseg
        sb[2] = sb[1]
    assert len(sb) == nseg + 1 and np.all(np.diff(sb) >= 0) and sb[-1] <= T
    assert G % 2
    return sb.astype(np.int64), ((np.arange(nseg) * 2 + 1) % G).astype(np.int32)


def trial_table(case):
    i = np.arange(case["ntrial"])
    return ((i * 3 + 1) % case["nseg"]).astype(np.int32), ((i * 2 + i // case["G"]) % case["G"]).astype(np.int32)


def file_table(case):
    """files of the online scan: a lead of unowned frames, an empty file; the large case's first file is 2500 frames (chunks of 1024)"""
    T = case["gcase"][2]
    first = min(2500, (T - 4) * 3 // 5)
    fb = np.array([3, 3 + first, 3 + first, T - 1], np.int64)
    assert len(fb) == case["nfiles"] + 1
    return fb


@functools.lru_cache(maxsize=None)
def _batch_models(name):
    case = CASES[name]
    ms = []
    for k in range(case["G"]):
        w, mean, iv = gr.model(case["gcase"], 0 if k == 0 else 10 + k)
        if k:
            iv = iv * np.exp(np.random.default_rng(100 + k).normal(0.0, 0.1, iv.shape))
        ms.append((w, mean, iv))
    return tuple(np.stack([m[i] for m in ms]) for i in range(3))


def sizes(case):
    """every quantity that sizes a workspace (tests/test_cpu_ws_history.py: dominance)"""
    C, D, T, _ = case["gcase"]
    return dict(C=C, D_tiles=(D + 3) // 4, T=T, nseg=case["nseg"], G=case["G"], ntrial=case["ntrial"], ctop=max(case["ctops"]),
                trial_ctop=max(case["trial_ctops"]), nfiles=case["nfiles"], energy_files=len(case["energy"]), energy_frames=max(case["energy"]),
                cohort=case["cohort"], list_len=max(case["lists"]), nlists=len(case["lists"]), M=case["ms"][0], S=case["ms"][1])


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _torch():
    import torch
    return torch


_KEEP = []                       # every device tensor of the running step: see dev()


def dev(a):
    """a device copy that lives until the step has synchronised its context (Step.run).  The contexts here own a private stream and a
    call on device tensors only enqueues: a tensor dropped right after the call goes back to torch's caching allocator, and the next
    tensor -- filled on torch's stream -- may land in it while the kernel that reads it is still queued"""
    t = _torch()
    out = t.from_numpy(np.array(a)).cuda()
    _KEEP.append(out)
    return out


def to(form, a):
    return a if form == "host" or a is None else dev(a)


def buf(form, shape, dtype=np.float64, fill=None):
    """an output buffer of the form, pre-filled with the sentinel of its dtype"""
    if fill is None:
        fill = SENT32 if np.dtype(dtype) == np.float32 else (SENTINEL if np.dtype(dtype) == np.float64 else -77)
    a = np.full(shape, fill, dtype)
    return a if form == "host" else dev(a)


def host(a):
    if a is None:
        return None
    if type(a).__module__.startswith("torch"):
        _torch().cuda.synchronize()
        return a.cpu().numpy()
    return np.array(a)


class Handles:
    """the model handles of one context, made on first use and kept (a used handle is part of the history); log: what the
    non-vacuity assertions read: (launches of k_llk_mfma, of k_stats_z) after the chunked calls, in programme order -- the first
    entry is the default path, the second the "stats_z 0" step (no k_stats_z there: its count is the earlier call's)"""

    def __init__(self, ctx):
        self.ctx, self.h, self.log = ctx, {}, {}

    def get(self, key, make):
        if key not in self.h:
            self.h[key] = make()
        return self.h[key]

    def world(self, case):
        return self.get((case["name"], "world"), lambda: self.ctx.gmm(*gr.model(case["gcase"])))

    def clients(self, case):
        return self.get((case["name"], "clients"), lambda: [self.ctx.gmm(*gr.model(case["gcase"], s)) for s in (5, 6)])

    def batch(self, case, shared=False):
        C, D = case["gcase"][:2]
        w, m, iv = _batch_models(case["name"])

        def make():
            b = self.ctx.gmm_batch(case["G"], C, D)
            return b.load_cov(w[0], m, np.ascontiguousarray(1.0 / iv[0])) if shared else b.load(w, m, iv)
        return self.get((case["name"], "batch", shared), make)

    def close(self):
        for v in self.h.values():
            for g in (v if isinstance(v, list) else [v]):
                g.close()
        self.h = {}


def counters(ctx, out):
    for k in COUNTERS:
        out["delta " + k] = np.array([ctx.set_option(k, 0)], np.float64)
    return out


class Step:
    def __init__(self, name, fn, reaches, forms=FORMS, opts=None, only=None):
        self.name, self.fn, self.reaches, self.forms, self.opts, self.only = name, fn, tuple(reaches), tuple(forms), dict(opts or {}), only

    def applies(self, case):
        return self.only is None or self.only(case)

    def run(self, ctx, handles, case, form):
        for k in COUNTERS:
            ctx.set_option(k, 0)
        opts = dict(case["opts"])
        opts.update(self.opts)
        try:
            with options(ctx, opts):
                out = self.fn(ctx, handles, case, form)
            ctx.sync()
            return counters(ctx, {k: host(v) for k, v in out.items() if v is not None})
        finally:
            del _KEEP[:]


# ---------------------------------------------------------------------------------------------------------------- Gmm
def s_llk(ctx, h, case, form):
    g, x = h.world(case), to(form, frames(case, form))
    T = case["gcase"][2]
    out, sums = buf(form, (T,)), buf(form, (2,), fill=0.0)
    g.llk(x, *WIDE, out=out, sums=sums)
    clamped = g.llk(x)
    sb, _ = seg_table(case)
    means = ctx.segment_means(dev(np.stack([clamped, host(out)])), sb)
    return {"llk": out, "sums": sums, "llk clamped": clamped, "segment means": means}


def s_occ(ctx, h, case, form):
    return {"occ": h.world(case).occ(to(form, frames(case, form)))}


def s_em(ctx, h, case, form):
    g, x = h.world(case), to(form, frames(case, form))
    acc = buf(form, (g.em_acc_len(),), fill=0.0)
    g.em_accumulate(x, weight=0.5, acc=acc)
    if case["opts"].get("timing"):
        h.log.setdefault((case["name"], "em", form), []).append((ctx.kernel_launches("k_llk_mfma"), ctx.kernel_launches("k_stats_z")))
    first = host(acc)
    g.em_accumulate(x, weight=0.5, acc=acc)
    w0, mean0, iv0 = gr.model(case["gcase"])
    w, mean, cov = g.em_get(acc, to(form, mean0), to(form, np.ascontiguousarray(1.0 / iv0)))      # the M-step of the accumulator
    signal = to(form, np.ascontiguousarray((1.0 / iv0).mean(0)))
    cov2 = to(form, cov.copy())
    _, counts = ctx.variance_control(cov2, 0.9, 1.1, signal, g.C, g.D)
    return {"acc w=0.5": first, "acc w=0.5 twice": acc, "em_get w": w, "em_get mean": mean, "em_get cov": cov, "variance_control cov": cov2,
            "variance_control counts": counts}


def s_tv(ctx, h, case, form):
    g, x = h.world(case), to(form, frames(case, form))
    C, D, T, _ = case["gcase"]
    out = {}
    for name, ub in layouts(T):
        if name not in case["tv"]:
            continue
        U = len(ub) - 1
        N, F = buf(form, (U, C)), buf(form, (U, C * D))
        g.tv_stats(x, ub, N, F)
        if case["opts"].get("timing") and name == "b":
            h.log.setdefault((case["name"], "tv", form), []).append((ctx.kernel_launches("k_llk_mfma"), ctx.kernel_launches("k_stats_z")))
        out["N(%s)" % name], out["F(%s)" % name] = N, F
    return out


def s_tv_lines(ctx, h, case, form):
    g, x = h.world(case), to(form, frames(case, form))
    C, D, T, _ = case["gcase"]
    sb, _ = seg_table(case)
    fb = sb[:6] if len(sb) > 6 else sb                    # five files (one empty); a file on two lines, a line of one file, an empty line
    lines = [[0, 2], [3], [], [4, 2, 0]]
    N, F = buf(form, (len(lines), C)), buf(form, (len(lines), C * D))
    g.tv_stats_lines(x, np.r_[fb[:-1], T] if len(sb) > 6 else fb, lines, N, F)
    return {"N": N, "F": F}


def _tops(case):
    return [c for c in case["ctops"] if c <= case["gcase"][0]]


def _determine(ctx, h, case, form, complete):
    g, x = h.world(case), to(form, frames(case, form))
    out = {}
    for ctop in _tops(case):
        d = g.llk_determine_top(x, ctop, complete, *WIDE)
        out.update({"top%d %s" % (ctop, k): v for k, v in d.items()})
    return out


def s_top_complete(ctx, h, case, form):
    return _determine(ctx, h, case, form, True)


def s_top_partial(ctx, h, case, form):
    return _determine(ctx, h, case, form, False)


def s_use_top(ctx, h, case, form):
    g, cl, x = h.world(case), h.clients(case), to(form, frames(case, form))
    out = {}
    for ctop in _tops(case):
        for complete in (True, False):
            d = g.llk_determine_top(x, ctop, complete, *WIDE)
            tag = "top%d %s" % (ctop, "complete" if complete else "partial")
            out[tag + " use_top"] = cl[0].llk_use_top(x, d["idx"], d["nontop_llk"], complete, *WIDE)
            out[tag + " use_top_multi"] = type(g).llk_use_top_multi(cl, x, d["idx"], d["nontop_llk"], complete)
    return out


@functools.lru_cache(maxsize=None)
def _offsets(name):
    case = CASES[name]
    w, mean, iv = gr.model(case["gcase"])
    return np.ascontiguousarray(gr.model(case["gcase"], 21)[1] - mean)       # [C, D]: a client's shift of every mean


def s_feat_comp(ctx, h, case, form):
    g = h.world(case)
    C, D, T, _ = case["gcase"]
    off = to(form, _offsets(case["name"]))
    x32 = _frames(case["name"], "float32").copy()
    inplace = to(form, x32)
    g.feat_compensate(inplace, off, out=inplace)                              # float32 in place
    wide = buf(form, (T, D + 3), np.float32)
    g.feat_compensate(to(form, _frames(case["name"], "float64")), off, out=wide[:, :D])     # float64 -> float32, row-strided
    return {"f32 in place": inplace, "f64 to f32 strided": wide}


def s_feat_map(ctx, h, case, form):
    g = h.world(case)
    w, mean, iv = gr.model(case["gcase"])
    ci_mean, ci_iv = gr.model(case["gcase"], 22)[1], _batch_models(case["name"])[2][1]
    tabs = [to(form, np.ascontiguousarray(a)) for a in (mean, 1.0 / iv, ci_mean, 1.0 / ci_iv)]
    out, best = g.feat_map(*tabs, to(form, frames(case, form)))
    return {"out": out, "best": best}


def s_moments(ctx, h, case, form):
    D = case["gcase"][1]
    acc = buf(form, (2 * D + 1,), fill=0.0)
    x = to(form, frames(case, form))
    ctx.frame_moments(x, acc)
    return {"acc": acc, "unusable frames": np.array([ctx.count_unusable_frames(x)], np.float64)}


def s_topgauss(ctx, h, case, form):
    g, x = h.world(case), to(form, frames(case, form))
    out = {}
    for tag, cap, share in (("mass 0.9", 20, 0.9), ("fixed 5", 17, 5.0)):
        d = g.topgauss_compute(x, cap, share, True, *WIDE)
        d["n_capped"] = np.array([d["n_capped"]], np.float64)
        out.update({"%s %s" % (tag, k): v for k, v in d.items()})
    return out


def s_em_tv_stats_z0(ctx, h, case, form):
    out = {"em " + k: v for k, v in s_em(ctx, h, case, form).items()}
    out.update({"tv " + k: v for k, v in s_tv(ctx, h, case, form).items()})
    return out


# ---------------------------------------------------------------------------------------------------------------- GmmBatch
def s_batch_llk(ctx, h, case, form):
    b, x = h.batch(case), to(form, frames(case, form))
    sb, sm = seg_table(case)
    out, ssum = buf(form, (case["gcase"][2],)), buf(form, (len(sm),))
    b.llk(x, sb, sm, *WIDE, out=out, seg_sum=ssum)
    return {"llk": out, "seg_sum": ssum}


def s_batch_tv(ctx, h, case, form):
    b, x = h.batch(case), to(form, frames(case, form))
    C, D = case["gcase"][:2]
    sb, sm = seg_table(case)
    N, F, sl = buf(form, (len(sm), C)), buf(form, (len(sm), C * D)), buf(form, (len(sm), 2))
    b.tv_stats(x, sb, sm, N, F, sl)
    return {"N": N, "F": F, "seg_llk": sl}


def s_batch_em(ctx, h, case, form):
    b, x = h.batch(case), to(form, frames(case, form))
    C, D = case["gcase"][:2]
    sb, sm = seg_table(case)
    N, F, S, sl = buf(form, (len(sm), C)), buf(form, (len(sm), C * D)), buf(form, (len(sm), C * D)), buf(form, (len(sm), 2))
    b.em_stats(x, sb, sm, N, F, S, sl)
    return {"N": N, "F": F, "S": S, "seg_llk": sl}


def s_batch_feat_comp(ctx, h, case, form):
    b = h.batch(case)
    C, D, T, _ = case["gcase"]
    sb, sm = seg_table(case)
    offs = np.stack([_offsets(case["name"]) * (1.0 + 0.25 * k) for k in range(case["G"])])
    out = buf(form, (T, D), np.float32)
    b.feat_compensate(to(form, frames(case, form)), sb, sm, to(form, offs), out=out)
    return {"out": out}


def _trials(ctx, h, case, form, shared):
    b, world, x = h.batch(case, shared), h.world(case), to(form, frames(case, form))
    sb, _ = seg_table(case)
    ts, tm = trial_table(case)
    out = {}
    for ctop in case["trial_ctops"]:
        for complete in (True, False):
            llr, cm, wm = buf(form, (len(ts),)), buf(form, (len(ts),)), buf(form, (len(sb) - 1,))
            b.llr_trials(world, x, sb, ts, tm, ctop, complete, llr=llr, client_mean=cm, world_mean=wm)
            tag = "ctop%d %s " % (ctop, "complete" if complete else "partial")
            out[tag + "llr"], out[tag + "client_mean"], out[tag + "world_mean"] = llr, cm, wm
    return out


def s_trials_shared(ctx, h, case, form):
    return _trials(ctx, h, case, form, True)


def s_trials_per_model(ctx, h, case, form):
    return _trials(ctx, h, case, form, False)


@functools.lru_cache(maxsize=None)
def _stats(name):
    """statistics rows of G clients (mllr_ref.generate: a Gaussian of occupancy 0 and NaN first-order sums per client)"""
    case = CASES[name]
    C, D = case["gcase"][:2]
    s = mllr_ref.generate(case["G"], C, D, seed=C + D)
    N, F = s["N"], s["F"]
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.ascontiguousarray((F.reshape(-1, C, D) ** 2 / N[:, :, None] + N[:, :, None] * s["cov0"][None]).reshape(F.shape))
    w0 = gr.model(case["gcase"])[0]
    return dict(N=N, F=F, S=S, count=np.ascontiguousarray(N.sum(1)), w0=w0, mean0=s["mean0"], cov0=s["cov0"])


def s_map_adapt(ctx, h, case, form):
    b, s = h.batch(case), _stats(case["name"])
    t = lambda k: to(form, s[k])
    out = {}
    for method in ("MAPOccDep", "MAPConst2"):
        m, w = b.map_adapt(t("N"), t("F"), t("count"), t("w0"), t("mean0"), t("mean0"), method, True, True, (14.0, 15.0, 16.0), 0.6)
        out[method + " mean"], out[method + " w"] = m, w
    return out


def s_map_adapt_full(ctx, h, case, form):
    b, s = h.batch(case), _stats(case["name"])
    t = lambda k: to(form, s[k])
    m, c, w, st = b.map_adapt_full(t("N"), t("F"), t("S"), t("count"), t("w0"), t("mean0"), t("cov0"), t("mean0"), t("cov0"), "MAPOccDep", True, True,
                                   True, (14.0, 15.0, 16.0), 0.6)
    return {"mean": m, "cov": c, "w": w, "status": st}


def s_normalize(ctx, h, case, form):
    b = h.batch(case)
    G = case["G"]
    w, m, iv = _batch_models(case["name"])
    mean, cov = dev(m.reshape(G, -1).copy()), dev((1.0 / iv).reshape(G, -1).copy())
    b.normalize(to(form, w), mean, cov, 2, False)
    m1, c1 = dev(m.reshape(G, -1).copy()), dev((1.0 / iv).reshape(G, -1).copy())
    b.normalize(to(form, w[0].copy()), m1, c1, 1, True)
    return {"mean": mean, "cov": cov, "mean (mean only, shared w)": m1, "cov (mean only, shared w)": c1}


def s_mllr(ctx, h, case, form):
    b, s = h.batch(case), _stats(case["name"])
    W, means, st = b.mllr_adapt(to(form, s["N"]), to(form, s["F"]), to(form, s["mean0"]), to(form, s["cov0"]))
    return {"W": W, "means": means, "status": st}


# ---------------------------------------------------------------------------------------------------------------- Context
def _norm_runs(case):
    sb, _ = seg_table(case)
    nseg, G = case["nseg"], case["G"]
    rows = [(int(sb[s]), int(sb[s + 1] - sb[s]), s * G // nseg) for s in range(nseg) if sb[s + 1] > sb[s]]
    return np.array(rows, np.int64)


def s_normfeat(ctx, h, case, form):
    C, D, T, _ = case["gcase"]
    G = case["G"]
    x = dev(_frames(case["name"], "float32"))
    runs = _norm_runs(case)
    acc = buf(form, (G, 2 * D + 1), fill=0.0)
    ctx.frame_moments_groups(x, to(form, runs), G, acc)
    mean, std = buf(form, (G, D)), buf(form, (G, D))
    ctx.frame_moments_stats(acc, D, mean, std)
    out = buf("device", (T, D), np.float32)
    ctx.feat_norm_apply(x, to(form, runs), mean, std, out=out)
    return {"acc": acc, "mean": mean, "std": std, "out": out}


def s_norm_online(ctx, h, case, form):
    """with a device table the call never reads the file bounds back: it sizes WS_NORM_STATE / WS_NORM_DECAY by the frames that fit
    between x and the end of the ALLOCATION that holds x.  A small tensor lives in a 2 MiB block of torch's caching allocator, so the
    judged cases ask for up to TORCH_SMALL_BLOCK / (4 D) frames' worth; the large cases' frames are the head of a resident buffer of
    case["online_rows"] rows (what a feature server holds), which bounds more"""
    C, D, T, _ = case["gcase"]
    x = _frames(case["name"], "float32")
    if case["online_rows"]:
        x = np.concatenate([x, np.zeros((case["online_rows"] - T, D), np.float32)])
    x = dev(x)[:T]
    out = buf("device", (T, D), np.float64)
    ctx.feat_norm_online(x, to(form, file_table(case)), 300, 40, out=out)
    return {"out": out}


def s_runs(ctx, h, case, form):
    C, D, T, _ = case["gcase"]
    x = dev(_frames(case["name"], "float32"))
    nr = _norm_runs(case)
    dst = np.concatenate([[1], 1 + np.cumsum(nr[:-1, 1])])
    runs = np.stack([nr[:, 0], dst, nr[:, 1]], 1).astype(np.int64)
    packed = buf("device", (int(nr[:, 1].sum()) + 2, D), np.float32)
    ctx.gather_runs(x, to(form, runs), packed)
    back = buf("device", (T, D), np.float32)
    ctx.scatter_runs(back, to(form, runs), packed)
    pick = (np.arange(0, T, 3)[::-1]).astype(np.int64)
    picked = buf("device", (len(pick), D), np.float32)
    ctx.gather_frames(x, to(form, pick), picked)
    return {"gathered": packed, "scattered": back, "gather_frames": picked}


def s_energy(ctx, h, case, form):
    cols, runs, t0 = [], [], 2
    for f, n in enumerate(case["energy"]):
        cols.append(er.energy_like(n, 40 + f))
        if n:
            runs.append((t0, n, f))
        t0 += n + 1
    col = np.full(t0 + 1, 1e30, np.float32)
    for (a, n, f) in runs:
        col[a:a + n] = cols[f]
    wide = np.full((len(col), 3), 1e30, np.float32)
    wide[:, 1] = col
    xd = dev(wide)
    r = ctx.energy_detect(xd[:, 1:2], to(form, np.array(runs, np.int64)), len(case["energy"]), C=3, nb_train_it=6, alpha=0.25)
    return dict(r)


@functools.lru_cache(maxsize=None)
def _scores(name):
    case = CASES[name]
    M, S = case["ms"]
    n = case["cohort"]
    val = lambda shape, seed: er.energy_like(int(np.prod(shape)), seed).astype(np.float64).reshape(shape)
    return dict(scores=val((M, S), 71), zc=val((M, n), 72), tc=val((n, S), 73), lst=val((sum(case["lists"]),), 74), trials=val((case["ntrial"],), 75))


def s_score_matrix(ctx, h, case, form):
    s = _scores(case["name"])
    M, S = case["ms"]
    zc, tc = to(form, s["zc"]), to(form, s["tc"])
    out = {}
    for tag, kw in (("trimmed", dict(mean_mode=0, percent_h=0.1, percent_l=0.05)), ("median", dict(mean_mode=1, percent_h=0.1, percent_l=0.05)),
                    ("plain", dict(mean_mode=0))):
        rm, rs, cm, cs = buf(form, (M,)), buf(form, (M,)), buf(form, (S,)), buf(form, (S,))
        ctx.score_cohort_stats(zc, 0, out_mean=rm, out_std=rs, **kw)
        ctx.score_cohort_stats(tc, 1, out_mean=cm, out_std=cs, **kw)
        sc, first = to(form, s["scores"].copy()), buf(form, (M, S))
        ctx.score_normalize(sc, 2, rm, rs, cm, cs, first_out=first)           # NORM_ZT
        out.update({tag + " row_mean": rm, tag + " row_std": rs, tag + " col_mean": cm, tag + " col_std": cs, tag + " zt": sc, tag + " first": first})
    return out


def s_score_lists(ctx, h, case, form):
    s = _scores(case["name"])
    off = np.concatenate([[0], np.cumsum(case["lists"])]).astype(np.int64)
    nd = len(case["lists"])
    lst = to(form, s["lst"])
    out = {}
    for tag, kw in (("trimmed", dict(mean_mode=0, percent_h=0.1, percent_l=0.05)), ("median", dict(mean_mode=1, percent_h=0.1, percent_l=0.05)),
                    ("plain", dict(mean_mode=0))):
        m, sd = buf(form, (nd,)), buf(form, (nd,))
        ctx.score_list_stats(off, lst, out_mean=m, out_std=sd, **kw)
        rid = (np.arange(case["ntrial"]) % nd).astype(np.int32)
        sc = to(form, s["trials"].copy())
        ctx.score_normalize_list(sc, 0, to(form, rid), m, sd)                 # NORM_Z
        out.update({tag + " mean": m, tag + " std": sd, tag + " z": sc})
    return out


# ---------------------------------------------------------------------------------------------------------------- the programme
_use = ("gmmiv_llk_determine_top", "gmmiv_llk_use_top", "gmmiv_llk_use_top_multi")
_em = ("gmmiv_em_accumulate", "gmmiv_em_get", "gmmiv_variance_control")
_mllr_ok = lambda case: case["gcase"][1] <= MLLR_MAX_DIM
PROGRAMME = (
    Step("llk", s_llk, ("gmmiv_llk", "gmmiv_segment_means")),
    Step("occ", s_occ, ("gmmiv_occ",)),
    Step("em_accumulate", s_em, _em),
    Step("tv_stats", s_tv, ("gmmiv_tv_stats",)),
    Step("tv_stats_lines", s_tv_lines, ("gmmiv_tv_stats_lines",)),
    Step("determine_top complete", s_top_complete, ("gmmiv_llk_determine_top",)),
    Step("determine_top partial", s_top_partial, ("gmmiv_llk_determine_top",)),
    Step("use_top", s_use_top, _use),
    Step("topgauss", s_topgauss, ("gmmiv_topgauss_compute",)),
    Step("feat_compensate", s_feat_comp, ("gmmiv_feat_compensate",)),
    Step("feat_map", s_feat_map, ("gmmiv_feat_map",)),
    Step("frame_moments", s_moments, ("gmmiv_frame_moments", "gmmiv_count_unusable_frames")),
    Step("em + tv [stats_z 0]", s_em_tv_stats_z0, _em + ("gmmiv_tv_stats",), opts={"stats_z": 0}),
    Step("determine_top [topc_fused 0]", s_top_complete, ("gmmiv_llk_determine_top",), opts={"topc_fused": 0}),
    Step("determine_top [topc_fused 0 topc_z 0]", s_top_partial, ("gmmiv_llk_determine_top",), opts={"topc_fused": 0, "topc_z": 0}),
    Step("use_top [topc_use_lanes 1]", s_use_top, _use, opts={"topc_use_lanes": 1}),
    Step("batch llk", s_batch_llk, ("gmmiv_llk_models",)),
    Step("batch tv_stats", s_batch_tv, ("gmmiv_tv_stats_models",)),
    Step("batch em_stats", s_batch_em, ("gmmiv_em_stats_models",)),
    Step("batch feat_compensate", s_batch_feat_comp, ("gmmiv_feat_compensate_models",)),
    Step("llr_trials shared tables", s_trials_shared, ("gmmiv_llr_trials",)),
    Step("llr_trials per-model tables", s_trials_per_model, ("gmmiv_llr_trials",)),
    Step("map_adapt", s_map_adapt, ("gmmiv_map_adapt_models",)),
    Step("map_adapt_full", s_map_adapt_full, ("gmmiv_map_adapt_models_full",)),
    Step("normalize", s_normalize, ("gmmiv_normalize_models",)),
    Step("mllr_adapt", s_mllr, ("gmmiv_mllr_adapt_models",), only=_mllr_ok),
    Step("normfeat", s_normfeat, ("gmmiv_frame_moments_groups", "gmmiv_frame_moments_stats", "gmmiv_feat_norm_apply")),
    Step("feat_norm_online", s_norm_online, ("gmmiv_feat_norm_online",)),
    Step("gather + scatter runs", s_runs, ("gmmiv_gather_runs", "gmmiv_scatter_runs", "gmmiv_gather_frames")),
    Step("energy_detect", s_energy, ("gmmiv_energy_train", "gmmiv_energy_select")),
    Step("score matrix", s_score_matrix, ("gmmiv_score_cohort_stats", "gmmiv_score_normalize")),
    Step("score lists", s_score_lists, ("gmmiv_score_list_stats", "gmmiv_score_normalize_list")),
)
STEPS = {s.name: s for s in PROGRAMME}
# reached by the plumbing of every sequence (Handles, Step.run, nan_calls, workspace_table), not by one step
PLUMBING = ("gmmiv_ctx_create", "gmmiv_ctx_destroy", "gmmiv_ctx_sync", "gmmiv_ctx_set_option", "gmmiv_ctx_kernel_launches", "gmmiv_ctx_workspace_bytes",
            "gmmiv_gmm_create", "gmmiv_gmm_destroy", "gmmiv_gmm_batch_create", "gmmiv_gmm_batch_load", "gmmiv_gmm_batch_load_cov",
            "gmmiv_gmm_batch_destroy", "gmmiv_score_cosine", "gmmiv_dgemm")
# reached by the used-handle tests of tests/test_gpu_ws_history.py: C entry point -> the binding's method those tests call
HANDLE_TESTS = {"gmmiv_gmm_set": "set", "gmmiv_gmm_set_cov": "set_cov", "gmmiv_gmm_batch_packed": "packed"}
_BACKEND = "history case in test_gpu_backend_elementwise / test_gpu_estimation_elementwise"
_NO_WS = "no workspace: no `scratch(` in its body"
_COMM = "communicator"
_IVEC = "i-vector back end: not in this programme's families and no history case of its own yet"
EXEMPT_REASONS = (_BACKEND, _NO_WS, _COMM, _IVEC)
EXEMPT = {
    "gmmiv_score_mahalanobis": _BACKEND, "gmmiv_score_twocov": _BACKEND, "gmmiv_score_plda": _BACKEND, "gmmiv_score_twocov_mix_part": _BACKEND,
    "gmmiv_plda_precompute": _BACKEND,
    "gmmiv_ctx_set_hook": _NO_WS, "gmmiv_ctx_last_kernel_ms": _NO_WS, "gmmiv_ctx_kernel_ms": _NO_WS, "gmmiv_trial_piece": _NO_WS,
    "gmmiv_ctx_stream": _NO_WS,
    "gmmiv_comm_create": _COMM,
}
EXEMPT.update({"gmmiv_" + n: _IVEC for n in (
    "tv_subtract_m", "tv_subtract_m_to", "tv_tett", "tv_estimate_w", "tv_estimate_a_and_c", "tv_update_t", "tv_min_divergence", "tv_orthonormalize_t",
    "tv_norm_statistics", "tv_subtract_m_plus_tw", "tv_norm_t", "tv_weighted_cov", "tv_approximate_tctc", "tv_estimate_w_ubm_weight",
    "tv_estimate_w_eigen", "iv_normalize", "dev_means", "dev_cov_mat", "dev_wccn_chol", "dev_mahalanobis", "dev_scatter_mat", "sym_eigen",
    "dev_efr_matrix", "dev_lda", "plda_em_iteration", "twocov_model", "score_apply_trials", "jfa_subtract", "jfa_subtract_sessions", "jfa_estimate_z",
    "jfa_estimate_z_and_d")})


# ---------------------------------------------------------------------------------------------------------------- sequences
def plan(cases, reverse=False):
    """(case, step, form) in programme order, case by case"""
    items = [(c, s, f) for c in cases for s in PROGRAMME if s.applies(c) for f in s.forms]
    return items[::-1] if reverse else items


SEQUENCES = {
    "fresh_small": ((SMALL, False),),
    "fresh_small_again": ((SMALL, False),),
    "fresh_large": ((LARGE, False),),
    "large_then_small": ((LARGE, False), (SMALL, False)),
    "large_then_small_reversed": ((LARGE, False), (SMALL, True)),
    "small_then_large": ((SMALL, False), (LARGE, False)),
}
NAN_SHAPE = (33, 45, 47)         # score_cosine on NaN vectors of (33, 45) x (33, 47), as test_gpu_backend_elementwise.py


def nan_calls(ctx):
    """the two NaN-as-data calls that finish a large pass: the shared WS_T* slots hold NaN afterwards -> True when both returned NaN"""
    t = _torch()
    dim, M, S = NAN_SHAPE
    sc = ctx.score_cosine(np.full((dim, M), np.nan), np.full((dim, S), np.nan))
    A = t.full((130, 70), float("nan"), dtype=t.float64, device="cuda")
    B = t.full((70, 90), float("nan"), dtype=t.float64, device="cuda")
    Cm = t.zeros((130, 90), dtype=t.float64, device="cuda")
    ctx.dgemm(0, 0, 1.0, A, B, 0.0, Cm)
    t.cuda.synchronize()
    return bool(np.isnan(sc).all()) and bool(t.isnan(Cm).all().item())


def workspace_table(ctx):
    return [ctx.workspace_bytes(i) for i in range(64)]


def run_sequence(name, moved=None):
    """one context, the passes of SEQUENCES[name] -> dict(results {(case, step, form): outputs}, seconds {...}, ws [(pass, table)],
    nan_ok, log, total).  moved: {step name: options} set for that step of the FIRST pass only and put back after it"""
    from lia_ral_amd import capi
    ctx = capi.Context(0)
    h = Handles(ctx)
    res = dict(results={}, seconds={}, ws=[], nan_ok=None, log=h.log)
    t_all = time.perf_counter()
    try:
        for k, (cases, reverse) in enumerate(SEQUENCES[name]):
            for case, step, form in plan(cases, reverse):
                t0 = time.perf_counter()
                with options(ctx, (moved or {}).get(step.name, {}) if k == 0 else {}):
                    res["results"][(case["name"], step.name, form)] = step.run(ctx, h, case, form)
                res["seconds"][(case["name"], step.name, form)] = time.perf_counter() - t0
            if cases is LARGE:
                ok = nan_calls(ctx)
                res["nan_ok"] = ok if res["nan_ok"] is None else (res["nan_ok"] and ok)
            res["ws"].append(("large" if cases is LARGE else "small", workspace_table(ctx)))
    finally:
        h.close()
        ctx.close()
    res["total"] = time.perf_counter() - t_all
    return res
