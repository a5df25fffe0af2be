"""The programme behind tests/test_gpu_ws_history.py: every frame-consuming entry point, the batched models, the front-end / score
calls -- windowed NormFeat (include/gmmiv_feat_window.h) and TurnDetection (include/gmmiv_turn.h) among them -- and the i-vector back
end (T-matrix chain, development set, PLDA, scoring rules, JFA) of one context as an ordered list of 54 named steps, run on small
(judged) and large (dirtying) cases in several orders.
Plain numpy at import: the GPU is touched only inside a step.  No reference is involved -- a step returns EVERYTHING its call
produces and the test compares bits between contexts with different histories ("Results do not depend on a context's
history").

step        (ctx, handles, case, form) -> {name: array}.  form "host": numpy in and out (DevIn / DevOut / XView stage through the
            workspaces, float64 frames); form "device": torch tensors (float32 frames).  Every step ends with the deltas of the
            three counters; an output with rows the call must not touch is the whole buffer, pre-filled with a sentinel.
case        a row of SMALL or LARGE.  Data comes from the generators of the reference modules (gmm_ref.model / frames,
            mllr_ref.generate, energy_ref.energy_like, tv_ref.statistics, backend_ref.score_case / ivn_inputs / dev_inputs / jfa_inputs,
            estimation_ref.em_inputs / precompute_inputs / eigen_matrix / lda_inputs / twocov_inputs / ortho_inputs); only the integer
            tables (segments, trials, runs; run_table / turn_table for the label segments of windowed NormFeat and TurnDetection) and
            the inputs of the dirtying back-end shapes -- the same recipes at sizes the reference tables do not hold -- are laid out here.
sequence    an ordered list of (case, step, form) run on ONE context: see SEQUENCES.
"""
import functools
import time

import numpy as np

import backend_ref as br
import energy_ref as er
import estimation_ref as es
import gmm_ref as gr
import iv_trials_ref as ivr
import mllr_ref
import normwin_ref as nw
import turn_ref as tn
import tv_ref as tr
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
# The i-vector part of a case (its "iv" entry).  tv: the T-matrix chains (C, D, R, U); dev: a development set -- a name of
# backend_ref.DEV_CASES, or (dim, speakers, sessions of the longest speaker); plda: (dim, rf, rg) of plda_precompute; score: (dim, M, S)
# of the scoring rules, rf = dim for PLDA; ivn: (dim_in, dim_out, n); jfa: (C, D, R) on backend_ref's 11 speakers and 24 sessions, or
# (C, D, R, sessions per speaker); eig: the order of sym_eigen / dev_efr_matrix / dev_lda / twocov_model; ortho: keys of
# estimation_ref.ortho_inputs (the "row at 5e-5" ones take the step route); em: names of estimation_ref.EM_CASES, or (dim, rf, rg) on
# the session counts of the case's own development set; gemm: (M, N, K, nz) of the split-K product, NT, K layers of 48 and a short last one
# ((128, 80, 112) and (256, 240, 208) qualify for the 128 x 80 tile of "gemm_nt80": full row tiles, N = k 80, K = k 16).
# Judged: every shape is a row of the reference modules' own tables, so each has a per-element verdict elsewhere.  Odd R = 35 takes
# the GEMM-built SPD route, even R = 70 the left-looking kernels at an order that is no multiple of 32; (16, 12, 40, 75) under tv_batch
# 16 is two calls of 16 + 16 + 5 and 16 + 16 + 6 utterances; (6, 4, 70, 65) crosses the 64 utterances of the narrow column sum; both scoring counts of
# the second and third case are odd (the even-stride pad copy on either side).
IV_SMALL = (
    dict(tv=((5, 3, 2, 7),), dev="3x[1,2,1]", plda=(5, 2, 1), score=(5, 3, 7), ivn=(5, 3, 7), jfa=(3, 1, 1), eig=2, ortho=((2, 3, "plain"),),
         em=("5x2x1 [1,2,1,3]",), gemm=(5, 3, 100, 3)),
    dict(tv=((8, 12, 35, 20),), dev="33x257", plda=(33, 7, 3), score=(33, 33, 31), ivn=(60, 40, 33), jfa=(6, 5, 3), eig=33,
         ortho=((33, 520, "plain"),), em=("33x7x3 257 speakers",), gemm=(128, 80, 112, 3)),
    dict(tv=((16, 12, 40, 75), (6, 4, 70, 65)), dev="8x[600,1,2]", plda=(34, 5, 5), score=(130, 131, 129), ivn=(33, 33, 130), jfa=(5, 13, 7), eig=65,
         ortho=((24, 1000, "plain"), (24, 1000, "row at 5e-5")), em=("34x5x5 [3]*40", "8x3x2 [600,1,2]"), gemm=(130, 160, 100, 3)),
)
# Dirtying, all finite: each dominates every judged set in every quantity of sizes().  (36, 60, 92, 129) is a row of tv_ref.ESTEP_CASES;
# its odd companion there, (8, 12, 91, 129), has fewer Gaussians than the judged 16 and is widened to (18, 14, 91, 129).
JFA_SESSIONS_LARGE = ((2, 0, 5, 13, 1, 3, 0, 0, 7, 1, 2, 4, 1), (1, 3, 0, 11, 2, 2, 0, 6, 1, 5, 1, 0, 3, 2, 4))
IV_LARGE = (
    dict(tv=((36, 60, 92, 129),), dev=(35, 259, 601), plda=(67, 9, 11), score=(133, 263, 259), ivn=(61, 43, 263), jfa=(7, 15, 9, JFA_SESSIONS_LARGE[0]),
         eig=67, ortho=((35, 1003, "plain"), (35, 1003, "row at 5e-5")), em=((35, 9, 7),), gemm=(256, 240, 208, 5)),
    dict(tv=((18, 14, 91, 129),), dev=(37, 261, 603), plda=(69, 11, 7), score=(131, 259, 261), ivn=(67, 41, 259), jfa=(9, 14, 8, JFA_SESSIONS_LARGE[1]),
         eig=69, ortho=((37, 1100, "plain"), (37, 1100, "row at 5e-5")), em=((37, 8, 6),), gemm=(257, 163, 292, 7)),
)
TV_BATCH = 16                    # the "tv_batch" of the short-batch E-step; with "tv_acc_mb" 0 every batch is a super-batch of its own
EIG_COND = 1e3                   # the condition number (estimation_ref.CONDS) of the eigen / LDA / two-covariance inputs

# name, (C, D, T, spread), segments, models, trials, ctop of determine_top / of llr_trials, utterance layouts of tv_stats, online
# files, energy files (frames), cohort length, list lengths, matrix (M, S), options of the whole case, planted frames
# runs: the label segments of windowed NormFeat and TurnDetection (run_table): P = gmmiv_turn_tile_positions at the case's columns for
# (TURN_W, TURN_S); heads = per file of file_table the lengths of its first runs, a guard frame after each; cycle = the lengths that
# fill the rest of a file that has heads, no frame between them.  Judged: runs of 0 positions (L = 5 and L = 2 W = 8), 1 (9, 10, 11),
# 2 (12, 14) and more, P + 1 = 15 positions (L = 51) where the file holds them -- at T = 65 and 66 no file does -- and a file without runs.
TURN_W, TURN_S, TURN_COLS = 4, 3, 60       # the windows of the "turn detection" step; the columns it reads of a wider matrix
RUN_CYCLE = (1, 2, 1, 1, 3, 1, 2)          # dirtying: runs without positions, seven of them in eleven frames
SMALL = (
    dict(name="s37x13x65", gcase=(37, 13, 65, 2.0), nseg=5, G=3, ntrial=6, ctops=(10, 17), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0, iv=IV_SMALL[0],
         runs=dict(P=32, heads=((5, 8, 9, 11), (), (12, 12)), cycle=())),
    dict(name="s129x60x257", gcase=(129, 60, 257, 2.0), nseg=5, G=3, ntrial=6, ctops=(10, 17, 70), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0, iv=IV_SMALL[1],
         runs=dict(P=14, heads=((5, 8, 51, 9), (), (12, 40, 20)), cycle=())),
    dict(name="s40x97x66", gcase=(40, 97, 66, 0.5), nseg=5, G=3, ntrial=6, ctops=(10, 17), trial_ctops=(10, 17), tv="abc", nfiles=3,
         energy=(65, 0, 257), cohort=33, lists=(5, 65, 17), ms=(5, 7), opts={}, plant=False, online_rows=0, iv=IV_SMALL[2],
         runs=dict(P=14, heads=((5, 8, 9, 12), (), (10, 14)), cycle=())),
)
LARGE = (
    dict(name="L530x60x4300", gcase=(530, 60, 4300, 2.0), nseg=40, G=7, ntrial=60, ctops=(10, 17, 70, 100), trial_ctops=(17, 64), tv="bc",
         nfiles=3, energy=(5000, 2500, 0, 6001, 700, 9000, 1300), cohort=100003, lists=(100003, 7, 2049, 64), ms=(7, 11),
         opts={"z_scratch_mb": Z_MB_530, "timing": 1}, plant=True, online_rows=48000, iv=IV_LARGE[0],
         runs=dict(P=14, heads=((51, 300, 9, 12), (), (8, 5, 200, 14)), cycle=RUN_CYCLE)),
    dict(name="L96x101x700", gcase=(96, 101, 700, 0.5), nseg=40, G=7, ntrial=60, ctops=(10, 17, 64), trial_ctops=(17, 64), tv="abc", nfiles=3,
         energy=(5000, 2500, 0, 6001, 700, 9000, 1300), cohort=100003, lists=(100003, 7, 2049, 64), ms=(7, 11), opts={}, plant=True, online_rows=48000,
         iv=IV_LARGE[1],
         runs=dict(P=14, heads=((51, 150, 9, 12), (), (8, 5, 40)), cycle=RUN_CYCLE)),
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
def _run_table(name):
    case = CASES[name]
    fb, spec, rows = file_table(case), case["runs"], []
    assert len(spec["heads"]) == case["nfiles"]
    for f, heads in enumerate(spec["heads"]):
        pos, end = int(fb[f]), int(fb[f + 1])
        for n in heads:
            assert pos + n <= end, (name, f, n)
            rows.append((pos, n, f))
            pos += n + 1
        k = 0
        while heads and spec["cycle"] and pos + spec["cycle"][k % len(spec["cycle"])] <= end:
            n = spec["cycle"][k % len(spec["cycle"])]
            rows.append((pos, n, f))
            pos, k = pos + n, k + 1
    return _frozen((np.array(rows, np.int64).reshape(-1, 3), fb[:-1].copy()))


def run_table(case):
    """-> (runs [nrun, 3] = (first frame, length, file), file_first [nfiles]) of the "normfeat window" and "turn detection" steps.
    The existing tables do not serve as they are: seg_table / _norm_runs cut [3, T - 1) into ADJACENT segments of G groups (G = 7 > nfiles
    on the dirtying cases) and drop the empty one, so no run is shorter than 2 W, none lies behind a guard frame and there cannot be 2049 of
    them; file_table is sound as the files' extents -- [file_begin[f], file_begin[f + 1]), the middle file empty -- and the runs are laid
    inside them: begins strictly increasing, no overlap (gmmiv_plan_norm_windows), file ids non-decreasing, a file without runs"""
    return _run_table(case["name"])


def turn_cols(case):
    return min(case["gcase"][1], TURN_COLS)


@functools.lru_cache(maxsize=None)
def _turn_table(name):
    case = CASES[name]
    runs, _ = _run_table(name)
    nf = case["nfiles"]
    n = [tn.positions_as_written(int(L), TURN_W, TURN_S) for L in runs[:, 1]]
    po = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    npos = int(po[-1])
    rng = np.random.default_rng(len(runs) + npos)
    curve = rng.integers(-50, 50, npos).astype(np.float64)                 # exact under the smoothing; no -0.5 (stream_order.poison)
    curve[npos // 2] = np.nan
    dec = (rng.random(npos) < 0.3).astype(np.uint8)
    cnt = np.zeros(nf, np.int64)
    for r, (b, L, f) in enumerate(runs):
        cnt[f] += len(tn.segments_as_written(int(b), int(L), TURN_W, TURN_S, dec[int(po[r]):int(po[r + 1])]))
    room = cnt.copy()
    room[0] -= 2                                                           # two entries short for the first file, three long for the last
    room[nf - 1] += 3
    assert room.min() >= 0 and cnt[0] > 2
    return _frozen(dict(runs=runs, pos_off=po, curve=curve, dec=dec, seg_count=cnt, seg_off=np.concatenate([[0], np.cumsum(room)]).astype(np.int64)))


def turn_table(case):
    """-> dict(runs, pos_off: the CSR of turn_ref.positions_as_written for (TURN_W, TURN_S); curve: an integer curve with one NaN over
    pos_off, for turn_pick alone; dec: a decision table of its own, for turn_segments alone; seg_count: the segments per file that dec
    makes (turn_ref.segments_as_written); seg_off: the CSR of a room two entries short for file 0 and three long for the last file)"""
    return _turn_table(case["name"])


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
    out = dict(C=C, D_tiles=(D + 3) // 4, T=T, nseg=case["nseg"], G=case["G"], ntrial=case["ntrial"], ctop=max(case["ctops"]),
               trial_ctop=max(case["trial_ctops"]), nfiles=case["nfiles"], energy_files=len(case["energy"]), energy_frames=max(case["energy"]),
               cohort=case["cohort"], list_len=max(case["lists"]), nlists=len(case["lists"]), M=case["ms"][0], S=case["ms"][1])
    out.update(run_sizes(case))
    out.update(iv_sizes(case))
    return out


NORMWIN = (0.5, 0.8, 0.01)       # window duration (s), windowComp, frame length (s) of the "normfeat window" step


@functools.lru_cache(maxsize=None)
def _window_plan(name):
    runs, first = _run_table(name)
    return _frozen(nw.plan(runs, CASES[name]["nfiles"], first, *NORMWIN))


def run_sizes(case):
    """what sizes a slot of gmmiv_feat_norm_window and the gmmiv_turn_* calls: the run partials are 2 D doubles per run (WS_PART), the
    staged tables and outputs go by runs, positions, steps and files, the segment room by the CSR the caller brings -- seg_room is the
    larger of the room of turn_table's own dec and of nrun + npos, which no chain of the judged cases can exceed (a run yields at most
    one segment per position and one more)"""
    t = turn_table(case)
    nrun, npos = len(t["runs"]), int(t["pos_off"][-1])
    return dict(nrun=nrun, npos=npos, nsteps=len(_window_plan(case["name"])[2]), nrun_D=nrun * case["gcase"][1], seg_room=max(int(t["seg_off"][-1]), nrun + npos))


def iv_sizes(case):
    """the quantities that size a workspace of the i-vector back end: the largest of each over the sets of the case"""
    iv = case["iv"]
    tv = iv["tv"]
    _, sps = dev_data(case)
    ems = [em_state(case, k) for k in range(len(iv["em"]))]
    jfa = jfa_data(case)
    out = dict(tv_C=max(t[0] for t in tv), tv_D=max(t[1] for t in tv), tv_CD=max(t[0] * t[1] for t in tv), tv_R=max(t[2] for t in tv),
               tv_P=max(t[2] * (t[2] + 1) // 2 for t in tv), tv_U=max(t[3] for t in tv), tv_batches=max(-(-t[3] // TV_BATCH) for t in tv),
               tv_UCD=max(t[3] * t[0] * t[1] for t in tv), tv_RCD=max(t[2] * t[0] * t[1] for t in tv), tv_CP=max(t[0] * t[2] * (t[2] + 1) // 2 for t in tv),
               dev_dim=iv["dev"][0] if not isinstance(iv["dev"], str) else br.DEV_CASES[iv["dev"]][0], dev_speakers=len(sps), dev_sessions=int(sps.sum()),
               dev_longest=int(sps.max()), plda_dim=iv["plda"][0], plda_rf=iv["plda"][1], plda_rg=iv["plda"][2], score_dim=iv["score"][0],
               score_M=iv["score"][1], score_S=iv["score"][2], score_trials=len(trial_lists(case)[0]), ivn_in=iv["ivn"][0], ivn_out=iv["ivn"][1],
               ivn_n=iv["ivn"][2], jfa_C=jfa["C"], jfa_D=jfa["D"], jfa_CD=jfa["C"] * jfa["D"], jfa_R=jfa["R"], jfa_speakers=jfa["nspk"],
               jfa_sessions=jfa["nsess"], eig=iv["eig"], ortho_R=max(k[0] for k in iv["ortho"]), ortho_SV=max(k[1] for k in iv["ortho"]),
               em_dim=max(s[0].shape[0] for s in ems), em_sessions=max(s[0].shape[1] for s in ems), em_speakers=max(len(s[1]) for s in ems),
               em_longest=max(int(s[1].max()) for s in ems), em_rf=max(s[2].shape[1] for s in ems), em_rg=max(s[3].shape[1] for s in ems),
               gemm_M=iv["gemm"][0], gemm_N=iv["gemm"][1], gemm_K=iv["gemm"][2], gemm_slabs=iv["gemm"][0] * iv["gemm"][1] * iv["gemm"][3])
    return out


# ---------------------------------------------------------------------------------------------------------------- i-vector inputs
def _frozen(d):
    for v in (d.values() if isinstance(d, dict) else d):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def tv_inputs(C, D, R, U):
    """one T-matrix chain in double: tv_ref.statistics, and on them, in plain numpy, what each link is handed -- the centred statistics
    F0, the packed TETt, the normalised statistics and T of the approximate extractors with their Wm / Dm / Q, SPD accumulators for the
    M-step and the sums of a minimum-divergence call (the recipe of tv_ref.md_problem on this chain's T)"""
    s = tr.statistics(C, D, R, U)
    N, F, means, iv, Tm = s["N"], s["F"], s["means"], s["invvar"], s["Tm"]
    rng = np.random.default_rng(7919 * C + 101 * R + U)
    il = np.tril_indices(R)
    F0 = np.ascontiguousarray(F - np.repeat(N, D, axis=1) * means[None, :])
    Tc, ivc = Tm.reshape(R, C, D), iv.reshape(C, D)
    te = np.stack([((Tc[:, c, :] * ivc[c]) @ Tc[:, c, :].T)[il] for c in range(C)])
    siv = np.sqrt(iv)[None, :]
    Fn, Tn = np.ascontiguousarray(F0 * siv), np.ascontiguousarray(Tm * siv)
    weight = rng.dirichlet(np.ones(C))
    Q = np.ascontiguousarray(np.linalg.qr(rng.normal(size=(R, R)))[0])
    Wm = (Tn * np.repeat(weight, D)[None, :]) @ Tn.T
    A3 = (Tn.T @ Q).reshape(C, D, R)
    G = rng.normal(size=(C, R, R + 3))
    A = np.einsum("cik,cjk->cij", G, G) / (R + 3) + 0.5 * np.eye(R)[None]
    n = 50
    Wn = rng.normal(size=(n, R)) * np.exp(rng.normal(0.0, 1.0, R))[None, :] + 0.3
    Rm = Wn.T @ Wn + 0.1 * n * np.eye(R)
    return _frozen(dict(N=N, F=F, means=means, invvar=iv, Tm=Tm, F0=F0, te=np.ascontiguousarray(te), Wv=rng.normal(size=(U, R)), Fn=Fn, Tn=Tn,
                        weight=weight, Q=Q, Wm=np.ascontiguousarray((Wm + Wm.T) / 2), Dm=np.ascontiguousarray(np.sum(A3 * A3, 1)),
                        Ap=np.ascontiguousarray(A[:, il[0], il[1]]), Cmx=rng.normal(size=(R, C * D)), md_Rm=np.ascontiguousarray((Rm + Rm.T) / 2),
                        md_r=Wn.sum(0), md_meanW=Wn.sum(0) / n, md_n=n))


def chains(case):
    return [("%dx%dx%dx%d " % k, k, tv_inputs(*k)) for k in case["iv"]["tv"]]


@functools.lru_cache(maxsize=None)
def _dev_large(dim, nspk, longest):
    """the recipe of backend_ref.dev_inputs on ragged counts of 1 .. 4 sessions and one speaker of `longest`"""
    rng = np.random.default_rng(100 * dim + nspk)
    sps = rng.integers(1, 5, nspk).astype(np.int64)
    sps[nspk // 3] = longest
    cls = np.repeat(np.arange(nspk), sps)
    X = np.ascontiguousarray((rng.normal(size=(dim, nspk)) * 1.5)[:, cls] + rng.normal(size=(dim, int(sps.sum()))))
    return _frozen((X, sps))


def dev_data(case):
    """-> (X [dim, n], sessions per speaker)"""
    d = case["iv"]["dev"]
    return es.dev_set(d) if isinstance(d, str) else _dev_large(*d)


@functools.lru_cache(maxsize=None)
def _em_large(dim, rf, rg, dev):
    """the recipe of estimation_ref.em_inputs on the session counts of a large development set"""
    sps = _dev_large(*dev)[1]
    rng = np.random.default_rng(1000 * dim + 10 * rf + rg)
    k, n = len(sps), int(sps.sum())
    cls = np.repeat(np.arange(k), sps)
    Ft, Gt = rng.normal(size=(dim, rf)), 0.5 * rng.normal(size=(dim, rg))
    X = Ft @ rng.normal(size=(rf, k))[:, cls] + Gt @ rng.normal(size=(rg, n)) + 0.3 * rng.normal(size=(dim, n)) + 0.2
    F, G = rng.normal(size=(dim, rf)), 0.5 * rng.normal(size=(dim, rg))
    return _frozen(tuple(np.ascontiguousarray(a) for a in (X, sps, F, G, np.cov(X) + 0.1 * np.eye(dim), 0.1 * rng.normal(size=dim) + 0.05)))


def em_state(case, k):
    """-> (X, sps, F, G, Sigma, Delta) of the k-th EM set of the case"""
    e = case["iv"]["em"][k]
    return es.em_inputs(e) if isinstance(e, str) else _em_large(*e, case["iv"]["dev"])


@functools.lru_cache(maxsize=None)
def _jfa_large(C, D, R, sessions):
    """the recipe of backend_ref.jfa_inputs on another table of sessions per speaker"""
    rng = np.random.default_rng(10007 * C + 101 * D + R)
    SV = C * D
    nses = np.asarray(sessions, np.int64)
    nspk, nsess = len(nses), int(nses.sum())
    sb = np.concatenate([[0], np.cumsum(nses)]).astype(np.int64)

    def mag(shape):
        return rng.uniform(1.0, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    g = np.ones(C)
    g[br.jfa_faint(C)], g[0] = br.JFA_FAINT, br.JFA_LOUD
    Nh = rng.uniform(0.2, 8.0, (nsess, C)) * g[None, :]
    Fh = (Nh[:, :, None] * rng.uniform(-1.0, 1.0, (nsess, C, D))).reshape(nsess, SV)
    N = np.stack([Nh[sb[i]:sb[i + 1]].sum(0) for i in range(nspk)])
    F = np.stack([Fh[sb[i]:sb[i + 1]].sum(0) for i in range(nspk)])
    return _frozen(dict(C=C, D=D, R=R, nspk=nspk, nsess=nsess, sb=sb, owner=np.repeat(np.arange(nspk), nses).astype(np.int64), Nh=np.ascontiguousarray(Nh),
                        Fh=np.ascontiguousarray(Fh), N=np.ascontiguousarray(N), F=np.ascontiguousarray(F), m=mag(SV), V=mag((R, SV)), Um=mag((R, SV)),
                        Y=mag((nspk, R)), X=mag((nsess, R)), Dm=rng.uniform(1.0, 2.0, SV), Z=mag((nspk, SV)), iv=rng.uniform(0.5, 2.0, SV)))


def jfa_data(case):
    j = case["iv"]["jfa"]
    return br.jfa_inputs(*j) if len(j) == 3 else _jfa_large(*j)


def score_data(case):
    return br.score_case(*case["iv"]["score"], "plain")


def ftjf_pair(case):
    """-> (A, B): the FTJF of the case and a second one of the same rf that differs from it in ONE element (A stays positive definite)"""
    A = score_data(case)["FTJF"]
    B = A.copy()
    B[A.shape[0] // 2, A.shape[0] // 2] += 0.25
    return A, B


def trial_lists(case):
    dim, M, S = case["iv"]["score"]
    return ivr.trial_list("sparse", M, S)


@functools.lru_cache(maxsize=None)
def gemm_operands(M, N, K, nz):
    rng = np.random.default_rng([M, N, K])
    return _frozen((rng.normal(size=(M, K)), rng.normal(size=(N, K)), rng.normal(size=(M, N))))


# ---------------------------------------------------------------------------------------------------------------- plumbing
def _torch():
    import torch
    return torch


_KEEP = []                       # every device tensor of the running step: see dev()
RECORDER = None                  # tests/stream_order.py: while set, every device tensor of a step is registered with it under its role


def dev(a, role="in"):
    """a device copy that lives until the step has synchronised its context (Step.run).  The contexts here own a private stream and a
    call on device tensors only enqueues: a tensor dropped right after the call goes back to torch's caching allocator, and the next
    tensor -- filled on torch's stream -- may land in it while the kernel that reads it is still queued"""
    t = _torch()
    out = t.from_numpy(np.array(a)).cuda()
    _KEEP.append(out)
    if RECORDER is not None:
        RECORDER.register(out, role)
    return out


def to(form, a):
    return a if form == "host" or a is None else dev(a)


def buf(form, shape, dtype=np.float64, fill=None):
    """an output buffer of the form, pre-filled with the sentinel of its dtype"""
    if fill is None:
        fill = SENT32 if np.dtype(dtype) == np.float32 else (SENTINEL if np.dtype(dtype) == np.float64 else -77)
    a = np.full(shape, fill, dtype)
    return a if form == "host" else dev(a, "out")


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
    entry is the default path, the second the "stats_z 0" step (no k_stats_z there: its count is the earlier call's) -- and the
    launches of k_dgemm(L) after either call of an E-step (ws_history.estep)"""

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


def s_normwin(ctx, h, case, form):
    """the plan of NORMWIN on run_table, then two calls, each on a copy of the frames: flags 0 with both statistics, cmsOnly with
    neither.  The rewritten buffers come back whole: the guard frames between the runs and the unowned rows keep their values"""
    from lia_ral_amd import capi
    D, nf = case["gcase"][1], case["nfiles"]
    runs, first = run_table(case)
    off, st, al = capi.plan_norm_windows(runs, nf, first, *NORMWIN)
    r, o, s, a = to(form, runs), to(form, off), to(form, st), to(form, al)
    x = frames(case, form)
    both = mut("device", x)
    gstat, sstat = buf(form, (nf, 2 * D)), buf(form, (len(al), 2 * D))
    ctx.feat_norm_window(both, r, nf, o, s, a, gstat=gstat, step_stat=sstat)
    cms = mut("device", x)
    ctx.feat_norm_window(cms, r, nf, o, s, a, cms_only=True, stats=False)
    return {"frames": both, "gstat": gstat, "step_stat": sstat, "frames cmsOnly": cms}


def s_turn(ctx, h, case, form):
    """(a) the chain of a caller: curve -> pick -> segments, counted, then filled into the room the counts give and three entries more;
    (b) turn_pick alone on turn_table's integer curve with smoothed = NULL: the smoothed curve lives in WS_PART; (c) turn_segments alone
    on turn_table's dec, in a room two entries short for file 0 and three long for the last file.  For D > TURN_COLS the frames are the
    first TURN_COLS columns of the matrix, with its stride"""
    nf, W, S = case["nfiles"], TURN_W, TURN_S
    t = turn_table(case)
    nrun, npos = len(t["runs"]), int(t["pos_off"][-1])
    x = dev(frames(case, form))[:, :turn_cols(case)]
    r, p = to(form, t["runs"]), to(form, t["pos_off"])
    ints = lambda n: buf(form, (n,), np.int64)
    # (a)
    value, status = buf(form, (npos,)), buf(form, (npos,), np.int32)
    ctx.turn_curve(x, r, nf, p, W, S, "DGLR", value=value, status=status, npos=npos)
    sm, dec, rs, nt = buf(form, (npos,)), buf(form, (npos,), np.uint8, fill=9), buf(form, (nrun, 2)), ints(nrun)
    ctx.turn_pick(value, p, 0.5, sm, dec, rs, nt, npos=npos)
    cnt = ints(nf)
    ctx.turn_segments(r, nf, p, dec, W, S, seg_count=cnt, npos=npos)
    off = np.concatenate([[0], np.cumsum(host(cnt))]).astype(np.int64)
    assert 0 < off[-1] <= nrun + npos
    cnt_fill, sb, sl = ints(nf), ints(int(off[-1]) + 3), ints(int(off[-1]) + 3)
    ctx.turn_segments(r, nf, p, dec, W, S, seg_off=to(form, off), seg_begin=sb, seg_len=sl, seg_count=cnt_fill, npos=npos)
    out = {"value": value, "status": status, "smoothed": sm, "dec": dec, "run_stats": rs, "n_turns": nt, "seg_count": cnt, "seg_count of the fill": cnt_fill,
           "seg_begin": sb, "seg_len": sl}
    # (b)
    dec_b, rs_b, nt_b = buf(form, (npos,), np.uint8, fill=9), buf(form, (nrun, 2)), ints(nrun)
    ctx.turn_pick(to(form, t["curve"]), p, 0.5, dec=dec_b, run_stats=rs_b, n_turns=nt_b, npos=npos, smooth=False)
    out.update({"pick alone dec": dec_b, "pick alone run_stats": rs_b, "pick alone n_turns": nt_b})
    # (c)
    room = int(t["seg_off"][-1])
    cnt_c, sb_c, sl_c = ints(nf), ints(room + 3), ints(room + 3)
    ctx.turn_segments(r, nf, p, to(form, t["dec"]), W, S, seg_off=to(form, t["seg_off"]), seg_begin=sb_c, seg_len=sl_c, seg_count=cnt_c, npos=npos)
    out.update({"segments alone seg_count": cnt_c, "segments alone seg_begin": sb_c, "segments alone seg_len": sl_c})
    return out


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


# ---------------------------------------------------------------------------------------------------------------- i-vector back end
def mut(form, a):
    """a writable copy in the form: what a call that works in place is handed (the cached inputs are read-only)"""
    return np.array(a) if form == "host" else dev(a, "inout")


def s_tv_centre(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        N, m = to(form, p["N"]), to(form, p["means"])
        out[tag + "subtract_m"] = ctx.tv_subtract_m(N, mut(form, p["F"]), m, C, D)
        out[tag + "subtract_m_to"] = ctx.tv_subtract_m_to(N, to(form, p["F"]), buf(form, p["F"].shape), m, C, D)
        inplace = mut(form, p["F"])
        out[tag + "subtract_m_to in place"] = ctx.tv_subtract_m_to(N, inplace, inplace, m, C, D)
        out[tag + "norm_statistics"] = ctx.tv_norm_statistics(N, mut(form, p["F"]), m, to(form, p["invvar"]), C, D)
        out[tag + "subtract_m_plus_tw"] = ctx.tv_subtract_m_plus_tw(N, mut(form, p["F"]), m, to(form, p["Tm"]), to(form, p["Wv"]), C, D)
    return out


def s_tv_tett(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        out[tag + "tett"] = ctx.tv_tett(to(form, p["Tm"]), to(form, p["invvar"]), C, D, out=buf(form, p["te"].shape))
    return out


def s_tv_estimate_w(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        out[tag + "W"] = ctx.tv_estimate_w(*(to(form, p[k]) for k in ("N", "F0", "Tm", "invvar", "te")), C, D, out=buf(form, (U, R)))
    return out


def estep(ctx, h, case, form, log):
    """tv_estimate_a_and_c on the two halves of the utterances into ONE set of accumulators: host arrays (the library works on
    hipMalloc'd copies of them) or device tensors.  Where the case times its kernels, the launches of k_dgemm(L) -- one per batch -- of
    either call go to the log"""
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        N, F0, Tm, iv, te = (to(form, p[k]) for k in ("N", "F0", "Tm", "invvar", "te"))
        acc = {k: buf(form, s, fill=0.0) for k, s in (("A", p["Ap"].shape), ("Cmx", (R, C * D)), ("Rm", (R, R)), ("r", (R,)), ("meanW", (R,)))}
        half = U // 2
        for k, (lo, hi) in enumerate(((0, half), (half, U))):
            acc["W"] = buf(form, (hi - lo, R))
            ctx.tv_estimate_a_and_c(N[lo:hi], F0[lo:hi], Tm, iv, te, C, D, acc=acc)
            out[tag + "W of call %d" % (k + 1)] = acc["W"]
            if k == 0:
                out[tag + "A after call 1"] = host(acc["A"])
            if case["opts"].get("timing"):
                h.log.setdefault((case["name"], log, form), []).append(ctx.kernel_launches("k_dgemm(L)"))
        out.update({tag + k: acc[k] for k in ("A", "Cmx", "Rm", "r", "meanW")})
    return out


def estep_batches(case, tv_batch):
    """the batches -- one launch of k_dgemm(L) each -- of either call of the E-step on the last chain of the case"""
    U = case["iv"]["tv"][-1][3]
    return [-(-n // min(n, tv_batch)) for n in (U // 2, U - U // 2)]


def s_tv_estep(ctx, h, case, form):
    return estep(ctx, h, case, form, "e-step")


def s_tv_estep_batches(ctx, h, case, form):
    return estep(ctx, h, case, form, "e-step in batches")


def s_tv_estep_chol_gemm(ctx, h, case, form):
    return estep(ctx, h, case, form, "e-step chol_gemm")


def s_tv_update_t(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        out[tag + "T"] = ctx.tv_update_t(to(form, p["Ap"]), to(form, p["Cmx"]), C, D, out=buf(form, (R, C * D)))
    return out


def s_tv_min_divergence(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        Rm, r, mean, Tm = (mut(form, p[k]) for k in ("md_Rm", "md_r", "means", "Tm"))
        ctx.tv_min_divergence(Rm, r, to(form, p["md_meanW"]), mean, Tm, p["md_n"], C, D)
        out.update({tag + "Rn": Rm, tag + "r / n": r, tag + "mean": mean, tag + "Ch T": Tm})
    return out


def s_tv_mstep(ctx, h, case, form):
    out = s_tv_update_t(ctx, h, case, form)
    out.update(s_tv_min_divergence(ctx, h, case, form))
    for key in case["iv"]["ortho"]:
        out["orthonormalize_t %dx%d %s" % key] = ctx.tv_orthonormalize_t(mut(form, es.ortho_inputs(key)))
    return out


def s_tv_approximate(ctx, h, case, form):
    out = {}
    for tag, (C, D, R, U), p in chains(case):
        N, Fn, Tn, Q = (to(form, p[k]) for k in ("N", "Fn", "Tn", "Q"))
        out[tag + "norm_t"] = ctx.tv_norm_t(mut(form, p["Tm"]), to(form, p["invvar"]), C, D)
        out[tag + "weighted_cov"] = ctx.tv_weighted_cov(Tn, to(form, p["weight"]), C, D, out=buf(form, (R, R)))
        out[tag + "approximate_tctc"] = ctx.tv_approximate_tctc(Tn, Q, C, D, out=buf(form, (C, R), fill=0.0))
        out[tag + "approximate_tctc onto a start"] = ctx.tv_approximate_tctc(Tn, Q, C, D, out=mut(form, p["Dm"]))
        out[tag + "W ubm_weight"] = ctx.tv_estimate_w_ubm_weight(N, Fn, Tn, to(form, p["Wm"]), C, D, out=buf(form, (U, R), fill=0.0))
        out[tag + "W ubm_weight onto a start"] = ctx.tv_estimate_w_ubm_weight(N, Fn, Tn, to(form, p["Wm"]), C, D, out=mut(form, p["Wv"]))
        out[tag + "W eigen"] = ctx.tv_estimate_w_eigen(N, Fn, Tn, to(form, p["Dm"]), Q, C, D, out=buf(form, (U, R), fill=0.0))
    return out


def s_dgemm_splitk(ctx, h, case, form):
    """gmmiv_dgemm takes device operands only.  The two forms are two calls of the split-K product on them: "host" writes alpha A B^T over
    a sentinel-filled C (beta = 0 must not read it), "device" accumulates -2 C onto it"""
    M, N, K, nz = case["iv"]["gemm"]
    A, B, C0 = gemm_operands(M, N, K, nz)
    Cm = buf("device", (M, N)) if form == "host" else dev(C0)
    ctx.dgemm(0, 1, 1.0 if form == "host" else -0.5, dev(A), dev(B), 0.0 if form == "host" else -2.0, Cm, nz=nz)
    return {"C": Cm}


def s_iv_normalize(ctx, h, case, form):
    din, dout, n = case["iv"]["ivn"]
    p = br.ivn_inputs(din, dout, n)
    out = {}
    for mean, M, ln in br.IVN_FORMS:
        mu, Mx = (to(form, p["mean"]) if mean else None), (to(form, p["M"]) if M else None)
        tag = "mean %d M %d length_norm %d" % (bool(mean), bool(M), ln)
        out[tag] = ctx.iv_normalize(to(form, p["X"]), mu, Mx, ln, out=buf(form, (dout if M else din, n)))
        if not M:
            X = mut(form, p["X"])
            out[tag + " in place"] = ctx.iv_normalize(X, mu, None, ln, out=X)
    return out


def s_dev_set(ctx, h, case, form):
    """the results of dev_means / _cov_mat / _scatter_mat are host arrays in either form (the binding allocates them); the two calls
    governed by an inverse run on the sets that have one (more than 2 dim sessions)"""
    X, sps = dev_data(case)
    dim, n = X.shape
    Xa = to(form, X)
    out = dict(zip(("mean", "speaker means"), ctx.dev_means(Xa, sps)))
    out.update(zip(("Sigma", "W", "B"), ctx.dev_cov_mat(Xa, sps)))
    out.update(zip(("SB", "SW"), ctx.dev_scatter_mat(Xa, sps)))
    if n > 2 * dim:
        out["wccn_chol"] = ctx.dev_wccn_chol(Xa, sps, out=buf(form, (dim, dim)))
        out["mahalanobis"] = ctx.dev_mahalanobis(Xa, sps, out=buf(form, (dim, dim)))
    return out


def s_eigen(ctx, h, case, form):
    n = case["iv"]["eig"]
    A = to(form, es.eigen_matrix(("spd", n, EIG_COND)))
    W, B = (to(form, a) for a in es.lda_inputs(("spd", n, EIG_COND)))
    out = {}
    for rank in sorted({n, max(n // 2, 1)}, reverse=True):
        out["sym_eigen rank %d vect" % rank], out["sym_eigen rank %d val" % rank] = ctx.sym_eigen(A, rank, out=(buf(form, (n, rank)), buf(form, (rank,))))
        out["lda rank %d mat" % rank], out["lda rank %d val" % rank] = ctx.dev_lda(W, B, rank, out=(buf(form, (rank, n)), buf(form, (rank,))))
    out["efr_matrix"] = ctx.dev_efr_matrix(A, out=buf(form, (n, n)))
    return out


def s_plda(ctx, h, case, form):
    out = {}
    for k in range(len(case["iv"]["em"])):
        state = em_state(case, k)
        sps = state[1]
        X, F, G, Sigma, Delta = (mut(form, state[i]) for i in (0, 2, 3, 4, 5))
        for it in (1, 2):
            ctx.plda_em_iteration(X, sps, F, G, Sigma, Delta)
            out.update({"em set %d iteration %d %s" % (k, it, name): host(a) for name, a in zip(("X", "F", "G", "Sigma", "Delta"), (X, F, G, Sigma, Delta))})
    dim, rf, rg = case["iv"]["plda"]
    F, G, S = (to(form, a) for a in es.precompute_inputs((dim, rf, rg)))
    out["FTJ"], out["FTJF"] = ctx.plda_precompute(F, G, S, out=(buf(form, (rf, dim)), buf(form, (rf, rf))))
    n = case["iv"]["eig"]
    W, B = (to(form, a) for a in es.twocov_inputs((n, EIG_COND)))
    out["twocov G"], out["twocov H"] = ctx.twocov_model(W, B, out=(buf(form, (n, n)), buf(form, (n, n))))
    return out


def s_score_rules(ctx, h, case, form):
    """the five rules and the trial mask; PLDA with FTJF A, with B (one element of A moved, the same session counts: a K_n kept from A
    would be used again), then with A again"""
    p = score_data(case)
    M, S = p["M"], p["S"]
    m, s, ms = to(form, p["m"]), to(form, p["s"]), to(form, p["msum"])
    A, B = ftjf_pair(case)
    out = {"cosine": ctx.score_cosine(m, s, out=buf(form, (M, S))),
           "mahalanobis": ctx.score_mahalanobis(m, s, to(form, p["Mah"]), out=buf(form, (M, S))),
           "twocov": ctx.score_twocov(m, s, to(form, p["G"]), to(form, p["H"]), out=buf(form, (M, S))),
           "twocov_mix_part": ctx.score_twocov_mix_part(m, s, to(form, p["G"]), mut(form, p["C_in"]))}
    for tag, Fm in (("A", A), ("B", B), ("A again", A)):
        out["plda FTJF " + tag] = ctx.score_plda(ms, p["nsess"], s, to(form, Fm), out=buf(form, (M, S)))
    mask = (np.random.default_rng(M + S).random((M, S)) < 0.3).astype(np.uint8)
    out["apply_trials"] = ctx.score_apply_trials(to(form, mask), mut(form, p["C_in"]), -7.5)
    return out


def s_score_trials(ctx, h, case, form):
    """the four list rules on a sparse shuffled list; PLDA with the FTJF the matrix rule used last (the context's K_n cache is shared)"""
    p = score_data(case)
    m, s, ms = to(form, p["m"]), to(form, p["s"]), to(form, p["msum"])
    tm, ts = trial_lists(case)
    A, _ = ftjf_pair(case)
    return {"cosine": ctx.score_cosine_trials(m, s, tm, ts, out=buf(form, (len(tm),))),
            "mahalanobis": ctx.score_mahalanobis_trials(m, s, to(form, p["Mah"]), tm, ts, out=buf(form, (len(tm),))),
            "twocov": ctx.score_twocov_trials(m, s, to(form, p["G"]), to(form, p["H"]), tm, ts, out=buf(form, (len(tm),))),
            "plda": ctx.score_plda_trials(ms, p["nsess"], s, to(form, A), tm, ts, out=buf(form, (len(tm),)))}


def s_jfa(ctx, h, case, form):
    p = jfa_data(case)
    C, D = p["C"], p["D"]
    out = {}
    for f in br.JFA_SUBTRACT_FORMS:
        N, F, kw = br.jfa_subtract_args(p, f)
        out["subtract " + f] = ctx.jfa_subtract(to(form, N), mut(form, F), C, D, **{k: to(form, v) for k, v in kw.items()})
    out["subtract_sessions"] = ctx.jfa_subtract_sessions(p["sb"], to(form, p["Nh"]), mut(form, p["F"]), to(form, p["Um"]), to(form, p["X"]), C, D)
    N, F, iv = to(form, p["N"]), to(form, p["F"]), to(form, p["iv"])
    for tau in (-1.0, 14.0):
        out["estimate_z tau %g" % tau] = ctx.jfa_estimate_z(N, F, iv, to(form, p["Dm"]), C, D, tau=tau, out=buf(form, p["F"].shape))
    Dm = mut(form, p["Dm"])
    out["estimate_z_and_d Z"] = ctx.jfa_estimate_z_and_d(N, F, iv, Dm, C, D, out=buf(form, p["F"].shape))
    out["estimate_z_and_d D"] = Dm
    return out


# ---------------------------------------------------------------------------------------------------------------- the programme
_use =("gmmiv_llk_determine_top", "gmmiv_llk_use_top", "gmmiv_llk_use_top_multi")
_em = ("gmmiv_em_accumulate", "gmmiv_em_get", "gmmiv_variance_control")
_mllr_ok = lambda case: case["gcase"][1] <= MLLR_MAX_DIM
_approx = ("gmmiv_tv_norm_t", "gmmiv_tv_weighted_cov", "gmmiv_tv_approximate_tctc", "gmmiv_tv_estimate_w_ubm_weight", "gmmiv_tv_estimate_w_eigen")
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
    Step("normfeat window", s_normwin, ("gmmiv_plan_norm_windows", "gmmiv_feat_norm_window")),
    Step("turn detection", s_turn, ("gmmiv_turn_curve", "gmmiv_turn_pick", "gmmiv_turn_segments")),
    Step("gather + scatter runs", s_runs, ("gmmiv_gather_runs", "gmmiv_scatter_runs", "gmmiv_gather_frames")),
    Step("energy_detect", s_energy, ("gmmiv_energy_train", "gmmiv_energy_select")),
    Step("score matrix", s_score_matrix, ("gmmiv_score_cohort_stats", "gmmiv_score_normalize")),
    Step("score lists", s_score_lists, ("gmmiv_score_list_stats", "gmmiv_score_normalize_list")),
    # the i-vector back end: in every sequence -- the reversed one too -- these interleave with the GMM side on one context
    Step("tv centre", s_tv_centre, ("gmmiv_tv_subtract_m", "gmmiv_tv_subtract_m_to", "gmmiv_tv_norm_statistics", "gmmiv_tv_subtract_m_plus_tw")),
    Step("tv tett", s_tv_tett, ("gmmiv_tv_tett",)),
    Step("tv estimate_w", s_tv_estimate_w, ("gmmiv_tv_estimate_w",)),
    Step("tv e-step", s_tv_estep, ("gmmiv_tv_estimate_a_and_c",)),
    Step("tv m-step", s_tv_mstep, ("gmmiv_tv_update_t", "gmmiv_tv_min_divergence", "gmmiv_tv_orthonormalize_t")),
    Step("tv approximate", s_tv_approximate, _approx),
    Step("tv e-step [tv_batch 16 tv_acc_mb 0]", s_tv_estep_batches, ("gmmiv_tv_estimate_a_and_c",), opts={"tv_batch": TV_BATCH, "tv_acc_mb": 0}),
    Step("tv e-step [chol_gemm 1]", s_tv_estep_chol_gemm, ("gmmiv_tv_estimate_a_and_c",), opts={"chol_gemm": 1}),
    Step("tv tett [tv_tett_direct 0]", s_tv_tett, ("gmmiv_tv_tett",), opts={"tv_tett_direct": 0}),
    Step("tv update_t [tv_mstep_solve 0]", s_tv_update_t, ("gmmiv_tv_update_t",), opts={"tv_mstep_solve": 0}),
    Step("tv min_divergence [tv_md_device 0]", s_tv_min_divergence, ("gmmiv_tv_min_divergence",), opts={"tv_md_device": 0}),
    Step("dgemm split-K", s_dgemm_splitk, ("gmmiv_dgemm",)),
    Step("dgemm split-K [gemm_nt80 0]", s_dgemm_splitk, ("gmmiv_dgemm",), opts={"gemm_nt80": 0}),
    Step("iv_normalize", s_iv_normalize, ("gmmiv_iv_normalize",)),
    Step("dev set", s_dev_set, ("gmmiv_dev_means", "gmmiv_dev_cov_mat", "gmmiv_dev_wccn_chol", "gmmiv_dev_mahalanobis", "gmmiv_dev_scatter_mat")),
    Step("eigen", s_eigen, ("gmmiv_sym_eigen", "gmmiv_dev_efr_matrix", "gmmiv_dev_lda")),
    Step("plda", s_plda, ("gmmiv_plda_em_iteration", "gmmiv_plda_precompute", "gmmiv_twocov_model")),
    Step("score rules", s_score_rules, ("gmmiv_score_cosine", "gmmiv_score_mahalanobis", "gmmiv_score_twocov", "gmmiv_score_twocov_mix_part",
                                        "gmmiv_score_plda", "gmmiv_score_apply_trials")),
    Step("score trials", s_score_trials, ("gmmiv_score_cosine_trials", "gmmiv_score_mahalanobis_trials", "gmmiv_score_twocov_trials",
                                          "gmmiv_score_plda_trials")),
    Step("jfa", s_jfa, ("gmmiv_jfa_subtract", "gmmiv_jfa_subtract_sessions", "gmmiv_jfa_estimate_z", "gmmiv_jfa_estimate_z_and_d")),
)
BACKEND_FROM = "tv centre"       # the first step of the i-vector back end
STEPS = {s.name: s for s in PROGRAMME}
# reached by the plumbing of every sequence (Handles, Step.run, nan_calls, workspace_table), not by one step
PLUMBING = ("gmmiv_ctx_create", "gmmiv_ctx_destroy", "gmmiv_ctx_sync", "gmmiv_ctx_set_option", "gmmiv_ctx_kernel_launches", "gmmiv_ctx_workspace_bytes",
            "gmmiv_gmm_create", "gmmiv_gmm_destroy", "gmmiv_gmm_batch_create", "gmmiv_gmm_batch_load", "gmmiv_gmm_batch_load_cov",
            "gmmiv_gmm_batch_destroy", "gmmiv_score_cosine", "gmmiv_dgemm")
# reached by the used-handle tests of tests/test_gpu_ws_history.py: C entry point -> the binding's method those tests call
HANDLE_TESTS = {"gmmiv_gmm_set": "set", "gmmiv_gmm_set_cov": "set_cov", "gmmiv_gmm_batch_packed": "packed"}
_NO_WS = "no workspace: no `scratch(` in its body"
_COMM = "communicator"
EXEMPT_REASONS = (_NO_WS, _COMM)
EXEMPT = {
    "gmmiv_ctx_set_hook": _NO_WS, "gmmiv_ctx_last_kernel_ms": _NO_WS, "gmmiv_ctx_kernel_ms": _NO_WS, "gmmiv_trial_piece": _NO_WS,
    "gmmiv_ctx_stream": _NO_WS, "gmmiv_iv_trial_piece": _NO_WS,
    "gmmiv_comm_create": _COMM,
}


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


NAN_TV = (18, 14, 91, 129)      # the odd-rank dirtying chain: the GEMM-built SPD route, nine batches under tv_batch 16
NAN_DEV = (37, 261, 603)
NAN_IVN = (67, 41, 259)
NAN_JFA = (9, 14, 8, 15, 41)     # C, D, R, speakers, sessions
NAN_SCORE = (131, 259, 261)
NAN_EM = (37, 8, 6)
NAN_RUNS = (40, 10, TURN_W, TURN_S)     # files, runs of 290 frames per file, the windows of the turn calls: 400 runs, 37 600 positions


def nan(*shape):
    return np.full(shape, np.nan)


def all_nan(*arrays):
    return all(bool(np.isnan(host(a)).all()) for a in arrays)


def not_positive_definite(call):
    """a call with an SPD system in it, all of its data NaN: GMMIV_ERR_NUMERIC "not positive definite" and nothing else.  A HIP error
    (-2) is not data any more: it goes up, and the module starts nothing on the GPU after it"""
    from lia_ral_amd import capi
    try:
        call()
    except capi.GmmivError as e:
        if "error -2" in str(e):
            raise
        return "gmmiv error -4" in str(e) and "not positive definite" in str(e)
    return False


def nan_calls(ctx):
    """the NaN-as-data calls that finish a large pass, one per family of the back end at a large odd shape -- and one each of windowed
    NormFeat and TurnDetection above the judged sizes -- host arrays in (they are
    staged through the shared WS_T* / WS_X / WS_LSE / WS_PART / WS_TIV / WS_IVT_* slots, which hold NaN afterwards) -> {call: whether it
    answered as it must}: NaN everywhere from a call without an SPD system, "not positive definite" from one with; the last entry is a
    finite call the context must still serve"""
    t = _torch()
    ok = {}
    dim, M, S = NAN_SHAPE
    ok["score_cosine"] = all_nan(ctx.score_cosine(nan(dim, M), nan(dim, S)))
    A = t.full((130, 70), float("nan"), dtype=t.float64, device="cuda")
    B = t.full((70, 90), float("nan"), dtype=t.float64, device="cuda")
    Cm = t.zeros((130, 90), dtype=t.float64, device="cuda")
    ctx.dgemm(0, 0, 1.0, A, B, 0.0, Cm)
    t.cuda.synchronize()
    ok["dgemm"] = bool(t.isnan(Cm).all().item())
    # the T-matrix chain
    C, D, R, U = NAN_TV
    P, SV = R * (R + 1) // 2, C * D
    ok["tv_subtract_m"] = all_nan(ctx.tv_subtract_m(nan(U, C), nan(U, SV), nan(SV), C, D))
    ok["tv_tett"] = all_nan(ctx.tv_tett(nan(R, SV), nan(SV), C, D))
    with options(ctx, {"tv_batch": TV_BATCH}):
        ok["tv_estimate_w"] = not_positive_definite(lambda: ctx.tv_estimate_w(nan(U, C), nan(U, SV), nan(R, SV), nan(SV), nan(C, P), C, D))
        ok["tv_estimate_a_and_c"] = not_positive_definite(lambda: ctx.tv_estimate_a_and_c(nan(U, C), nan(U, SV), nan(R, SV), nan(SV), nan(C, P), C, D))
    ok["tv_update_t"] = not_positive_definite(lambda: ctx.tv_update_t(nan(C, P), nan(R, SV), C, D))
    ok["tv_min_divergence"] = not_positive_definite(lambda: ctx.tv_min_divergence(nan(R, R), nan(R), nan(R), nan(SV), nan(R, SV), 50, C, D))
    ok["tv_norm_t"] = all_nan(ctx.tv_norm_t(nan(R, SV), nan(SV), C, D))
    ok["tv_estimate_w_eigen"] = all_nan(ctx.tv_estimate_w_eigen(nan(U, C), nan(U, SV), nan(R, SV), nan(C, R), nan(R, R), C, D))
    # the development set
    dim, nspk, longest = NAN_DEV
    sps = _dev_large(*NAN_DEV)[1]
    X = nan(dim, int(sps.sum()))
    ok["dev_means"] = all_nan(*ctx.dev_means(X, sps))
    ok["dev_cov_mat"] = all_nan(*ctx.dev_cov_mat(X, sps))
    ok["dev_scatter_mat"] = all_nan(*ctx.dev_scatter_mat(X, sps))
    ok["dev_mahalanobis"] = not_positive_definite(lambda: ctx.dev_mahalanobis(X, sps))
    ok["dev_wccn_chol"] = not_positive_definite(lambda: ctx.dev_wccn_chol(X, sps))
    # iv_normalize, JFA
    din, dout, n = NAN_IVN
    ok["iv_normalize"] = all_nan(ctx.iv_normalize(nan(din, n), nan(din), nan(dout, din), True))
    C, D, R, nspk, nsess = NAN_JFA
    SV = C * D
    ok["jfa_subtract"] = all_nan(ctx.jfa_subtract(nan(nspk, C), nan(nspk, SV), C, D, means=nan(SV), T=nan(R, SV), W=nan(nspk, R), Dm=nan(SV), Z=nan(nspk, SV)))
    sb = np.concatenate([[0], np.cumsum(JFA_SESSIONS_LARGE[1])]).astype(np.int64)
    ok["jfa_subtract_sessions"] = all_nan(ctx.jfa_subtract_sessions(sb, nan(nsess, C), nan(nspk, SV), nan(R, SV), nan(nsess, R), C, D)[np.diff(sb) > 0])
    ok["jfa_estimate_z"] = all_nan(ctx.jfa_estimate_z(nan(nspk, C), nan(nspk, SV), nan(SV), nan(SV), C, D))
    Dm = nan(SV)
    ok["jfa_estimate_z_and_d"] = all_nan(ctx.jfa_estimate_z_and_d(nan(nspk, C), nan(nspk, SV), nan(SV), Dm, C, D), Dm)
    # the four rules on a trial list: NaN vectors under finite matrices
    dim, M, S = NAN_SCORE
    p = br.score_case(dim, M, S, "plain")
    tm, ts = ivr.trial_list("sparse", M, S)
    ok["score_cosine_trials"] = all_nan(ctx.score_cosine_trials(nan(dim, M), nan(dim, S), tm, ts))
    ok["score_mahalanobis_trials"] = all_nan(ctx.score_mahalanobis_trials(nan(dim, M), nan(dim, S), p["Mah"], tm, ts))
    ok["score_twocov_trials"] = all_nan(ctx.score_twocov_trials(nan(dim, M), nan(dim, S), p["G"], p["H"], tm, ts))
    ok["score_plda_trials"] = all_nan(ctx.score_plda_trials(nan(dim, M), p["nsess"], nan(dim, S), p["FTJF"], tm, ts))
    ok["score_plda_trials NaN FTJF"] = not_positive_definite(lambda: ctx.score_plda_trials(nan(dim, M), p["nsess"], nan(dim, S), nan(dim, dim), tm, ts))
    # windowed NormFeat and TurnDetection, host tables: more files, runs, steps and positions than any judged case, NaN frames
    from lia_ral_amd import capi
    nf, per, W, S = NAN_RUNS
    big = np.array([[i * 3000 + k * 300, 290, i] for i in range(nf) for k in range(per)], np.int64)
    xb = t.full((nf * 3000, 70), float("nan"), dtype=t.float64, device="cuda")
    ob, sb, ab = capi.plan_norm_windows(big, nf, big[::per, 0].copy(), 5.0, 1.0, 0.01)
    ok["feat_norm_window"] = len(ab) > max(run_sizes(c)["nsteps"] for c in SMALL) and all_nan(*ctx.feat_norm_window(xb, big, nf, ob, sb, nan(len(ab))))
    po = capi.plan_turn_positions(big, nf, W, S)
    value, status = ctx.turn_curve(xb[:, :TURN_COLS], big, nf, po, W, S, "DGLR")
    ok["turn_curve"] = all_nan(value) and bool((status == tn.BAD_COV).all()) and len(value) == per * nf * tn.positions_as_written(290, W, S)
    sm, dec, rs, nt = ctx.turn_pick(value, po, 0.5)
    ok["turn_pick"] = all_nan(sm, rs) and not dec.any() and not nt.any()
    # PLDA EM
    dim, rf, rg = NAN_EM
    n = int(sps.sum())
    ok["plda_em_iteration"] = not_positive_definite(lambda: ctx.plda_em_iteration(nan(dim, n), sps, nan(dim, rf), nan(dim, rg), nan(dim, dim), nan(dim)))
    fin = br.score_case(5, 3, 7, "plain")
    ok["a finite call after them"] = bool(np.isfinite(ctx.score_cosine(fin["m"], fin["s"])).all())
    return ok


def workspace_table(ctx):
    return [ctx.workspace_bytes(i) for i in range(64)]


def run_sequence(name, moved=None):
    """one context, the passes of SEQUENCES[name] -> dict(results {(case, step, form): outputs}, seconds {...}, ws [(pass, table)],
    nan {call: answered as it must}, nan_ok, log, total).  moved: {step name: options} set for that step of the FIRST pass only and put back after it"""
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
                res["nan"] = nan_calls(ctx)
                ok = all(res["nan"].values())
                res["nan_ok"] = ok if res["nan_ok"] is None else (res["nan_ok"] and ok)
            res["ws"].append(("large" if cases is LARGE else "small", workspace_table(ctx)))
    finally:
        h.close()
        ctx.close()
    res["total"] = time.perf_counter() - t_all
    return res
