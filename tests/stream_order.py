"""The late-producer mode of the programme of tests/ws_history.py (tests/test_gpu_stream_order.py, tests/test_cpu_stream_order.py).

include/gmmiv.h, "STREAM ORDER": a device array is read and written in the order of the context's stream.  Every other test hands the
library inputs that are complete before the call is made, so a read from another stream -- or by the host, before the stream has
reached the call -- sees the right data all the same.  Here the inputs of a call are wrong when the call is made and become right
only ON THE CONTEXT'S STREAM, behind a spin kernel: whoever reads them out of stream order reads poison.

Recorder    what ws_history.dev() registers while ws_history.RECORDER is set: every device tensor of the running step with its role
            ("in": dev() / to(), "out": buf(), "inout": mut()), a staging copy of its true data, its poison and a snapshot buffer.
LateLib     stands in for capi.lib.  Every gmmiv_* call but those of the context, the planners and the communicator (plain()) goes
            through late_call(): see there for the seven steps.
Backend     the device operations the two need (torch on the GPU; the CPU test has one on numpy arrays that logs).

Plain numpy at import; torch is touched only by TorchBackend.
"""
import ctypes as ct
import re
import time

import numpy as np

import gmm_ref as gr
import ws_history as wh
from test_cpu_ws_history import abi_functions

SPIN_CYCLES = 20_000_000         # torch.cuda._sleep in front of the restoring copies: about 10 ms (the figure of the enqueue tests: 2e9 ~ 1 s)

# ---------------------------------------------------------------------------------------------------------------- the ABI
_HANDLE = re.compile(r"\b(gmmiv_ctx|gmmiv_gmm|gmmiv_gmm_batch|gmmiv_comm|gmmiv_hook_fn)\b|(?<!unsigned )\bchar\b")
_PLANNERS = ("gmmiv_em_acc_len", "gmmiv_tv_packed_len", "gmmiv_shard_range", "gmmiv_energy_stage_frames", "gmmiv_trial_piece",
             "gmmiv_score_list_class", "gmmiv_iv_trial_piece", "gmmiv_iv_trial_anchor", "gmmiv_turn_tile_positions")
_COLLECTIVE = re.compile(r"gmmiv_(allreduce|reduce_scatter|allgather|broadcast)_f64(_begin)?$")


def plain(name):
    """whether the proxy forwards `name` as it is: the context, planner and communicator functions (the rows of
    test_cpu_judged_inventory.EXEMPT with those reasons, and gmmiv_plan_norm_windows, a planner that is judged because it hands back
    doubles; the handle functions are NOT among them -- they take device arrays)"""
    return (name.startswith(("gmmiv_ctx_", "gmmiv_comm_", "gmmiv_plan_")) or name in ("gmmiv_last_error", "gmmiv_version") or name in _PLANNERS
            or bool(_COLLECTIVE.match(name)))


def prototypes():
    """{function: [(parameter name, 'scalar' | 'handle' | 'read' | 'written')]} from the headers of include/: a pointer to const is read, any
    other array pointer is written (and perhaps read)"""
    out = {}
    for name, text in abi_functions().items():
        params = []
        for p in (q.strip() for q in text.split(",")):
            if not p or p == "void":
                continue
            pname = re.findall(r"[A-Za-z_][A-Za-z_0-9]*", p)[-1]
            if "*" not in p:
                kind = "scalar"
            elif _HANDLE.search(p):
                kind = "handle"
            else:
                kind = "read" if re.match(r"const\b", p) else "written"
            params.append((pname, kind))
        out[name] = params
    return out


def address(arg):
    """the address a ctypes argument carries: an int, 0 for NULL, or None for what is no c_void_p (a byref: a host scalar)"""
    if arg is None:
        return 0
    if isinstance(arg, ct.c_void_p):
        return arg.value or 0
    return None


# ---------------------------------------------------------------------------------------------------------------- poison
def is_float(a):
    return a.dtype.is_floating_point if hasattr(a.dtype, "is_floating_point") else np.issubdtype(a.dtype, np.floating)


def poison(a):
    """floating: -(a) - 1 -- finite wherever a is and different from it in every element but an exact -0.5 (register() refuses one) -- and
    1 where a itself is NaN or infinite (planted statistics): never NaN or Inf, which would take the screened paths and move the
    counters; an integer or byte table: all zeros, used only where ZERO_IS_VALID names the parameter and NOT_LATE does not"""
    if not is_float(a):
        return a * 0
    if type(a).__module__.startswith("torch"):
        import torch
        return torch.where(torch.isfinite(a), -a - 1, torch.ones_like(a))
    return np.where(np.isfinite(a), -a - 1, np.ones_like(a))


# (step, parameter of the ABI function the table is passed as, the reason): integer device tables that are uploaded complete, because
# the header does not make 0 a valid value of every element.  Integer tables only; every floating-point array is late.
NOT_LATE = (
    ("gather + scatter runs", "runs", "include/gmmiv.h, gmmiv_gather_runs / gmmiv_scatter_runs: rows of (source frame, output row, length) that 'must not "
     "overlap' in the written matrix, and no sentence makes a run of length 0 valid: all-zero rows would all name row 0"),
    ("normfeat window", "step_off", "include/gmmiv_feat_window.h: the CSR of the steps per file; a host table that does not end at nsteps is refused, and no "
     "sentence makes a CSR of zeros valid when there are steps"),
    ("normfeat window", "steps", "include/gmmiv_feat_window.h: rows of (window lo, window hi, apply lo, apply hi) with 'lo <= apply lo < apply hi <= hi': "
     "an all-zero row breaks apply lo < apply hi"),
    ("turn detection", "pos_off", "include/gmmiv_turn.h: 'the CSR of gmmiv_plan_turn_positions for the same (W, S)'; a host table that does not end at npos "
     "is refused, and no sentence makes a CSR of zeros valid when there are positions"),
)
# the integer tables that ARE late, with the sentence of the header that makes an all-zero table valid
ZERO_IS_VALID = {
    "frame_idx": "gmmiv_gather_frames: out[i] = x[frame_idx[i]]: 0 is a frame of x",
    "runs": "RUN TABLE (first frame, length, group / file): ids non-decreasing in [0, n), 'files / runs without frames are valid'",
    "file_begin": "gmmiv_feat_norm_online: 'nfiles = 0 and files / runs without frames are valid': all offsets 0 are empty files",
    "row_id": "gmmiv_score_normalize_list: an id in [0, nrow)",
    "col_id": "gmmiv_score_normalize_list: an id in [0, ncol)",
    "trials": "gmmiv_score_apply_trials: a flag byte, 0 = fill the cell",
    "owner": "gmmiv_jfa_subtract: o = owner[r] is one of the nfact factor rows, and 0 is one",
    "dec": "gmmiv_turn_segments: a run 'is cut after frame b + W - 1 + i S of every i with dec[i] != 0': a table of zeros cuts nowhere",
    "seg_off": "gmmiv_turn_segments: 'Segments beyond a file's CSR room are not written': offsets that are all 0 are files without room",
}


# ---------------------------------------------------------------------------------------------------------------- the recorder
class Item:
    def __init__(self, t, role, true, bad, snap, first):
        self.t, self.role, self.true, self.bad, self.snap, self.first = t, role, true, bad, snap, first
        self.written = role != "in" and role != "inout"   # an output is never made late
        self.param = None                                  # the ABI parameter it was first passed as
        self.pending = False                               # snap holds the content right behind the last call


class Recorder:
    """the device tensors of one late step"""

    def __init__(self, backend):
        self.be, self.items = backend, []

    def register(self, t, role):
        assert role in ("in", "out", "inout"), role
        true = self.be.clone(t)
        bad = poison(true)
        if is_float(true):
            assert self.be.all_true((bad != true) & (bad == bad) & (abs(bad) < float("inf"))), "the poison must be finite and differ in every element"
        self.items.append(Item(t, role, true, bad, self.be.empty_like(t), self.be.first(bad)))

    def inputs(self):
        return [it for it in self.items if it.role == "in"]

    def outputs(self):
        return [it for it in self.items if it.role != "in"]


class LateLib:
    """capi.lib for one late step.  records: one dict per late call (function, device arrays throughout, stream busy on return, seconds
    on the host, inputs made late); faults: what rules (b) and the probe found; log: the actions in order (the CPU test reads it)"""

    def __init__(self, real, recorder, ctx_handle, step_name, spin=SPIN_CYCLES, protos=None):
        self.real, self.rec, self.h, self.step, self.spin = real, recorder, ctx_handle, step_name, spin
        self.protos = prototypes() if protos is None else protos
        self.not_late = {(s, p) for s, p, _ in NOT_LATE}
        self.records, self.faults, self.log = [], [], []

    def __getattr__(self, name):
        f = getattr(self.real, name)
        if not name.startswith("gmmiv_") or plain(name):
            return f
        return lambda *args: self.late_call(name, f, args)

    # -- the pieces
    def bind(self, name, args):
        """-> whether every array of the call lies in device memory; items get the parameter they are passed as, and an item passed
        through a pointer to non-const is the call's to write: it is late for THIS call and an in/out array from then on"""
        be, params = self.rec.be, self.protos[name]
        assert len(params) == len(args), "%s: %d arguments for %d parameters" % (name, len(args), len(params))
        throughout, now_written = True, []
        for (pname, kind), arg in zip(params, args):
            if kind in ("scalar", "handle"):
                continue
            a = address(arg)
            if a == 0:
                continue
            if a is None or not be.on_device(a):
                throughout = False
                continue
            for it in self.rec.items:
                lo, n = be.span(it.t)
                if lo <= a < lo + max(n, 1):
                    if it.param is None:
                        it.param = pname
                    if kind == "written" and not it.written:
                        now_written.append(it)
        return throughout, now_written

    def check_snapshots(self):
        """rule (b): the context is synchronised; a snapshot taken right behind the last call holds what its buffer holds now"""
        for k, it in enumerate(self.rec.items):
            if it.pending:
                it.pending = False
                if not self.rec.be.same_bits(it.snap, it.t):
                    self.faults.append("tensor %d (%s, passed as %s): the snapshot enqueued behind the call differs from the buffer after the stream was "
                                       "synchronised -- something wrote it out of stream order" % (k, it.role, it.param))

    def late_call(self, name, f, args):
        be = self.rec.be
        be.ctx_sync(self.h)                                                        # 1
        self.log.append(("sync", name))
        self.check_snapshots()
        throughout, now_written = self.bind(name, args)
        late = []
        for it in self.rec.items:
            if it.written or be.span(it.t)[1] == 0:
                continue
            if is_float(it.t):
                late.append(it)
            elif it.param is not None and (self.step, it.param) not in self.not_late:    # an integer table: zeros, where the header allows them
                if it.param in ZERO_IS_VALID:
                    late.append(it)
                else:
                    self.faults.append("%s: the integer table passed as %r is named neither in ZERO_IS_VALID nor in NOT_LATE" % (name, it.param))
        for it in late:                                                            # 2
            be.write_now(it.t, it.bad)
            self.log.append(("poison", id(it)))
        be.spin(self.spin)                                                         # 3 (the spin also without a late input: rule (c) reads the stream)
        self.log.append(("spin", self.spin))
        for it in late:
            be.enqueue_copy(it.t, it.true)
            self.log.append(("restore", id(it)))
        ev = be.mark()
        if late:
            seen = be.probe(late[0].t)                                             # 4
            self.log.append(("probe", id(late[0])))
            if seen != late[0].first:
                self.faults.append("%s: the probe read %r, not the poison %r: the restoring copies did not wait behind the spin" % (name, seen, late[0].first))
        t0 = time.perf_counter()
        self.log.append(("forward", name))
        try:
            rc = f(*args)                                                          # 5
        finally:
            seconds = time.perf_counter() - t0
            busy = be.busy(ev)                                                     # 6
            self.log.append(("busy", busy))
            self.records.append(dict(fn=name, throughout=throughout, busy=busy, seconds=seconds, late=len(late)))
        for it in now_written:
            it.written = True
        for it in self.rec.items:                                                  # 7
            if it.written:
                be.enqueue_copy(it.snap, it.t)
                it.pending = True
                self.log.append(("snapshot", id(it)))
        return rc

    def finish(self):
        """after the step has synchronised its context: the last snapshots"""
        self.rec.be.ctx_sync(self.h)
        self.check_snapshots()


class TorchBackend:
    def __init__(self, real, ctx):
        import torch
        self.t, self.real = torch, real
        self.stream = ctx.torch_stream()
        self.side = self.beside()
        self._ranges = None

    def beside(self):
        """a stream that RUNS beside the context's: streams share a few hardware queues, and a copy on a stream that shares the context's
        queue waits behind the spin like the context's own work -- the probe would then see the restored data and prove nothing"""
        t = self.t
        src = t.zeros(1, device="cuda")
        t.cuda.current_stream().synchronize()
        for _ in range(12):
            s = t.cuda.Stream()                            # torch's pool streams are non-blocking: not ordered with the NULL stream either
            if s.cuda_stream == self.stream.cuda_stream:
                continue
            with t.cuda.stream(self.stream):
                t.cuda._sleep(SPIN_CYCLES)
            ev = self.stream.record_event()
            with t.cuda.stream(s):
                src.cpu()
            s.synchronize()
            ran_beside = not ev.query()
            self.stream.synchronize()
            if ran_beside:
                return s
        raise AssertionError("no stream was found whose copies run while the context's stream spins")

    def ctx_sync(self, h):
        assert self.real.gmmiv_ctx_sync(h) == 0
        self.t.cuda.current_stream().synchronize()

    def clone(self, t):
        out = t.clone()
        self.t.cuda.current_stream().synchronize()
        return out

    def empty_like(self, t):
        return self.t.empty_like(t)

    def all_true(self, m):
        return bool(m.all().item())

    def first(self, t):
        return t.flatten()[0].item() if t.numel() else None

    def span(self, t):
        return t.data_ptr(), t.numel() * t.element_size()

    def on_device(self, a):
        if self._ranges is None or not any(lo <= a < hi for lo, hi in self._ranges):
            self._ranges = [(s["address"], s["address"] + s["total_size"]) for s in self.t.cuda.memory_snapshot()]
        return any(lo <= a < hi for lo, hi in self._ranges)

    def write_now(self, dst, src):
        dst.copy_(src)
        self.t.cuda.current_stream().synchronize()

    def spin(self, n):
        with self.t.cuda.stream(self.stream):
            self.t.cuda._sleep(int(n))

    def enqueue_copy(self, dst, src):
        with self.t.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)

    def mark(self):
        return self.stream.record_event()

    def busy(self, ev):
        return not ev.query()

    def probe(self, t):
        with self.t.cuda.stream(self.side):
            v = t.flatten()[:1].cpu()
        self.side.synchronize()
        return v[0].item()

    def same_bits(self, a, b):
        if a.numel() == 0:
            return True
        as_int = {1: self.t.uint8, 2: self.t.int16, 4: self.t.int32, 8: self.t.int64}[a.element_size()]
        return bool(self.t.equal(a.contiguous().view(as_int), b.contiguous().view(as_int)))


# ---------------------------------------------------------------------------------------------------------------- the handles step
def s_handles(ctx, h, case, form):
    """gmm_set, gmm_set_cov, gmm_batch_load and gmm_batch_load_cov from device arrays, each followed by a likelihood call on resident
    frames: the model uploads read their arrays in stream order too.  The handles are this step's own (a set() changes the model)"""
    C, D, T, _ = case["gcase"]
    x = wh.to(form, wh.frames(case, form))
    w, mean, iv = gr.model(case["gcase"], 31)
    w2, mean2, iv2 = gr.model(case["gcase"], 32)
    g = h.get((case["name"], "set"), lambda: ctx.gmm(*gr.model(case["gcase"], 30)))
    out = {}
    g.set(wh.to(form, w), wh.to(form, mean), wh.to(form, iv))
    out["llk after set"] = g.llk(x, *wh.WIDE, out=wh.buf(form, (T,)))
    g.set_cov(wh.to(form, w2), wh.to(form, mean2), wh.to(form, np.ascontiguousarray(1.0 / iv2)))
    out["llk after set_cov"] = g.llk(x, *wh.WIDE, out=wh.buf(form, (T,)))
    b = h.get((case["name"], "load"), lambda: ctx.gmm_batch(case["G"], C, D))
    bw, bm, biv = wh._batch_models(case["name"])
    sb, sm = wh.seg_table(case)
    b.load(wh.to(form, bw), wh.to(form, bm), wh.to(form, biv))
    out["batch llk after load"], out["seg_sum after load"] = b.llk(x, sb, sm, *wh.WIDE, out=wh.buf(form, (T,)), seg_sum=wh.buf(form, (len(sm),)))
    b.load_cov(wh.to(form, bw[0].copy()), wh.to(form, bm), wh.to(form, np.ascontiguousarray(1.0 / biv[0])))
    out["batch llk after load_cov"], out["seg_sum after load_cov"] = b.llk(x, sb, sm, *wh.WIDE, out=wh.buf(form, (T,)), seg_sum=wh.buf(form, (len(sm),)))
    return out


HANDLES = wh.Step("handles", s_handles, ("gmmiv_gmm_create", "gmmiv_gmm_set", "gmmiv_gmm_set_cov", "gmmiv_gmm_batch_create", "gmmiv_gmm_batch_load",
                                         "gmmiv_gmm_batch_load_cov", "gmmiv_llk", "gmmiv_llk_models"))
LATE_PROGRAMME = wh.PROGRAMME + (HANDLES,)

# ---------------------------------------------------------------------------------------------------------------- the header's table
E, W, S = "enqueues", "waits", "silent"
_GENERAL = "DEGENERATE INPUTS: 'a call whose arrays are all device pointers only enqueues on the context's stream' (the frame-consuming calls; " \
           "the exceptions are named there)"
_EXCEPT = "DEGENERATE INPUTS: named among the calls that wait (fallback flags / top-1 selection / a table upload)"
_NORM = "NormFeat: 'with device pointers throughout every call only enqueues on the context's stream'"
_NORMWIN = "gmmiv_feat_window.h: 'with device pointers throughout, gstat / step_stat included, the call only enqueues on the context's stream'"
_TURN = "gmmiv_turn.h: 'with device pointers throughout a call only enqueues on the context's stream'"
_MODELS = "'the call waits once for its table upload, like the other *_models calls'"
_SILENT = "no sentence on synchronisation"
_IVT = "gmmiv_iv_trials.h: 'NOT enqueue-only: it waits for the context's stream once after uploading its tables'"
# ABI function -> (what its header says of a call with device pointers throughout, the sentence).  Rule (c) of
# tests/test_gpu_stream_order.py holds the E rows: every late call with device arrays throughout returns with the stream busy.
ENQUEUE_ONLY = {
    "gmmiv_llk": (E, _GENERAL), "gmmiv_occ": (E, _GENERAL), "gmmiv_em_accumulate": (E, _GENERAL), "gmmiv_llk_use_top": (E, _GENERAL),
    "gmmiv_llk_use_top_multi": (E, _GENERAL), "gmmiv_frame_moments": (E, _GENERAL),
    "gmmiv_llk_determine_top": (W, _EXCEPT), "gmmiv_topgauss_compute": (W, _EXCEPT), "gmmiv_tv_stats": (W, _EXCEPT), "gmmiv_tv_stats_lines": (W, _EXCEPT),
    "gmmiv_count_unusable_frames": (W, "'this call waits for the stream'"),
    "gmmiv_gather_frames": (S, _SILENT),
    "gmmiv_gather_runs": (E, "'with a device table the call only enqueues on the context's stream (no synchronisation)'"),
    "gmmiv_scatter_runs": (E, "'a device table only enqueues'"),
    "gmmiv_plan_norm_windows": (S, "pure host, no frame data and no context: the proxy forwards it untouched (plain())"),
    "gmmiv_feat_norm_window": (E, _NORMWIN), "gmmiv_turn_curve": (E, _TURN), "gmmiv_turn_pick": (E, _TURN), "gmmiv_turn_segments": (E, _TURN),
    "gmmiv_frame_moments_groups": (E, _NORM), "gmmiv_frame_moments_stats": (E, _NORM), "gmmiv_feat_norm_apply": (E, _NORM), "gmmiv_feat_norm_online": (E, _NORM),
    "gmmiv_energy_train": (E, "'with device pointers throughout both calls only enqueue on the context's stream'"),
    "gmmiv_energy_select": (E, "'with device pointers throughout both calls only enqueue on the context's stream'"),
    "gmmiv_segment_means": (S, _SILENT), "gmmiv_em_get": (S, _SILENT), "gmmiv_variance_control": (S, _SILENT),
    "gmmiv_feat_compensate": (E, "'with device pointers throughout gmmiv_feat_compensate only enqueues'"),
    "gmmiv_feat_map": (W, "'gmmiv_feat_map waits once for its top-1 selection, like gmmiv_llk_determine_top'"),
    "gmmiv_llk_models": (W, _MODELS), "gmmiv_tv_stats_models": (W, _MODELS), "gmmiv_em_stats_models": (W, _MODELS), "gmmiv_feat_compensate_models": (W, _MODELS),
    "gmmiv_llr_trials": (W, "'the call is NOT enqueue-only.  It waits for the context's stream once after uploading its tables'"),
    "gmmiv_map_adapt_models": (S, _SILENT), "gmmiv_map_adapt_models_full": (S, _SILENT), "gmmiv_normalize_models": (S, _SILENT),
    "gmmiv_mllr_adapt_models": (E, "'The call never reads the status back: with device arrays it only enqueues.'"),
    "gmmiv_dgemm": (E, "'Only enqueues: gmmiv_ctx_sync (or the stream) orders the result.'"),
    "gmmiv_score_cohort_stats": (E, "'With device pointers throughout both calls only enqueue.'"),
    "gmmiv_score_normalize": (E, "'With device pointers throughout both calls only enqueue.'"),
    "gmmiv_score_list_stats": (W, "'the call is NOT enqueue-only: it waits for the context's stream once, after uploading its two tables'"),
    "gmmiv_score_normalize_list": (E, "'Only enqueues with device arrays.'"),
    "gmmiv_score_cosine_trials": (W, _IVT), "gmmiv_score_mahalanobis_trials": (W, _IVT), "gmmiv_score_twocov_trials": (W, _IVT), "gmmiv_score_plda_trials": (W, _IVT),
}
for _name in ("tv_subtract_m", "tv_subtract_m_to", "tv_tett", "tv_estimate_w", "tv_estimate_a_and_c", "tv_update_t", "tv_min_divergence", "tv_orthonormalize_t",
              "tv_norm_statistics", "tv_subtract_m_plus_tw", "tv_norm_t", "tv_weighted_cov", "tv_approximate_tctc", "tv_estimate_w_ubm_weight",
              "tv_estimate_w_eigen", "iv_normalize", "dev_means", "dev_cov_mat", "dev_scatter_mat", "dev_wccn_chol", "dev_mahalanobis", "sym_eigen",
              "dev_efr_matrix", "dev_lda", "plda_em_iteration", "plda_precompute", "twocov_model", "score_cosine", "score_mahalanobis", "score_twocov",
              "score_plda", "score_twocov_mix_part", "score_apply_trials", "jfa_subtract", "jfa_subtract_sessions", "jfa_estimate_z", "jfa_estimate_z_and_d"):
    ENQUEUE_ONLY["gmmiv_" + _name] = (S, _SILENT)     # the i-vector back end: host factorisations and per-call allocations wait where they must
