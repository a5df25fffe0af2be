"""ctypes binding of include/gmmiv.h.  Arrays may be numpy arrays (host) or torch CUDA tensors
(device, used in place).  Raises GmmivError on any non-zero status -- never falls back to a CPU path."""
import ctypes as ct
import os
import sys
import weakref

import numpy as np

try:  # PyTorch-ROCm bundles its own HIP runtime: load it first so the process holds ONE runtime
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the binding itself
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
# GMMIV_LIB_PATH: development knob (tools/k1_ablate.sh times instrumented builds of the same library); still libgmmiv, never a fallback
LIB_PATH = os.environ.get("GMMIV_LIB_PATH") or os.path.join(_HERE, "csrc", "libgmmiv.so")

F32, F64 = 0, 1
NORMWIN_CMS, NORMWIN_VAR = 1, 2  # include/gmmiv_feat_window.h
TURN_GLR, TURN_DGLR, TURN_BIC = 0, 1, 2  # include/gmmiv_turn.h
TURN_BAD_COV, TURN_CLAMPED = 1, 2
TURN_CRIT = {"GLR": TURN_GLR, "DGLR": TURN_DGLR, "BIC": TURN_BIC}
TOP_PARTIAL, TOP_COMPLETE = 0, 1


class GmmivError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        raise GmmivError("libgmmiv.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'` "
                         "or `make -C lia_ral_amd/csrc`" % LIB_PATH)
    lib = ct.CDLL(LIB_PATH)
    lib.gmmiv_last_error.restype = ct.c_char_p
    lib.gmmiv_version.restype = ct.c_char_p
    lib.gmmiv_em_acc_len.restype = ct.c_size_t
    lib.gmmiv_tv_packed_len.restype = ct.c_size_t
    lib.gmmiv_ctx_last_kernel_ms.restype = ct.c_double
    lib.gmmiv_ctx_kernel_ms.restype = ct.c_double
    lib.gmmiv_ctx_kernel_launches.restype = ct.c_long
    lib.gmmiv_ctx_set_option.restype = ct.c_long
    lib.gmmiv_comm_backend.restype = ct.c_char_p
    lib.gmmiv_comm_take_bytes.restype = ct.c_double
    lib.gmmiv_ctx_stream.restype = ct.c_void_p
    lib.gmmiv_plan_model_tiles.restype = ct.c_int64
    lib.gmmiv_plan_feat_tiles.restype = ct.c_int64
    lib.gmmiv_plan_trial_tiles.restype = ct.c_int64
    lib.gmmiv_plan_score_lists.restype = ct.c_int64
    lib.gmmiv_energy_stage_frames.restype = ct.c_int64
    lib.gmmiv_plan_norm_windows.restype = ct.c_int64
    lib.gmmiv_plan_turn_positions.restype = ct.c_int64
    return lib


lib = _load()


def _chk(rc):
    if rc != 0:
        raise GmmivError("gmmiv error %d: %s" % (rc, lib.gmmiv_last_error().decode()))


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a):
    """void* of a numpy array or torch tensor (None -> NULL)."""
    if a is None:
        return ct.c_void_p(0)
    if _is_torch(a):
        assert a.is_contiguous() or (a.dim() == 2 and a.stride(1) == 1)  # feature matrices may be row-strided (ldx)
        return ct.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"]
    return ct.c_void_p(a.ctypes.data)


def _f64(a):
    if a is None or _is_torch(a):
        return a
    return np.ascontiguousarray(a, dtype=np.float64)


def _feat(x):
    """-> (array, dtype code, T, ldx)"""
    if _is_torch(x):
        import torch
        assert x.dim() == 2 and x.stride(1) == 1
        dt = F64 if x.dtype == torch.float64 else F32
        assert x.dtype in (torch.float32, torch.float64)
        return x, dt, x.shape[0], x.stride(0) if x.shape[0] > 1 else x.shape[1]
    x = np.asarray(x)
    if x.dtype not in (np.float32, np.float64):
        x = x.astype(np.float64)
    x = np.ascontiguousarray(x)
    return x, (F64 if x.dtype == np.float64 else F32), x.shape[0], x.shape[1]


def _feat_view(x):
    """-> (array, dtype code, T, ld) WITHOUT a copy: a torch tensor or a numpy array whose rows are contiguous and evenly strided (a
    column slice of a wider matrix keeps its row stride) -- the frames gmmiv_feat_compensate / gmmiv_feat_map read and write"""
    if _is_torch(x):
        return _feat(x)
    assert isinstance(x, np.ndarray) and x.ndim == 2 and x.dtype in (np.float32, np.float64)
    assert x.shape[0] == 0 or x.shape[1] == 0 or x.strides[1] == x.itemsize
    ld = x.strides[0] // x.itemsize if x.shape[0] > 1 else x.shape[1]
    assert x.shape[0] <= 1 or (x.strides[0] % x.itemsize == 0 and ld >= x.shape[1])
    return x, (F64 if x.dtype == np.float64 else F32), x.shape[0], ld


def _feat_like(x, dtype_code):
    """an output frame matrix of the kind of x (numpy / torch device), compact rows"""
    if _is_torch(x):
        import torch
        return torch.empty((x.shape[0], x.shape[1]), dtype=torch.float64 if dtype_code == F64 else torch.float32, device=x.device)
    return np.empty((x.shape[0], x.shape[1]), np.float64 if dtype_code == F64 else np.float32)


def _vptr(a):
    """void* of the first element of a frame view (no contiguity demand beyond _feat_view's)"""
    return ct.c_void_p(a.data_ptr()) if _is_torch(a) else ct.c_void_p(a.ctypes.data)


STREAM_DEFAULT = -1        # GMMIV_STREAM_DEFAULT: launch on the NULL (legacy default) stream, torch's default stream


class Context:
    """stream: a hipStream_t handle (e.g. torch.cuda.current_stream().cuda_stream) or None for a private non-blocking stream.
    The handle 0 -- what torch reports for its DEFAULT stream -- means "the stream torch is using", so it is passed on as
    GMMIV_STREAM_DEFAULT: every call of the context is then ordered with the torch kernels around it (a private stream would not be).
    torch_stream(): the same stream as a torch object, for `with torch.cuda.stream(ctx.torch_stream()):`."""

    def __init__(self, device=0, stream=None):
        self._h = ct.c_void_p()
        self.device = int(device)
        self._models = weakref.WeakSet()   # Gmm / GmmBatch handles of this context: destroyed with it, at the latest
        if stream is not None and int(stream) == 0:
            stream = STREAM_DEFAULT
        _chk(lib.gmmiv_ctx_create(ct.c_int(device), ct.c_void_p(stream or 0), ct.byref(self._h)))

    def stream(self):
        return int(lib.gmmiv_ctx_stream(self._h) or 0)

    def ordered(self):
        """Context manager: the context's stream waits for torch's current stream on entry, torch's current stream waits for
        the context's on exit -- calls made inside see every tensor torch has written and torch sees their results.  A no-op
        when both are the same stream."""
        import contextlib
        import torch
        cur = torch.cuda.current_stream(self.device)
        mine = self.torch_stream()
        if cur.cuda_stream == mine.cuda_stream:
            return contextlib.nullcontext()

        @contextlib.contextmanager
        def bracket():
            mine.wait_stream(cur)
            try:
                yield
            finally:
                cur.wait_stream(mine)
        return bracket()

    def torch_stream(self):
        import torch
        h = self.stream()
        if h == 0:         # the NULL stream
            return torch.cuda.default_stream(self.device)
        return torch.cuda.ExternalStream(h, device=self.device)

    def close(self):
        if self._h:
            # a model handle holds a pointer to its context: one that outlives it (kept alive by a traceback, say) must not be
            # destroyed afterwards -- gmmiv_gmm_destroy would read the freed context
            for m in list(self._models):
                m.close()
            lib.gmmiv_ctx_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            if sys is None or sys.is_finalizing():   # the HIP runtime may already be gone at interpreter exit
                return
            self.close()
        except Exception:
            pass

    def kernel_ms(self, name):
        return lib.gmmiv_ctx_kernel_ms(self._h, name.encode())

    def kernel_launches(self, name):
        return lib.gmmiv_ctx_kernel_launches(self._h, name.encode())

    def sync(self):
        _chk(lib.gmmiv_ctx_sync(self._h))

    def set_option(self, key, value):
        return lib.gmmiv_ctx_set_option(self._h, key.encode(), ct.c_long(value))

    def trial_piece(self):
        """gmmiv_trial_piece: the frames per work item gmmiv_llr_trials uses on this context ("trials_piece" if set and valid, else TRIAL_PIECE)"""
        return int(lib.gmmiv_trial_piece(self._h))

    def set_hook(self, point, fn):
        """gmmiv_ctx_set_hook: `fn()` is called on the host at `point` ("tv_a_ready": inside tv_estimate_a_and_c once A is
        complete and before the Cmx GEMM is enqueued; "md_factored": inside tv_min_divergence after R is factored, before T is
        read).  fn = None removes the hook.  Exceptions raised by fn are kept and re-raised by the next checked call."""
        if not hasattr(self, "_hooks"):
            self._hooks = {}
        if fn is None:
            self._hooks.pop(point, None)
            rc = lib.gmmiv_ctx_set_hook(self._h, point.encode(), None, None)
        else:
            def tramp(_user, fn=fn):
                try:
                    fn()
                except BaseException as e:      # noqa: BLE001 - a C frame is below us: park it
                    self._hook_error = e
            cb = _HOOK_T(tramp)
            self._hooks[point] = cb             # keep the trampoline alive as long as it is installed
            rc = lib.gmmiv_ctx_set_hook(self._h, point.encode(), ct.cast(cb, ct.c_void_p), None)
        if rc != 0:
            raise GmmivError("unknown hook point %r" % point)

    def _raise_hook_error(self):
        e = getattr(self, "_hook_error", None)
        if e is not None:
            self._hook_error = None
            raise e

    def last_kernel_ms(self):
        name = ct.c_char_p()
        ms = lib.gmmiv_ctx_last_kernel_ms(self._h, ct.byref(name))
        return ms, (name.value.decode() if name.value else "")

    # ---- model
    def gmm(self, w, mean, covinv):
        return Gmm(self, w, mean, covinv)

    # ---- FrameAccGD
    def gmm_batch(self, G, C, D):
        """G models of one (C, D) for the per-segment entry points: .load, .llk, .tv_stats, .map_adapt (GmmBatch)."""
        return GmmBatch(self, G, C, D)

    def frame_moments(self, x, acc=None):
        x, dt, T, ldx = _feat(x)
        D = x.shape[1]
        if acc is None:
            acc = np.zeros(2 * D + 1)
        _chk(lib.gmmiv_frame_moments(self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), D, _ptr(acc)))
        return acc

    def count_unusable_frames(self, x):
        """gmmiv_count_unusable_frames: the frames with a NaN, infinite or absurd (|x| > 1e18) feature value; waits for the stream"""
        x, dt, T, ldx = _feat(x)
        n = ct.c_int64(0)
        _chk(lib.gmmiv_count_unusable_frames(self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), x.shape[1], ct.byref(n)))
        return int(n.value)

    # ---- frame selection on the device (x, out: torch CUDA tensors)
    def gather_frames(self, x, frame_idx, out):
        x, dt, T, ldx = _feat(x)
        idx = frame_idx if _is_torch(frame_idx) else np.ascontiguousarray(frame_idx, np.int64)
        _chk(lib.gmmiv_gather_frames(self._h, _ptr(x), dt, ct.c_int64(ldx), x.shape[1], _ptr(idx), ct.c_int64(idx.shape[0]), _ptr(out)))
        return out

    def gather_runs(self, x, runs, out):
        """runs [nrun, 3] int64 (source frame, output row, length), host or device."""
        x, dt, T, ldx = _feat(x)
        r = runs if _is_torch(runs) else np.ascontiguousarray(runs, np.int64)
        _chk(lib.gmmiv_gather_runs(self._h, _ptr(x), dt, ct.c_int64(ldx), x.shape[1], _ptr(r), ct.c_int64(r.shape[0]), _ptr(out)))
        return out

    def scatter_runs(self, x, runs, inp):
        """The inverse of gather_runs: rows [dst, dst + len) of `inp` (compact, device) go back to frames [src, src + len) of the device
        frame matrix x; runs [nrun, 3] int64 (frame, row, length), host or device."""
        x, dt, T, ldx = _feat(x)
        r = runs if _is_torch(runs) else np.ascontiguousarray(runs, np.int64)
        _chk(lib.gmmiv_scatter_runs(self._h, _ptr(x), dt, ct.c_int64(ldx), x.shape[1], _ptr(r), ct.c_int64(r.shape[0]), _ptr(inp)))
        return x

    # ---- NormFeat's default mode and NormFeatWindowMode's online mode (x, out: torch device frame matrices, column slices allowed)
    @staticmethod
    def _tab(a):
        return a if a is None or _is_torch(a) else np.ascontiguousarray(a, np.int64)

    def frame_moments_groups(self, x, runs, ngroups, acc=None):
        """acc[g] += (sum x, sum x^2, n) over the runs of group g; runs [nrun, 3] int64 (first frame, length, group), group ids
        non-decreasing, host or device; acc [ngroups, 2 D + 1] float64 (numpy, or torch device), accumulated into."""
        x, dt, T, ldx = _feat_view(x)
        D = x.shape[1]
        r = self._tab(runs)
        if acc is None:
            acc = np.zeros((ngroups, 2 * D + 1))
        _chk(lib.gmmiv_frame_moments_groups(self._h, _vptr(x), dt, ct.c_int64(ldx), D, _ptr(r), ct.c_int64(r.shape[0]), ct.c_int64(ngroups), _ptr(acc)))
        return acc

    def frame_moments_stats(self, acc, D, mean=None, std=None):
        """FrameAccGD mean / biased std of every group of acc [ngroups, 2 D + 1] -> (mean, std) [ngroups, D] (of acc's kind)."""
        ngroups = acc.shape[0]
        if mean is None or std is None:
            if _is_torch(acc):
                import torch
                mean, std = torch.empty((ngroups, D), dtype=torch.float64, device=acc.device), torch.empty((ngroups, D), dtype=torch.float64, device=acc.device)
            else:
                mean, std = np.empty((ngroups, D)), np.empty((ngroups, D))
        a = acc if _is_torch(acc) else np.ascontiguousarray(acc, np.float64)
        _chk(lib.gmmiv_frame_moments_stats(self._h, ct.c_int64(ngroups), D, _ptr(a), _ptr(mean), _ptr(std)))
        return mean, std

    def feat_norm_apply(self, x, runs, mean, std, out=None, out_dtype=None, ngroups=None):
        """out = (x - mean[g]) / std[g] on the frames of the runs (computeZeroOne); mean / std [ngroups, D] float64 or None (no subtraction
        / no division); out=None allocates a matrix of out_dtype (default: x's; rows outside the runs are left unset), out=x is in place."""
        x, dt, T, ldx = _feat_view(x)
        D = x.shape[1]
        if out is None:
            out = _feat_like(x, dt if out_dtype is None else out_dtype)
        out, odt, To, ldo = _feat_view(out)
        assert out.shape[1] == D
        r = self._tab(runs)
        m = mean if mean is None or _is_torch(mean) else np.ascontiguousarray(mean, np.float64)
        s = std if std is None or _is_torch(std) else np.ascontiguousarray(std, np.float64)
        if ngroups is None:
            assert m is not None or s is not None, "feat_norm_apply: ngroups is needed when mean and std are both None"
            ngroups = (m if m is not None else s).shape[0]
        _chk(lib.gmmiv_feat_norm_apply(self._h, _vptr(x), dt, ct.c_int64(ldx), D, _ptr(r), ct.c_int64(r.shape[0]), ct.c_int64(ngroups), _ptr(m), _ptr(s),
                                       _vptr(out), odt, ct.c_int64(ldo)))
        return out

    def feat_norm_online(self, x, file_begin, window=300, look_ahead=0, out=None, out_dtype=None):
        """normFeatOnlineMode per file [file_begin[f], file_begin[f + 1]): running mean / std with the forgetting factor (W - 1) / W,
        initialised from W - L zeros and the first L = min(look_ahead, window) frames.  file_begin: nfiles + 1 int64, host or device."""
        x, dt, T, ldx = _feat_view(x)
        if out is None:
            out = _feat_like(x, dt if out_dtype is None else out_dtype)
        out, odt, To, ldo = _feat_view(out)
        assert out.shape[1] == x.shape[1]
        fb = self._tab(file_begin)
        _chk(lib.gmmiv_feat_norm_online(self._h, _vptr(x), dt, ct.c_int64(ldx), x.shape[1], _ptr(fb), ct.c_int64(fb.shape[0] - 1), ct.c_int64(window),
                                        ct.c_int64(look_ahead), _vptr(out), odt, ct.c_int64(ldo)))
        return out

    # ---- NormFeat's windowMode (include/gmmiv_feat_window.h): the steps of plan_norm_windows, every file's chain in one launch
    def feat_norm_window(self, x, runs, nfiles, step_off, steps, alpha, cms_only=False, var_only=False, gstat=None, step_stat=None, stats=True):
        """gmmiv_feat_norm_window, in place on x (a torch device frame matrix, column slices allowed): runs [nrun, 3] int64 (first frame,
        length, file), step_off [nfiles + 1], steps [nsteps, 4], alpha [nsteps] as plan_norm_windows returns them, host or device.
        -> (gstat [nfiles, 2 D] = gm | gs, step_stat [nsteps, 2 D] = m' | s'): numpy unless torch device arrays are passed (with device
        tables the call then only enqueues); stats=False passes NULL for both and returns (None, None)."""
        x, dt, T, ldx = _feat_view(x)
        D = x.shape[1]
        r, so, st = self._tab(runs), self._tab(step_off), self._tab(steps)
        al = alpha if alpha is None or _is_torch(alpha) else np.ascontiguousarray(alpha, np.float64)
        nrun = 0 if r is None else r.shape[0]
        nsteps = 0 if al is None else al.shape[0]
        if stats and gstat is None:
            gstat = np.zeros((nfiles, 2 * D))
        if stats and step_stat is None:
            step_stat = np.zeros((nsteps, 2 * D))
        flags = (NORMWIN_CMS if cms_only else 0) | (NORMWIN_VAR if var_only else 0)
        _chk(lib.gmmiv_feat_norm_window(self._h, _vptr(x), dt, ct.c_int64(ldx), D, _ptr(r), ct.c_int64(nrun), ct.c_int64(nfiles), _ptr(so), _ptr(st), _ptr(al),
                                        ct.c_int64(nsteps), flags, _ptr(gstat), _ptr(step_stat)))
        return gstat, step_stat

    # ---- TurnDetection (include/gmmiv_turn.h): the criterion curve, the decisions and the output segments of a list of files
    def turn_curve(self, x, runs, nfiles, pos_off, win_size=50, win_step=5, crit="DGLR", min_llk=-200.0, max_llk=200.0, value=None, status=None, npos=None):
        """gmmiv_turn_curve on x (a torch device frame matrix, column slices allowed): runs [nrun, 3] int64 (first frame, length, file) and
        pos_off [nrun + 1] as plan_turn_positions returns it, host or device (npos is then needed) -> (value [npos], status [npos] int32):
        numpy unless torch device arrays are passed (with device tables the call then only enqueues)."""
        x, dt, T, ldx = _feat_view(x)
        D = x.shape[1]
        r, po = self._tab(runs), self._tab(pos_off)
        nrun = 0 if r is None else r.shape[0]
        if npos is None:
            npos = int(po[-1])
        if value is None:
            value = np.zeros(npos)
        if status is None:
            status = np.zeros(npos, np.int32)
        _chk(lib.gmmiv_turn_curve(self._h, _vptr(x), dt, ct.c_int64(ldx), D, _ptr(r), ct.c_int64(nrun), ct.c_int64(nfiles), _ptr(po), ct.c_int64(npos),
                                  ct.c_int64(win_size), ct.c_int64(win_step), turn_crit(crit), ct.c_double(min_llk), ct.c_double(max_llk), _ptr(value), _ptr(status)))
        return value, status

    def turn_pick(self, value, pos_off, alpha=0.7, smoothed=None, dec=None, run_stats=None, n_turns=None, npos=None, smooth=True):
        """gmmiv_turn_pick on a curve (numpy or torch device) -> (smoothed [npos], dec [npos] uint8, run_stats [nrun, 2] = mean | std,
        n_turns [nrun]); outputs numpy unless torch device arrays are passed.  smooth=False passes NULL for smoothed (the library keeps the
        smoothed curve in its workspace) and returns None in its place."""
        po = self._tab(pos_off)
        nrun = po.shape[0] - 1
        v = value if _is_torch(value) else np.ascontiguousarray(value, np.float64)
        if npos is None:
            npos = int(v.shape[0])
        if smoothed is None and smooth:
            smoothed = np.zeros(npos)
        if dec is None:
            dec = np.zeros(npos, np.uint8)
        if run_stats is None:
            run_stats = np.zeros((nrun, 2))
        if n_turns is None:
            n_turns = np.zeros(nrun, np.int64)
        _chk(lib.gmmiv_turn_pick(self._h, _ptr(v), _ptr(po), ct.c_int64(nrun), ct.c_int64(npos), ct.c_double(alpha), _ptr(smoothed), _ptr(dec), _ptr(run_stats),
                                 _ptr(n_turns)))
        return smoothed, dec, run_stats, n_turns

    def turn_segments(self, runs, nfiles, pos_off, dec, win_size=50, win_step=5, seg_off=None, seg_begin=None, seg_len=None, seg_count=None, npos=None):
        """gmmiv_turn_segments.  seg_begin is None: the counting call -> seg_count [nfiles]; with seg_off [nfiles + 1], seg_begin, seg_len:
        the fill call -> (seg_count, seg_begin, seg_len).  Arrays numpy or torch device."""
        r, po, so = self._tab(runs), self._tab(pos_off), self._tab(seg_off)
        nrun = 0 if r is None else r.shape[0]
        d = dec if _is_torch(dec) else np.ascontiguousarray(dec, np.uint8)
        if npos is None:
            npos = int(d.shape[0])
        if seg_count is None:
            seg_count = np.zeros(nfiles, np.int64)
        _chk(lib.gmmiv_turn_segments(self._h, _ptr(r), ct.c_int64(nrun), ct.c_int64(nfiles), _ptr(po), ct.c_int64(npos), _ptr(d), ct.c_int64(win_size),
                                     ct.c_int64(win_step), _ptr(seg_count), _ptr(so), _ptr(seg_begin), _ptr(seg_len)))
        return seg_count if seg_begin is None else (seg_count, seg_begin, seg_len)

    def turn_detect(self, x, runs, nfiles, win_size=50, win_step=5, alpha=0.7, crit="DGLR", min_llk=-200.0, max_llk=200.0):
        """plan + curve + pick + count + fill with host tables and outputs -> dict(pos_off, value, status, smoothed, dec, run_stats, n_turns,
        seg_off [nfiles + 1], seg_begin, seg_len)"""
        r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
        po = plan_turn_positions(r, nfiles, win_size, win_step)
        value, status = self.turn_curve(x, r, nfiles, po, win_size, win_step, crit, min_llk, max_llk)
        sm, dec, rs, nt = self.turn_pick(value, po, alpha)
        cnt = self.turn_segments(r, nfiles, po, dec, win_size, win_step)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        sb, sl = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.int64)
        if off[-1] > 0:
            self.turn_segments(r, nfiles, po, dec, win_size, win_step, seg_off=off, seg_begin=sb, seg_len=sl)
        return dict(pos_off=po, value=value, status=status, smoothed=sm, dec=dec, run_stats=rs, n_turns=nt, seg_off=off, seg_begin=sb, seg_len=sl)

    # ---- EnergyDetector on resident frames: x is the ENERGY COLUMN, a torch device view [T, 1] (x[:, 16:17] of a wider matrix keeps its stride)
    def energy_train(self, x, runs, nfiles, C=3, nb_train_it=10, variance_flooring=0.5, variance_ceiling=10.0, alpha=0.0, model=None, threshold=None,
                     status=None):
        """gmmiv_energy_train: runs [nrun, 3] int64 (first frame, length, file), host or device -> (model [nfiles, 3 C] = w | mean | cov,
        threshold [nfiles], status [nfiles] int32); outputs numpy unless torch device arrays are passed (then the call only enqueues)."""
        x, dt, T, ldx = _feat_view(x)
        assert x.shape[1] == 1, "energy_train: x is one column"
        r = self._tab(runs)
        if model is None:
            model = np.zeros((nfiles, 3 * C))
        if threshold is None:
            threshold = np.zeros(nfiles)
        if status is None:
            status = np.zeros(nfiles, np.int32)
        _chk(lib.gmmiv_energy_train(self._h, _vptr(x), dt, ct.c_int64(ldx), _ptr(r), ct.c_int64(0 if r is None else r.shape[0]), ct.c_int64(nfiles), int(C),
                                    int(nb_train_it), ct.c_double(variance_flooring), ct.c_double(variance_ceiling), ct.c_double(alpha), _ptr(model),
                                    _ptr(threshold), _ptr(status)))
        return model, threshold, status

    def energy_select(self, x, runs, nfiles, threshold, seg_off=None, seg_begin=None, seg_len=None, n_above=None, seg_count=None):
        """gmmiv_energy_select.  seg_begin is None: the counting call -> (n_above [nfiles], seg_count [nfiles]); with seg_off [nfiles + 1],
        seg_begin, seg_len: the fill call -> (n_above, seg_count, seg_begin, seg_len).  Arrays numpy or torch device."""
        x, dt, T, ldx = _feat_view(x)
        assert x.shape[1] == 1, "energy_select: x is one column"
        r = self._tab(runs)
        th = threshold if _is_torch(threshold) else np.ascontiguousarray(threshold, np.float64)
        if n_above is None:
            n_above = np.zeros(nfiles, np.int64)
        if seg_count is None:
            seg_count = np.zeros(nfiles, np.int64)
        so = self._tab(seg_off)
        _chk(lib.gmmiv_energy_select(self._h, _vptr(x), dt, ct.c_int64(ldx), _ptr(r), ct.c_int64(0 if r is None else r.shape[0]), ct.c_int64(nfiles), _ptr(th),
                                     _ptr(n_above), _ptr(seg_count), _ptr(so), _ptr(seg_begin), _ptr(seg_len)))
        return (n_above, seg_count) if seg_begin is None else (n_above, seg_count, seg_begin, seg_len)

    def energy_detect(self, x, runs, nfiles, **kw):
        """train + count + fill with host outputs -> dict(model, threshold, status, n_above, seg_off [nfiles + 1], seg_begin, seg_len)"""
        model, th, st = self.energy_train(x, runs, nfiles, **kw)
        above, cnt = self.energy_select(x, runs, nfiles, th)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
        sb, sl = np.zeros(int(off[-1]), np.int64), np.zeros(int(off[-1]), np.int64)
        if off[-1] > 0:
            self.energy_select(x, runs, nfiles, th, seg_off=off, seg_begin=sb, seg_len=sl)
        return dict(model=model, threshold=th, status=st, n_above=above, seg_off=off, seg_begin=sb, seg_len=sl)

    def segment_means(self, v, seg_begin, out=None):
        """v: torch CUDA float64 [nrows, ld] (or 1-D); seg_begin: nseg + 1 host offsets -> out [nrows, nseg]."""
        v2 = v if v.dim() == 2 else v.reshape(1, -1)
        sb = np.ascontiguousarray(seg_begin, np.int64)
        if out is None:
            out = np.empty((v2.shape[0], len(sb) - 1))
        _chk(lib.gmmiv_segment_means(self._h, _ptr(v2), ct.c_int64(v2.stride(0)), v2.shape[0], _ptr(sb), ct.c_int64(len(sb) - 1), _ptr(out)))
        return out

    def variance_control(self, cov, flooring, ceiling, cov_signal, C, D, count=True):
        counts = np.zeros(2, np.int64) if count else None
        _chk(lib.gmmiv_variance_control(self._h, C, D, _ptr(cov), ct.c_double(flooring), ct.c_double(ceiling),
                                        _ptr(_f64(cov_signal)), _ptr(counts)))
        return cov, counts

    # ---- TVAcc maths
    def tv_subtract_m(self, N, F, means, C, D):
        U = N.shape[0]
        _chk(lib.gmmiv_tv_subtract_m(self._h, ct.c_int64(U), C, D, _ptr(N), _ptr(F), _ptr(means)))
        return F

    def tv_subtract_m_to(self, N, F_src, F_dst, means, C, D):
        """F_dst = F_src - N means (restoreStats + substractM in one pass); F_dst may be F_src."""
        _chk(lib.gmmiv_tv_subtract_m_to(self._h, ct.c_int64(N.shape[0]), C, D, _ptr(N), _ptr(F_src), _ptr(F_dst), _ptr(means)))
        return F_dst

    def tv_tett(self, Tm, invvar, C, D, out=None):
        R = Tm.shape[0]
        if out is None:
            out = np.empty((C, lib.gmmiv_tv_packed_len(R)))
        _chk(lib.gmmiv_tv_tett(self._h, C, D, R, _ptr(Tm), _ptr(invvar), _ptr(out)))
        return out

    def tv_estimate_w(self, N, F, Tm, invvar, tett, C, D, out=None):
        U, R = N.shape[0], Tm.shape[0]
        if out is None:
            out = np.empty((U, R))
        _chk(lib.gmmiv_tv_estimate_w(self._h, ct.c_int64(U), C, D, R, _ptr(N), _ptr(F), _ptr(Tm), _ptr(invvar),
                                     _ptr(tett), _ptr(out)))
        return out

    # ---- approximate extractors (IvExtractor modes ubmWeight / eigenDecomposition); in-place on numpy / torch arrays
    def tv_norm_statistics(self, N, F, means, invvar, C, D):
        _chk(lib.gmmiv_tv_norm_statistics(self._h, ct.c_int64(N.shape[0]), C, D, _ptr(N), _ptr(F), _ptr(means), _ptr(invvar)))
        return F

    def tv_subtract_m_plus_tw(self, N, F, means, Tm, W, C, D):
        _chk(lib.gmmiv_tv_subtract_m_plus_tw(self._h, ct.c_int64(N.shape[0]), C, D, Tm.shape[0], _ptr(N), _ptr(F), _ptr(means),
                                             _ptr(Tm), _ptr(W)))
        return F

    # ---- JFA (gmmiv_jfa_*; the factor steps are tv_tett / tv_estimate_a_and_c / tv_estimate_w / tv_update_t) ----
    def jfa_subtract(self, N, F, C, D, owner=None, nfact=None, means=None, T=None, W=None, Dm=None, Z=None):
        rows = N.shape[0]
        if nfact is None:
            nfact = W.shape[0] if W is not None else (Z.shape[0] if Z is not None else rows)
        o = None if owner is None else (owner if _is_torch(owner) else np.ascontiguousarray(owner, np.int64))
        _chk(lib.gmmiv_jfa_subtract(self._h, ct.c_int64(rows), C, D, _ptr(N), _ptr(F), _ptr(o), ct.c_int64(nfact), _ptr(means),
                                    0 if T is None else T.shape[0], _ptr(T), _ptr(W), _ptr(Dm), _ptr(Z)))
        return F

    def jfa_subtract_sessions(self, sess_begin, N_h, F_X, U, X, C, D):
        sb = np.ascontiguousarray(sess_begin, np.int64)
        _chk(lib.gmmiv_jfa_subtract_sessions(self._h, ct.c_int64(len(sb) - 1), _ptr(sb), C, D, _ptr(N_h), _ptr(F_X), U.shape[0], _ptr(U), _ptr(X)))
        return F_X

    def jfa_estimate_z(self, N, F, invvar, Dm, C, D, tau=-1.0, out=None):
        if out is None:
            out = np.empty((N.shape[0], C * D))
        _chk(lib.gmmiv_jfa_estimate_z(self._h, ct.c_int64(N.shape[0]), C, D, _ptr(N), _ptr(F), _ptr(invvar), _ptr(Dm), ct.c_double(tau), _ptr(out)))
        return out

    def jfa_estimate_z_and_d(self, N, F, invvar, Dm, C, D, out=None):
        """Dm is updated in place; returns Z."""
        if out is None:
            out = np.empty((N.shape[0], C * D))
        _chk(lib.gmmiv_jfa_estimate_z_and_d(self._h, ct.c_int64(N.shape[0]), C, D, _ptr(N), _ptr(F), _ptr(invvar), _ptr(Dm), _ptr(out)))
        return out

    def tv_norm_t(self, Tm, invvar, C, D):
        _chk(lib.gmmiv_tv_norm_t(self._h, C, D, Tm.shape[0], _ptr(Tm), _ptr(invvar)))
        return Tm

    def tv_weighted_cov(self, Tm, weight, C, D, out=None):
        R = Tm.shape[0]
        if out is None:
            out = np.empty((R, R))
        _chk(lib.gmmiv_tv_weighted_cov(self._h, C, D, R, _ptr(Tm), _ptr(weight), _ptr(out)))
        return out

    def tv_approximate_tctc(self, Tm, Q, C, D, out=None):
        R = Tm.shape[0]
        if out is None:
            out = np.zeros((C, R))
        _chk(lib.gmmiv_tv_approximate_tctc(self._h, C, D, R, _ptr(Tm), _ptr(Q), _ptr(out)))
        return out

    def tv_estimate_w_ubm_weight(self, N, F, Tm, Wm, C, D, out=None):
        U, R = N.shape[0], Tm.shape[0]
        if out is None:
            out = np.zeros((U, R))
        _chk(lib.gmmiv_tv_estimate_w_ubm_weight(self._h, ct.c_int64(U), C, D, R, _ptr(N), _ptr(F), _ptr(Tm), _ptr(Wm), _ptr(out)))
        return out

    def tv_estimate_w_eigen(self, N, F, Tm, Dm, Q, C, D, out=None):
        U, R = N.shape[0], Tm.shape[0]
        if out is None:
            out = np.zeros((U, R))
        _chk(lib.gmmiv_tv_estimate_w_eigen(self._h, ct.c_int64(U), C, D, R, _ptr(N), _ptr(F), _ptr(Tm), _ptr(Dm), _ptr(Q), _ptr(out)))
        return out

    # ---- PldaDev: back-end estimation on a development set X[dim, n], sessions grouped by speaker
    def _dev_args(self, X, sps):
        sps = np.ascontiguousarray(sps, dtype=np.int64)
        return X.shape[0], ct.c_int64(X.shape[1]), _ptr(X), ct.c_int64(len(sps)), sps.ctypes.data_as(ct.c_void_p), sps

    def dev_means(self, X, sps):
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        mean = np.empty(dim); sm = np.empty((dim, len(keep)))
        _chk(lib.gmmiv_dev_means(self._h, dim, n, xp, k, sp, _ptr(mean), _ptr(sm)))
        return mean, sm

    def dev_cov_mat(self, X, sps):
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        S = np.empty((dim, dim)); W = np.empty((dim, dim)); B = np.empty((dim, dim))
        _chk(lib.gmmiv_dev_cov_mat(self._h, dim, n, xp, k, sp, _ptr(S), _ptr(W), _ptr(B)))
        return S, W, B

    def dev_wccn_chol(self, X, sps, out=None):
        """out (here and in the estimation calls below): a numpy array or a device tensor of the result's shape, written in place"""
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        if out is None:
            out = np.empty((dim, dim))
        _chk(lib.gmmiv_dev_wccn_chol(self._h, dim, n, xp, k, sp, _ptr(out)))
        return out

    def dev_mahalanobis(self, X, sps, out=None):
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        if out is None:
            out = np.empty((dim, dim))
        _chk(lib.gmmiv_dev_mahalanobis(self._h, dim, n, xp, k, sp, _ptr(out)))
        return out

    def dev_scatter_mat(self, X, sps):
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        SB = np.empty((dim, dim)); SW = np.empty((dim, dim))
        _chk(lib.gmmiv_dev_scatter_mat(self._h, dim, n, xp, k, sp, _ptr(SB), _ptr(SW)))
        return SB, SW

    def sym_eigen(self, A, rank=None, out=None):
        """out: (vect [n x rank], val [rank])"""
        n = A.shape[0]; rank = n if rank is None else rank
        vect, val = (np.empty((n, rank)), np.empty(rank)) if out is None else out
        _chk(lib.gmmiv_sym_eigen(self._h, n, _ptr(_f64(A)), rank, _ptr(vect), _ptr(val)))
        return vect, val

    def dev_efr_matrix(self, Cov, out=None):
        if out is None:
            out = np.empty((Cov.shape[0], Cov.shape[0]))
        _chk(lib.gmmiv_dev_efr_matrix(self._h, Cov.shape[0], _ptr(_f64(Cov)), _ptr(out)))
        return out

    def dev_lda(self, W, B, rank, out=None):
        """out: (ldaMat [rank x dim], eigval [rank])"""
        dim = W.shape[0]
        out, val = (np.empty((rank, dim)), np.empty(rank)) if out is None else out
        _chk(lib.gmmiv_dev_lda(self._h, dim, _ptr(_f64(W)), _ptr(_f64(B)), rank, _ptr(out), _ptr(val)))
        return out, val

    def plda_em_iteration(self, X, sps, F, G, Sigma, Delta):
        """One PldaModel::em_iteration, in place on X (centred by Delta), F, G, Sigma, Delta: float64 numpy arrays or device
        tensors, each on its own (the five ARE the outputs: there is no out=)."""
        dim, n, xp, k, sp, keep = self._dev_args(X, sps)
        _chk(lib.gmmiv_plda_em_iteration(self._h, dim, n, xp, k, sp, F.shape[1], G.shape[1], _ptr(F), _ptr(G), _ptr(Sigma), _ptr(Delta)))
        return X, F, G, Sigma, Delta

    def twocov_model(self, W, B, out=None):
        """out: (G, H)"""
        dim = W.shape[0]
        G, H = (np.empty((dim, dim)), np.empty((dim, dim))) if out is None else out
        _chk(lib.gmmiv_twocov_model(self._h, dim, _ptr(_f64(W)), _ptr(_f64(B)), _ptr(G), _ptr(H)))
        return G, H

    def plda_precompute(self, F, G, Sigma, out=None):
        """-> (FTJ [rf x dim], FTJF [rf x rf]); G may be None; out: (FTJ, FTJF)."""
        dim, rf = F.shape
        rg = 0 if G is None else G.shape[1]
        FTJ, FTJF = (np.empty((rf, dim)), np.empty((rf, rf))) if out is None else out
        _chk(lib.gmmiv_plda_precompute(self._h, dim, rf, rg, _ptr(_f64(F)), _ptr(_f64(G)), _ptr(_f64(Sigma)), _ptr(FTJ), _ptr(FTJF)))
        return FTJ, FTJF

    def tv_estimate_a_and_c(self, N, F, Tm, invvar, tett, C, D, acc=None):
        U, R = N.shape[0], Tm.shape[0]
        P = lib.gmmiv_tv_packed_len(R)
        if acc is None:
            acc = dict(A=np.zeros((C, P)), Cmx=np.zeros((R, C * D)), Rm=np.zeros((R, R)), r=np.zeros(R),
                       meanW=np.zeros(R))
        W = acc.get("W")
        if W is None or W.shape[0] != U:
            W = np.empty((U, R))
        self._hook_error = None
        rc = lib.gmmiv_tv_estimate_a_and_c(self._h, ct.c_int64(U), C, D, R, _ptr(N), _ptr(F), _ptr(Tm), _ptr(invvar),
                                           _ptr(tett), _ptr(W), _ptr(acc["A"]), _ptr(acc["Cmx"]), _ptr(acc["Rm"]),
                                           _ptr(acc["r"]), _ptr(acc["meanW"]))
        self._raise_hook_error()        # an exception parked by the hook comes first: it is the cause, and it never outlives this call
        _chk(rc)
        acc["W"] = W
        return acc

    def tv_update_t(self, A_packed, Cmx, C, D, out=None):
        R = Cmx.shape[0]
        if out is None:
            out = np.empty((R, C * D))
        _chk(lib.gmmiv_tv_update_t(self._h, C, D, R, _ptr(A_packed), _ptr(Cmx), _ptr(out)))
        return out

    def tv_min_divergence(self, Rm, r, meanW, means, Tm, n_sessions, C, D):
        R = Tm.shape[0]
        self._hook_error = None
        rc = lib.gmmiv_tv_min_divergence(self._h, C, D, R, ct.c_double(n_sessions), _ptr(Rm), _ptr(r), _ptr(meanW),
                                         _ptr(means), _ptr(Tm))
        self._raise_hook_error()
        _chk(rc)
        return means, Tm

    def tv_orthonormalize_t(self, Tm):
        """in place on Tm [R x SV], a numpy array or a device tensor (Tm IS the output: there is no out=)"""
        R, SV = Tm.shape
        _chk(lib.gmmiv_tv_orthonormalize_t(self._h, R, ct.c_int64(SV), _ptr(Tm)))
        return Tm

    def iv_normalize(self, X, mean=None, M=None, length_norm=True, out=None):
        dim_in, n = X.shape
        dim_out = M.shape[0] if M is not None else dim_in
        if out is None:
            out = np.empty((dim_out, n))
        _chk(lib.gmmiv_iv_normalize(self._h, dim_in, dim_out, ct.c_int64(n), _ptr(X), _ptr(_f64(mean)), _ptr(_f64(M)),
                                    int(bool(length_norm)), _ptr(out)))
        return out

    # ---- scoring (vectors as columns: models[dim, M], segs[dim, S])
    def _score_out(self, models, segs, out):
        M, S = models.shape[1], segs.shape[1]
        if out is None:
            out = np.empty((M, S))
        return M, S, out

    def score_cosine(self, models, segs, out=None):
        M, S, out = self._score_out(models, segs, out)
        _chk(lib.gmmiv_score_cosine(self._h, models.shape[0], ct.c_int64(M), ct.c_int64(S), _ptr(models), _ptr(segs),
                                    _ptr(out)))
        return out

    def score_mahalanobis(self, models, segs, Mah, out=None):
        M, S, out = self._score_out(models, segs, out)
        _chk(lib.gmmiv_score_mahalanobis(self._h, models.shape[0], ct.c_int64(M), ct.c_int64(S), _ptr(models),
                                         _ptr(segs), _ptr(Mah), _ptr(out)))
        return out

    def score_twocov(self, models, segs, G, H, out=None):
        M, S, out = self._score_out(models, segs, out)
        _chk(lib.gmmiv_score_twocov(self._h, models.shape[0], ct.c_int64(M), ct.c_int64(S), _ptr(models), _ptr(segs),
                                    _ptr(G), _ptr(H), _ptr(out)))
        return out

    def score_twocov_mix_part(self, models, segs, G, scores):
        """scores += (m + s)^T G (m + s) (PldaTest::twoCovScoringMixPart); scores is updated in place."""
        M, S = models.shape[1], segs.shape[1]
        _chk(lib.gmmiv_score_twocov_mix_part(self._h, models.shape[0], ct.c_int64(M), ct.c_int64(S), _ptr(models), _ptr(segs), _ptr(G),
                                             _ptr(scores)))
        return scores

    def score_apply_trials(self, trials, scores, fill=0.0):
        """scores[m, s] = fill where trials[m, s] == 0 (PldaTest::_trials); in place."""
        M, S = scores.shape
        t = trials if _is_torch(trials) else np.ascontiguousarray(trials, np.uint8)
        _chk(lib.gmmiv_score_apply_trials(self._h, ct.c_int64(M), ct.c_int64(S), _ptr(t), ct.c_double(fill), _ptr(scores)))
        return scores

    # ---- the fp64 GEMM under all of the above, as the library calls it
    def dgemm(self, ta, tb, alpha, A, B, beta, C, nz=1, epi_mode=0, rv=None, cv=None, br=0.0, bc=0.0, cst=0.0, K=None):
        """C = epilogue(alpha op(A) op(B)) + beta C, in place (gmmiv_dgemm).  A, B, C: 2-D, or 3-D with the batch first,
        torch.float64 CUDA tensors whose last stride is 1.  The leading dimensions and batch strides are the tensors' strides
        (a batch stride of 0 -- an expanded operand -- is a shared matrix) and data_ptr() is passed as it is, so a view that
        starts inside a larger buffer keeps its offset.  K is read from A; pass it when M == 0 leaves it open."""
        import torch
        for t in (A, B, C):
            assert _is_torch(t) and t.is_cuda and t.dtype == torch.float64 and t.dim() in (2, 3) and t.stride(-1) == 1
        batch = C.shape[0] if C.dim() == 3 else 1
        assert all(t.dim() == 2 or t.shape[0] == batch for t in (A, B))

        def ld(t):      # a single row has no stride of its own
            return t.stride(-2) if t.shape[-2] > 1 else max(t.stride(-2), t.shape[-1], 1)

        def bs(t):
            return t.stride(0) if t.dim() == 3 and batch > 1 else 0
        M, N = C.shape[-2], C.shape[-1]
        if K is None:
            K = A.shape[-2] if ta else A.shape[-1]
        assert tuple(A.shape[-2:]) == ((K, M) if ta else (M, K)) and tuple(B.shape[-2:]) == ((N, K) if tb else (K, N))
        for v in (rv, cv):
            assert v is None or (v.is_cuda and v.dtype == torch.float64 and v.is_contiguous())
        _chk(lib.gmmiv_dgemm(self._h, int(bool(ta)), int(bool(tb)), M, N, K, ct.c_double(alpha), _vptr(A), ct.c_int64(ld(A)),
                             ct.c_int64(bs(A)), _vptr(B), ct.c_int64(ld(B)), ct.c_int64(bs(B)), ct.c_double(beta), _vptr(C),
                             ct.c_int64(ld(C)), ct.c_int64(bs(C)), batch, int(nz), int(epi_mode), _ptr(rv), _ptr(cv),
                             ct.c_double(br), ct.c_double(bc), ct.c_double(cst)))
        return C

    def score_plda(self, models_sum, nsess, segs, FTJF, out=None):
        M, S, out = self._score_out(models_sum, segs, out)
        ns = np.ascontiguousarray(nsess, dtype=np.int64)
        _chk(lib.gmmiv_score_plda(self._h, models_sum.shape[0], ct.c_int64(M), ct.c_int64(S), _ptr(models_sum),
                                  ns.ctypes.data_as(ct.c_void_p), _ptr(segs), _ptr(FTJF), _ptr(out)))
        return out

    # ---- the scoring rules on a LIST of (model, segment) trials (include/gmmiv_iv_trials.h)
    def iv_trial_piece(self):
        """gmmiv_iv_trial_piece: the trials per work item the list rules use on this context"""
        return int(lib.gmmiv_iv_trial_piece(self._h))

    @staticmethod
    def _trial_args(trial_model, trial_seg, out):
        # a device tensor is passed on as it is: the library refuses it with a message
        tm = trial_model if _is_torch(trial_model) else np.ascontiguousarray(trial_model, dtype=np.int32)
        ts = trial_seg if _is_torch(trial_seg) else np.ascontiguousarray(trial_seg, dtype=np.int32)
        assert len(tm) == len(ts)
        if out is None:
            out = np.empty(len(tm))
        return tm, ts, out

    def score_cosine_trials(self, models, segs, trial_model, trial_seg, out=None):
        """the cosine score of every listed trial (trial_model[i], trial_seg[i]), in list order; out: numpy or a device tensor [ntrial]"""
        tm, ts, out = self._trial_args(trial_model, trial_seg, out)
        _chk(lib.gmmiv_score_cosine_trials(self._h, models.shape[0], ct.c_int64(models.shape[1]), ct.c_int64(segs.shape[1]), _ptr(models),
                                           _ptr(segs), _ptr(tm), _ptr(ts), ct.c_int64(len(tm)), _ptr(out)))
        return out

    def score_mahalanobis_trials(self, models, segs, Mah, trial_model, trial_seg, out=None):
        tm, ts, out = self._trial_args(trial_model, trial_seg, out)
        _chk(lib.gmmiv_score_mahalanobis_trials(self._h, models.shape[0], ct.c_int64(models.shape[1]), ct.c_int64(segs.shape[1]),
                                                _ptr(models), _ptr(segs), _ptr(Mah), _ptr(tm), _ptr(ts), ct.c_int64(len(tm)), _ptr(out)))
        return out

    def score_twocov_trials(self, models, segs, G, H, trial_model, trial_seg, out=None):
        tm, ts, out = self._trial_args(trial_model, trial_seg, out)
        _chk(lib.gmmiv_score_twocov_trials(self._h, models.shape[0], ct.c_int64(models.shape[1]), ct.c_int64(segs.shape[1]), _ptr(models),
                                           _ptr(segs), _ptr(G), _ptr(H), _ptr(tm), _ptr(ts), ct.c_int64(len(tm)), _ptr(out)))
        return out

    def score_plda_trials(self, models_sum, nsess, segs, FTJF, trial_model, trial_seg, out=None):
        tm, ts, out = self._trial_args(trial_model, trial_seg, out)
        ns = np.ascontiguousarray(nsess, dtype=np.int64)
        _chk(lib.gmmiv_score_plda_trials(self._h, models_sum.shape[0], ct.c_int64(models_sum.shape[1]), ct.c_int64(segs.shape[1]),
                                         _ptr(models_sum), ns.ctypes.data_as(ct.c_void_p), _ptr(segs), _ptr(FTJF), _ptr(tm), _ptr(ts),
                                         ct.c_int64(len(tm)), _ptr(out)))
        return out

    # ---- score normalisation (LIA_SpkDet/ComputeNorm): cohort statistics + the (x - mean) / std passes
    def score_cohort_stats(self, scores, axis, select=None, pre_mean=None, pre_std=None, mean_mode=0, percent_h=0.0,
                           percent_l=0.0, out_mean=None, out_std=None):
        """mean, std of every row (axis 0) or column (axis 1) of scores[rows, cols] the way DistribNorm::computeMeanStd
        computes them.  scores may be a row-strided view (stride(1) == 1).  select: bytes along the cohort axis."""
        rows, cols = scores.shape
        if _is_torch(scores):
            assert scores.dim() == 2 and (cols <= 1 or scores.stride(1) == 1)
            ld = scores.stride(0) if rows > 1 else cols
        else:
            scores = np.ascontiguousarray(scores, dtype=np.float64)
            ld = cols
        nd = rows if axis == 0 else cols
        if out_mean is None:
            out_mean = np.empty(nd)
        if out_std is None:
            out_std = np.empty(nd)
        sel = select if select is None or _is_torch(select) else np.ascontiguousarray(select, np.uint8)
        _chk(lib.gmmiv_score_cohort_stats(self._h, ct.c_int64(rows), ct.c_int64(cols), ct.c_void_p(_data_ptr(scores)),
                                          ct.c_int64(max(ld, cols)), int(axis), _ptr(sel), _ptr(_f64(pre_mean)),
                                          _ptr(_f64(pre_std)), int(mean_mode), ct.c_double(percent_h), ct.c_double(percent_l),
                                          _ptr(out_mean), _ptr(out_std)))
        return out_mean, out_std

    def score_normalize(self, scores, order, row_mean=None, row_std=None, col_mean=None, col_std=None, first_out=None):
        """scores[M, S] in place; order NORM_Z / NORM_T / NORM_ZT (t first) / NORM_TZ (z first).  first_out: None, or an
        [M, S] array that receives the score after the first of two normalisations."""
        M, S = scores.shape
        _chk(lib.gmmiv_score_normalize(self._h, ct.c_int64(M), ct.c_int64(S), _ptr(scores), int(order), _ptr(_f64(row_mean)),
                                       _ptr(_f64(row_std)), _ptr(_f64(col_mean)), _ptr(_f64(col_std)), _ptr(first_out)))
        return scores

    # ---- score normalisation on lists: CSR distributions of different lengths, a list of trials
    def score_list_stats(self, off, scores, pos=None, pre_id=None, pre_mean=None, pre_std=None, mean_mode=0, percent_h=0.0,
                         percent_l=0.0, out_mean=None, out_std=None):
        """mean, std of the distributions d = slots [off[d], off[d + 1]) of a score list the way DistribNorm::computeMeanStd computes
        them; slot k holds scores[pos[k]] (scores[k] without pos), pre-normalised by (pre_mean, pre_std)[pre_id[k]] when given.
        off: host int64.  The bits are those of score_cohort_stats(axis 0) on a one-row matrix of the same values."""
        off = np.ascontiguousarray(off, dtype=np.int64)
        nd = len(off) - 1
        scores = _f64(scores)
        pos = pos if pos is None or _is_torch(pos) else np.ascontiguousarray(pos, np.int64)
        pre_id = pre_id if pre_id is None or _is_torch(pre_id) else np.ascontiguousarray(pre_id, np.int32)
        pre_mean, pre_std = _f64(pre_mean), _f64(pre_std)
        if out_mean is None:
            out_mean = np.empty(max(nd, 0))
        if out_std is None:
            out_std = np.empty(max(nd, 0))
        npre = 0 if pre_mean is None else int(pre_mean.shape[0])
        _chk(lib.gmmiv_score_list_stats(self._h, ct.c_int64(nd), _ptr(off), _ptr(pos), _ptr(scores), ct.c_int64(int(scores.shape[0])),
                                        _ptr(pre_id), _ptr(pre_mean), _ptr(pre_std), ct.c_int64(npre), int(mean_mode),
                                        ct.c_double(percent_h), ct.c_double(percent_l), _ptr(out_mean), _ptr(out_std)))
        return out_mean, out_std

    def score_normalize_list(self, scores, order, row_id=None, row_mean=None, row_std=None, col_id=None, col_mean=None, col_std=None,
                             first_out=None):
        """scores[n] in place: (x - row_mean[row_id[i]]) / row_std[row_id[i]] and / or the same with the column vectors, in the order
        NORM_Z / NORM_T / NORM_ZT (t first) / NORM_TZ (z first).  first_out: None, or [n] for the value after the first of two."""
        ids = lambda a: a if a is None or _is_torch(a) else np.ascontiguousarray(a, np.int32)
        row_id, col_id = ids(row_id), ids(col_id)
        row_mean, row_std, col_mean, col_std = _f64(row_mean), _f64(row_std), _f64(col_mean), _f64(col_std)
        cnt = lambda v: 0 if v is None else int(v.shape[0])
        _chk(lib.gmmiv_score_normalize_list(self._h, ct.c_int64(int(scores.shape[0])), _ptr(scores), int(order), _ptr(row_id),
                                            _ptr(row_mean), _ptr(row_std), ct.c_int64(cnt(row_mean)), _ptr(col_id), _ptr(col_mean),
                                            _ptr(col_std), ct.c_int64(cnt(col_mean)), _ptr(first_out)))
        return scores

    def workspace_bytes(self, slot=-1):
        """Bytes held in the score-normalisation scratch slot (slot < 0) or in workspace slot `slot`."""
        return int(lib.gmmiv_ctx_workspace_bytes(self._h, int(slot)))


NORM_Z, NORM_T, NORM_ZT, NORM_TZ = 0, 1, 2, 3


def norm_scratch_bytes(ndist):
    """GMMIV_SCORE_NORM_SCRATCH_BYTES(ndist): the most device scratch the score-normalisation calls take"""
    return 512 * int(ndist) + 64
lib.gmmiv_ctx_workspace_bytes.restype = ct.c_size_t
lib.gmmiv_ctx_workspace_bytes.argtypes = [ct.c_void_p, ct.c_int]


SCORE_LIST_CLASSES = 7     # GMMIV_SCORE_LIST_CLASSES


def list_scratch_bytes(ndist):
    """GMMIV_SCORE_LIST_SCRATCH_BYTES(ndist): the device scratch of score_list_stats"""
    return 12 * int(ndist) + 8


ENERGY_EMPTY, ENERGY_NONFINITE, ENERGY_FLOORED, ENERGY_CEILED, ENERGY_MAX_C = 1, 2, 4, 8, 8   # GMMIV_ENERGY_*


def energy_stage_frames(dtype_code=F32):
    """gmmiv_energy_stage_frames: the longest selection gmmiv_energy_train stages in LDS; one frame more is streamed per iteration"""
    return int(lib.gmmiv_energy_stage_frames(int(dtype_code)))


def plan_norm_windows(runs, nfiles, file_first, window_duration=5.0, window_comp=1.0, frame_length=0.01):
    """gmmiv_plan_norm_windows (pure host): the schedule of NormFeat's windowMode on the run table [nrun, 3] (first frame, length, file);
    file_first [nfiles] = the buffer frame where each file starts -> (step_off [nfiles + 1], steps [nsteps, 4], alpha [nsteps])."""
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    ff = np.ascontiguousarray(file_first, np.int64)
    assert ff.shape[0] == nfiles
    off = np.zeros(nfiles + 1, np.int64)
    steps = np.zeros((max(r.shape[0], 1), 4), np.int64)  # at most one step per run
    alpha = np.zeros(max(r.shape[0], 1))
    n = lib.gmmiv_plan_norm_windows(_ptr(r), ct.c_int64(r.shape[0]), ct.c_int64(nfiles), _ptr(ff), ct.c_double(window_duration), ct.c_double(window_comp),
                                    ct.c_double(frame_length), _ptr(off), _ptr(steps), _ptr(alpha))
    if n < 0:
        raise GmmivError("gmmiv error: %s" % lib.gmmiv_last_error().decode())
    return off, np.ascontiguousarray(steps[:n]), np.ascontiguousarray(alpha[:n])


def turn_crit(name):
    """the GMMIV_TURN_* constant of a clusteringCrit name (or the constant itself); DELTABIC is refused: it is not a closed form of the
    windows' moments (a split of the merged Gaussian and two EM iterations per position)"""
    if isinstance(name, str):
        if name == "DELTABIC":
            raise GmmivError("clusteringCrit DELTABIC is not supported: it needs two EM iterations per window position (GLR, DGLR and BIC are)")
        if name not in TURN_CRIT:
            raise GmmivError("unknown clusteringCrit %r (GLR, DGLR or BIC)" % (name,))
        return TURN_CRIT[name]
    return int(name)


def turn_tile_positions(D, win_size=50, win_step=5):
    """gmmiv_turn_tile_positions: positions per tile of k_turn_curve (0: the windows do not fit the LDS)"""
    return int(lib.gmmiv_turn_tile_positions(int(D), ct.c_int64(win_size), ct.c_int64(win_step)))


def plan_turn_positions(runs, nfiles, win_size=50, win_step=5):
    """gmmiv_plan_turn_positions (pure host) on the run table [nrun, 3] (first frame, length, file) -> pos_off [nrun + 1]"""
    r = np.ascontiguousarray(runs, np.int64).reshape(-1, 3)
    off = np.zeros(r.shape[0] + 1, np.int64)
    n = lib.gmmiv_plan_turn_positions(_ptr(r), ct.c_int64(r.shape[0]), ct.c_int64(nfiles), ct.c_int64(win_size), ct.c_int64(win_step), _ptr(off))
    if n < 0:
        raise GmmivError("gmmiv error: %s" % lib.gmmiv_last_error().decode())
    return off


def score_list_class(n, streaming):
    """gmmiv_score_list_class -> (class of a distribution of n scores, threads per workgroup, scores staged in LDS)"""
    thr = ct.c_int(0); stage = ct.c_int64(0)
    k = lib.gmmiv_score_list_class(ct.c_int64(int(n)), int(bool(streaming)), ct.byref(thr), ct.byref(stage))
    return int(k), thr.value, stage.value


def plan_score_lists(off, streaming):
    """gmmiv_plan_score_lists (host only, needs no GPU) -> (cls [ndist], order [ndist], class_begin [SCORE_LIST_CLASSES + 1], classes
    that occur); streaming: the untrimmed mean_mode 0"""
    off = np.ascontiguousarray(off, np.int64)
    nd = len(off) - 1
    cls = np.zeros(max(nd, 0), np.int32); order = np.zeros(max(nd, 0), np.int32); cb = np.zeros(SCORE_LIST_CLASSES + 1, np.int64)
    used = lib.gmmiv_plan_score_lists(ct.c_int64(nd), _ptr(off), int(bool(streaming)), _ptr(cls), _ptr(order), _ptr(cb))
    if used < 0:
        raise GmmivError("gmmiv_plan_score_lists: bad offsets")
    return cls, order, cb, int(used)


def _data_ptr(a):
    return a.data_ptr() if _is_torch(a) else a.ctypes.data


COMM_ID_BYTES = 128
_HOOK_T = ct.CFUNCTYPE(None, ct.c_void_p)
lib.gmmiv_ctx_set_hook.argtypes = [ct.c_void_p, ct.c_char_p, ct.c_void_p, ct.c_void_p]


class Comm:
    """gmmiv_comm: the RCCL communicator of one context (one rank per GPU).  world == 1 needs no id and no RCCL.
    Buffers: torch CUDA tensors (float64, contiguous) are used in place; numpy arrays are accepted by allreduce / broadcast."""

    def __init__(self, ctx, world=1, rank=0, uid=None):
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        self._h = ct.c_void_p()
        if world > 1 and (uid is None or len(uid) != COMM_ID_BYTES):
            raise GmmivError("Comm: world > 1 needs the %d-byte id of rank 0 (Comm.unique_id())" % COMM_ID_BYTES)
        buf = ct.create_string_buffer(bytes(uid), COMM_ID_BYTES) if uid is not None else None
        _chk(lib.gmmiv_comm_create(ctx._h, self.world, self.rank, buf, ct.byref(self._h)))

    @staticmethod
    def unique_id(transport=None):
        """transport: "rccl", "shm" (ranks sharing a GPU / no RCCL; see include/gmmiv.h) or None = $GMMIV_COMM_TRANSPORT, else rccl."""
        buf = ct.create_string_buffer(COMM_ID_BYTES)
        _chk(lib.gmmiv_comm_get_unique_id_for(transport.encode() if transport else None, buf))
        return buf.raw

    @staticmethod
    def exchange_id_file(path, rank, timeout_s=120.0):
        buf = ct.create_string_buffer(COMM_ID_BYTES)
        _chk(lib.gmmiv_comm_exchange_id_file(path.encode(), int(rank), buf, ct.c_double(timeout_s)))
        return buf.raw

    def close(self):
        if self._h:
            lib.gmmiv_comm_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            if sys is None or sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def backend(self):
        return lib.gmmiv_comm_backend(self._h).decode()

    def info(self):
        """{"rccl_version": ncclGetVersion code, "rccl_comm_count": ncclCommCount} -- zeros when no RCCL is behind the communicator."""
        v, n = ct.c_int(0), ct.c_int(0)
        _chk(lib.gmmiv_comm_info(self._h, ct.byref(v), ct.byref(n)))
        return {"rccl_version": v.value, "rccl_comm_count": n.value}

    def take_bytes(self):
        return lib.gmmiv_comm_take_bytes(self._h)

    @staticmethod
    def _n(a):
        return a.numel() if _is_torch(a) else a.size

    def allreduce(self, a):
        _chk(lib.gmmiv_allreduce_f64(self._h, _ptr(a), ct.c_size_t(self._n(a))))
        return a

    def broadcast(self, a, root=0):
        _chk(lib.gmmiv_broadcast_f64(self._h, _ptr(a), ct.c_size_t(self._n(a)), int(root)))
        return a

    def reduce_scatter(self, send, recv):
        assert self._n(send) == self.world * self._n(recv)
        _chk(lib.gmmiv_reduce_scatter_f64(self._h, _ptr(send), _ptr(recv), ct.c_size_t(self._n(recv))))
        return recv

    def allgather(self, send, recv):
        assert self._n(recv) == self.world * self._n(send)
        _chk(lib.gmmiv_allgather_f64(self._h, _ptr(send), _ptr(recv), ct.c_size_t(self._n(send))))
        return recv

    # overlapped forms (device tensors): the collective runs on the communicator's side stream behind what the context's stream
    # holds so far; join() orders the context's stream behind everything begun since the last join
    def allreduce_begin(self, a):
        _chk(lib.gmmiv_allreduce_f64_begin(self._h, _ptr(a), ct.c_size_t(self._n(a))))
        return a

    def reduce_scatter_begin(self, send, recv):
        assert self._n(send) == self.world * self._n(recv)
        _chk(lib.gmmiv_reduce_scatter_f64_begin(self._h, _ptr(send), _ptr(recv), ct.c_size_t(self._n(recv))))
        return recv

    def allgather_begin(self, send, recv):
        assert self._n(recv) == self.world * self._n(send)
        _chk(lib.gmmiv_allgather_f64_begin(self._h, _ptr(send), _ptr(recv), ct.c_size_t(self._n(send))))
        return recv

    def join(self):
        _chk(lib.gmmiv_comm_join(self._h))


def shard_range(n, rank, world):
    """gmmiv_shard_range: contiguous [begin, end) of rank's share of n items."""
    b, e = ct.c_int64(), ct.c_int64()
    lib.gmmiv_shard_range(ct.c_int64(n), int(rank), int(world), ct.byref(b), ct.byref(e))
    return b.value, e.value


class Gmm:
    """Device-resident MixtureGD: w[C], mean[C,D], covinv[C,D]."""

    def __init__(self, ctx, w, mean, covinv):
        self.ctx = ctx
        w, mean, covinv = _f64(w), _f64(mean), _f64(covinv)
        self.C, self.D = mean.shape
        self._h = ct.c_void_p()
        _chk(lib.gmmiv_gmm_create(ctx._h, self.C, self.D, _ptr(w), _ptr(mean), _ptr(covinv), ct.byref(self._h)))
        ctx._models.add(self)

    def set(self, w, mean, covinv):
        _chk(lib.gmmiv_gmm_set(self._h, _ptr(_f64(w)), _ptr(_f64(mean)), _ptr(_f64(covinv))))

    def set_cov(self, w, mean, cov):
        _chk(lib.gmmiv_gmm_set_cov(self._h, _ptr(_f64(w)), _ptr(_f64(mean)), _ptr(_f64(cov))))

    def close(self):
        if self._h:
            lib.gmmiv_gmm_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            if sys is None or sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def llk(self, x, min_llk=-200.0, max_llk=200.0, out=None, sums=None):
        x, dt, T, ldx = _feat(x)
        if out is None:
            out = np.empty(T)
        _chk(lib.gmmiv_llk(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), ct.c_double(min_llk),
                           ct.c_double(max_llk), _ptr(out), _ptr(sums)))
        return out

    def llk_determine_top(self, x, ctop, complete=True, min_llk=-200.0, max_llk=200.0):
        x, dt, T, ldx = _feat(x)
        ctop = min(ctop, self.C)
        idx = np.empty((T, ctop), np.int32)
        lk = np.empty((T, ctop)); nlk = np.empty(T); nllk = np.empty(T); nw = np.empty(T); out = np.empty(T)
        _chk(lib.gmmiv_llk_determine_top(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), ctop,
                                         TOP_COMPLETE if complete else TOP_PARTIAL, ct.c_double(min_llk),
                                         ct.c_double(max_llk), _ptr(idx), _ptr(lk), _ptr(nlk), _ptr(nllk), _ptr(nw),
                                         _ptr(out)))
        return dict(idx=idx, lk=lk, nontop_lk=nlk, nontop_llk=nllk, nontop_w=nw, llk=out)

    def topgauss_compute(self, x, cap, top_gauss, complete=True, min_llk=-200.0, max_llk=200.0):
        """gmmiv_topgauss_compute (TopGauss::compute): top_gauss >= 1 a fixed count, < 1 a share of the frame's likelihood -> dict(idx
        [T, cap] with -1 behind the selection, count [T], snsw, snsl, llk [T], n_capped)"""
        x, dt, T, ldx = _feat(x)
        idx = np.empty((T, cap), np.int32); count = np.empty(T, np.int32)
        snsw = np.empty(T); snsl = np.empty(T); out = np.empty(T)
        n_capped = ct.c_int64(0)
        _chk(lib.gmmiv_topgauss_compute(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), int(cap), ct.c_double(top_gauss),
                                        TOP_COMPLETE if complete else TOP_PARTIAL, ct.c_double(min_llk), ct.c_double(max_llk), _ptr(idx),
                                        _ptr(count), _ptr(snsw), _ptr(snsl), _ptr(out), ct.byref(n_capped)))
        return dict(idx=idx, count=count, snsw=snsw, snsl=snsl, llk=out, n_capped=int(n_capped.value))

    def llk_use_top(self, x, idx, nontop_llk, complete=True, min_llk=-200.0, max_llk=200.0):
        x, dt, T, ldx = _feat(x)
        idx = np.ascontiguousarray(idx, np.int32)
        out = np.empty(T)
        _chk(lib.gmmiv_llk_use_top(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), idx.shape[1],
                                   _ptr(idx), _ptr(_f64(nontop_llk)), TOP_COMPLETE if complete else TOP_PARTIAL,
                                   ct.c_double(min_llk), ct.c_double(max_llk), _ptr(out)))
        return out

    @staticmethod
    def llk_use_top_multi(clients, x, idx, nontop_llk, complete=True, min_llk=-200.0, max_llk=200.0):
        """USE_TOP_DISTRIBS for a list of client models on the same frames and world indices (ComputeTest's client loop) in one
        call: [len(clients), T]."""
        x, dt, T, ldx = _feat(x)
        idx = np.ascontiguousarray(idx, np.int32)
        n = len(clients)
        out = np.empty((n, T))
        if n == 0:
            return out
        arr = (ct.c_void_p * n)(*[g._h for g in clients])
        _chk(lib.gmmiv_llk_use_top_multi(clients[0].ctx._h, n, arr, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), idx.shape[1],
                                         _ptr(idx), _ptr(_f64(nontop_llk)), TOP_COMPLETE if complete else TOP_PARTIAL,
                                         ct.c_double(min_llk), ct.c_double(max_llk), _ptr(out)))
        return out

    def occ(self, x):
        """Posterior vectors [T x C] (computeAndAccumulateOcc / getOccVect)."""
        x, dt, T, ldx = _feat(x)
        out = np.empty((T, self.C))
        _chk(lib.gmmiv_occ(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), _ptr(out)))
        return out

    def feat_compensate(self, x, offset, out=None, out_dtype=None):
        """out[t] = x[t] - sum_c gamma_tc offset[c] with this model's full posteriors (JFAAcc::normalizeFeatures).  x, out: numpy or
        torch device frame matrices (row-strided views allowed); out=None allocates one of out_dtype (default: x's), out=x is in place."""
        x, dt, T, ldx = _feat_view(x)
        if out is None:
            out = _feat_like(x, dt if out_dtype is None else out_dtype)
        out, odt, To, ldo = _feat_view(out)
        assert To == T and out.shape[1] == x.shape[1] == self.D
        off = offset if _is_torch(offset) else np.ascontiguousarray(offset, np.float64)
        _chk(lib.gmmiv_feat_compensate(self.ctx._h, self._h, _vptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), _ptr(off), _vptr(out), odt,
                                       ct.c_int64(ldo)))
        return out

    def feat_map(self, cd_mean, cd_cov, ci_mean, ci_cov, x, out=None, out_dtype=None, best=True):
        """Feature mapping (featureMapping, GeneralTools.cpp:762-811) with this model as the channel-dependent one: -> (out, best);
        best: int32 [T] (numpy, or torch device when x is), or None with best=False."""
        x, dt, T, ldx = _feat_view(x)
        if out is None:
            out = _feat_like(x, dt if out_dtype is None else out_dtype)
        out, odt, To, ldo = _feat_view(out)
        assert To == T and out.shape[1] == x.shape[1] == self.D
        tabs = [a if _is_torch(a) else np.ascontiguousarray(a, np.float64) for a in (cd_mean, cd_cov, ci_mean, ci_cov)]
        b = None
        if best is True:
            if _is_torch(x):
                import torch
                b = torch.empty(T, dtype=torch.int32, device=x.device)
            else:
                b = np.empty(T, np.int32)
        elif best is not False and best is not None:
            b = best
        _chk(lib.gmmiv_feat_map(self.ctx._h, self._h, _ptr(tabs[0]), _ptr(tabs[1]), _ptr(tabs[2]), _ptr(tabs[3]), _vptr(x), dt, ct.c_int64(T),
                                ct.c_int64(ldx), _vptr(out), odt, ct.c_int64(ldo), _ptr(b)))
        return out, b

    def em_acc_len(self):
        return lib.gmmiv_em_acc_len(self.C, self.D)

    def em_accumulate(self, x, weight=1.0, acc=None):
        x, dt, T, ldx = _feat(x)
        if acc is None:
            acc = np.zeros(self.em_acc_len())
        _chk(lib.gmmiv_em_accumulate(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx),
                                     ct.c_double(weight), _ptr(acc)))
        return acc

    def em_get(self, acc, prev_mean, prev_cov):
        C, D = self.C, self.D
        w = np.empty(C); mean = np.empty((C, D)); cov = np.empty((C, D))
        _chk(lib.gmmiv_em_get(self.ctx._h, C, D, _ptr(acc), _ptr(_f64(prev_mean)), _ptr(_f64(prev_cov)), _ptr(w),
                              _ptr(mean), _ptr(cov)))
        return w, mean, cov

    def split_acc(self, acc):
        C, D = self.C, self.D
        a = np.asarray(acc)
        return dict(occ=a[:C], sx=a[C:C + C * D].reshape(C, D), sxx=a[C + C * D:C + 2 * C * D].reshape(C, D),
                    llk=a[-2], count=a[-1])

    def tv_stats_lines(self, x, file_begin, lines, N=None, F=None):
        """Baum-Welch statistics per ndx LINE: lines = list of lists of file indices (a file may appear on several lines)."""
        x, dt, T, ldx = _feat(x)
        fb = np.ascontiguousarray(file_begin, dtype=np.int64)
        off = np.zeros(len(lines) + 1, np.int64)
        off[1:] = np.cumsum([len(l) for l in lines])
        files = np.ascontiguousarray([f for l in lines for f in l], dtype=np.int64) if off[-1] else np.zeros(1, np.int64)
        if N is None:
            N = np.empty((len(lines), self.C)); F = np.empty((len(lines), self.C * self.D))
        _chk(lib.gmmiv_tv_stats_lines(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), fb.ctypes.data_as(ct.c_void_p),
                                      ct.c_int64(len(fb) - 1), ct.c_int64(len(lines)), off.ctypes.data_as(ct.c_void_p),
                                      files.ctypes.data_as(ct.c_void_p), _ptr(N), _ptr(F)))
        return N, F

    def tv_stats(self, x, utt_begin, N=None, F=None):
        x, dt, T, ldx = _feat(x)
        ub = np.ascontiguousarray(utt_begin, dtype=np.int64)
        U = len(ub) - 1
        if N is None:
            N = np.empty((U, self.C)); F = np.empty((U, self.C * self.D))
        _chk(lib.gmmiv_tv_stats(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx),
                                ub.ctypes.data_as(ct.c_void_p), ct.c_int64(U), _ptr(N), _ptr(F)))
        return N, F


class ModelTile(ct.Structure):
    """gmmiv_model_tile: one workgroup of the batched log-likelihood kernel"""
    _fields_ = [("first", ct.c_int64), ("lo", ct.c_int64), ("hi", ct.c_int64), ("model", ct.c_int32), ("seg", ct.c_int32),
                ("pad_lo", ct.c_int32), ("pad_hi", ct.c_int32)]


def plan_model_tiles(seg_begin, seg_model, tile_frames=256):
    """gmmiv_plan_model_tiles (host only, needs no GPU) -> list of dicts first / lo / hi / model / seg / pad_lo / pad_hi"""
    sb = np.ascontiguousarray(seg_begin, np.int64)
    sm = np.ascontiguousarray(seg_model, np.int32)
    nseg = len(sb) - 1
    assert len(sm) == nseg
    args = (sb.ctypes.data_as(ct.c_void_p), sm.ctypes.data_as(ct.c_void_p), ct.c_int64(nseg), int(tile_frames))
    n = lib.gmmiv_plan_model_tiles(*args, ct.c_void_p(0), ct.c_int64(0))
    if n < 0:
        raise GmmivError("gmmiv_plan_model_tiles: bad argument")
    buf = (ModelTile * max(int(n), 1))()
    lib.gmmiv_plan_model_tiles(*args, ct.cast(buf, ct.c_void_p), ct.c_int64(n))
    return [{k: getattr(buf[i], k) for k, _ in ModelTile._fields_} for i in range(int(n))]


class FeatTile(ct.Structure):
    """gmmiv_feat_tile: one wave of the segment-aware k_feat_comp"""
    _fields_ = [("block", ct.c_int64), ("lo", ct.c_int64), ("hi", ct.c_int64), ("model", ct.c_int32), ("seg", ct.c_int32)]


def plan_feat_tiles(seg_begin, seg_model, blocks_per_tile=2, cap=None, count_only=False):
    """gmmiv_plan_feat_tiles (host only, needs no GPU) -> list of dicts block / lo / hi / model / seg, sorted by (seg, block); cap: at
    most that many entries are written (-> (count, the written entries)); count_only: the count alone (tiles = NULL)"""
    sb = np.ascontiguousarray(seg_begin, np.int64)
    sm = np.ascontiguousarray(seg_model, np.int32)
    nseg = len(sb) - 1
    assert len(sm) == nseg
    args = (sb.ctypes.data_as(ct.c_void_p), sm.ctypes.data_as(ct.c_void_p), ct.c_int64(nseg), int(blocks_per_tile))
    n = lib.gmmiv_plan_feat_tiles(*args, ct.c_void_p(0), ct.c_int64(0))
    if n < 0:
        raise GmmivError("gmmiv_plan_feat_tiles: bad argument")
    if count_only:
        return int(n)
    room = int(n) if cap is None else int(cap)
    buf = (FeatTile * max(room, 1))()
    n2 = lib.gmmiv_plan_feat_tiles(*args, ct.cast(buf, ct.c_void_p), ct.c_int64(room))
    tiles = [{k: getattr(buf[i], k) for k, _ in FeatTile._fields_} for i in range(min(int(n2), room))]
    return tiles if cap is None else (int(n2), tiles)


TRIAL_PIECE = int(lib.gmmiv_trial_piece(None))  # GMMIV_TRIAL_PIECE, read from the library: frames per work item of gmmiv_llr_trials


class TrialTile(ct.Structure):
    """gmmiv_trial_tile: one workgroup of the trial kernel"""
    _fields_ = [("lo", ct.c_int64), ("hi", ct.c_int64), ("trial", ct.c_int32), ("seg", ct.c_int32), ("model", ct.c_int32), ("piece", ct.c_int32)]


def plan_trial_tiles(seg_begin, trial_seg, trial_model, piece_frames=TRIAL_PIECE, count_only=False):
    """gmmiv_plan_trial_tiles (host only, needs no GPU) -> list of dicts lo / hi / trial / seg / model / piece, sorted by (segment, piece,
    position of the trial); count_only: the number of tiles alone (tiles = NULL)"""
    sb = np.ascontiguousarray(seg_begin, np.int64)
    ts = np.ascontiguousarray(trial_seg, np.int32)
    tm = np.ascontiguousarray(trial_model, np.int32)
    assert len(sb) >= 1 and len(ts) == len(tm)
    args = (sb.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sb) - 1), ts.ctypes.data_as(ct.c_void_p), tm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(ts)),
            int(piece_frames))
    n = lib.gmmiv_plan_trial_tiles(*args, ct.c_void_p(0), ct.c_int64(0))
    if n < 0:
        raise GmmivError("gmmiv_plan_trial_tiles: bad argument")
    if count_only:
        return int(n)
    buf = (TrialTile * max(int(n), 1))()
    lib.gmmiv_plan_trial_tiles(*args, ct.cast(buf, ct.c_void_p), ct.c_int64(n))
    return [{k: getattr(buf[i], k) for k, _ in TrialTile._fields_} for i in range(int(n))]


lib.gmmiv_plan_iv_trial_tiles.restype = ct.c_int64
IV_TRIAL_PIECE = int(lib.gmmiv_iv_trial_piece(None))  # GMMIV_IV_TRIAL_PIECE, read from the library
IV_ANCHOR_AUTO, IV_ANCHOR_MODEL, IV_ANCHOR_SEG = 0, 1, 2


class IvTrialTile(ct.Structure):
    """gmmiv_iv_trial_tile: one wave of k_score_trials"""
    _fields_ = [("anchor", ct.c_int32), ("reserved", ct.c_int32), ("lo", ct.c_int64), ("hi", ct.c_int64)]


def iv_trial_anchor(M, S, trial_model, trial_seg):
    """gmmiv_iv_trial_anchor (host only): IV_ANCHOR_SEG when the list names fewer distinct segments than models, else IV_ANCHOR_MODEL"""
    tm = np.ascontiguousarray(trial_model, np.int32)
    ts = np.ascontiguousarray(trial_seg, np.int32)
    r = lib.gmmiv_iv_trial_anchor(ct.c_int64(M), ct.c_int64(S), tm.ctypes.data_as(ct.c_void_p), ts.ctypes.data_as(ct.c_void_p), ct.c_int64(len(tm)))
    if r < 0:
        raise GmmivError("gmmiv_iv_trial_anchor: bad argument")
    return int(r)


def plan_iv_trial_tiles(M, S, trial_model, trial_seg, anchor=IV_ANCHOR_AUTO, piece=IV_TRIAL_PIECE, cap=None):
    """gmmiv_plan_iv_trial_tiles (host only, needs no GPU) -> (order [ntrial] int64: list positions sorted by (anchor, partner, position),
    tiles: list of (anchor, lo, hi), the number of tiles counted).  cap: write at most that many tiles (the count still covers all)."""
    tm = np.ascontiguousarray(trial_model, np.int32)
    ts = np.ascontiguousarray(trial_seg, np.int32)
    assert len(tm) == len(ts)
    args = (ct.c_int64(M), ct.c_int64(S), tm.ctypes.data_as(ct.c_void_p), ts.ctypes.data_as(ct.c_void_p), ct.c_int64(len(tm)), int(anchor), int(piece))
    n = lib.gmmiv_plan_iv_trial_tiles(*args, ct.c_void_p(0), ct.c_void_p(0), ct.c_int64(0))
    if n < 0:
        raise GmmivError("gmmiv_plan_iv_trial_tiles: bad argument")
    keep = int(n) if cap is None else min(int(cap), int(n))
    guard = 4                                           # entries behind `cap` that must stay untouched
    buf = (IvTrialTile * (keep + guard))()
    for i in range(keep, keep + guard):
        buf[i].anchor = -7
    order = np.zeros(len(tm), np.int64)
    n2 = lib.gmmiv_plan_iv_trial_tiles(*args, order.ctypes.data_as(ct.c_void_p), ct.cast(buf, ct.c_void_p), ct.c_int64(keep))
    assert n2 == n and all(buf[i].anchor == -7 for i in range(keep, keep + guard))
    return order, [(buf[i].anchor, buf[i].lo, buf[i].hi) for i in range(keep)], int(n)


MAP_METHODS = {"MAPOccDep": 1, "MAPModelBased": 2, "MAPConst": 3, "MAPConst2": 4}  # anything else: 0, the ML estimate (computeMAP's "mapAlgo unknown")


class GmmBatch:
    """G device-resident models of one shape, a model per SEGMENT of the frame matrix (batched enrolment / getLLK for many files)."""

    def __init__(self, ctx, G, C, D):
        self.ctx, self.G, self.C, self.D = ctx, int(G), int(C), int(D)
        self._h = ct.c_void_p()
        _chk(lib.gmmiv_gmm_batch_create(ctx._h, self.G, self.C, self.D, ct.byref(self._h)))
        ctx._models.add(self)

    def close(self):
        if self._h:
            lib.gmmiv_gmm_batch_destroy(self._h)
            self._h = ct.c_void_p()

    def __del__(self):
        try:
            if sys is None or sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def _stride(self, a, row):
        """[row] or [1, row]: shared (stride 0); [G, row]: one per model"""
        n = a.numel() if _is_torch(a) else a.size
        assert n in (row, self.G * row), "a table is shared ([%d]) or per model ([%d x %d])" % (row, self.G, row)
        return 0 if n == row and self.G > 1 else row

    def load(self, w, mean, covinv, strides=None):
        """w [C] or [G, C]; mean, covinv [C, D] or [G, C, D] (numpy or torch device): a table with one model's size is shared by all G.
        strides = (w, mean, covinv) in doubles: the tables are then pointers to model 0 (model g at p + g * stride), not sized arrays."""
        CD = self.C * self.D
        if strides is not None:
            _chk(lib.gmmiv_gmm_batch_load(self._h, _vptr(w), ct.c_int64(strides[0]), _vptr(mean), ct.c_int64(strides[1]), _vptr(covinv),
                                          ct.c_int64(strides[2])))
            return self
        w, mean, covinv = _f64(w), _f64(mean), _f64(covinv)
        _chk(lib.gmmiv_gmm_batch_load(self._h, _ptr(w), ct.c_int64(self._stride(w, self.C)), _ptr(mean), ct.c_int64(self._stride(mean, CD)),
                                      _ptr(covinv), ct.c_int64(self._stride(covinv, CD))))
        return self

    def load_cov(self, w, mean, cov):
        """load() from VARIANCES (gmmiv_gmm_batch_load_cov): covInv = 1 / cov on the device, as Gmm.set_cov"""
        w, mean, cov = _f64(w), _f64(mean), _f64(cov)
        CD = self.C * self.D
        _chk(lib.gmmiv_gmm_batch_load_cov(self._h, _ptr(w), ct.c_int64(self._stride(w, self.C)), _ptr(mean), ct.c_int64(self._stride(mean, CD)),
                                          _ptr(cov), ct.c_int64(self._stride(cov, CD))))
        return self

    def packed(self, g):
        """the packed MFMA operands of model g as a call builds them (tests: bit for bit those of a single-model handle)"""
        n = ct.c_int64()
        _chk(lib.gmmiv_gmm_batch_packed(self._h, int(g), ct.c_void_p(0), ct.byref(n)))
        out = np.empty(n.value)
        _chk(lib.gmmiv_gmm_batch_packed(self._h, int(g), _ptr(out), ct.byref(n)))
        return out

    @staticmethod
    def _segs(seg_begin, seg_model):
        sb = np.ascontiguousarray(seg_begin, np.int64)
        sm = np.ascontiguousarray(seg_model, np.int32)
        assert len(sb) == len(sm) + 1
        return sb, sm

    def llk(self, x, seg_begin, seg_model, min_llk=-200.0, max_llk=200.0, out=None, seg_sum=None):
        """-> (llk [T], seg_sum [nseg]); entries of llk outside the segments keep what `out` holds (a fresh array: NaN)"""
        x, dt, T, ldx = _feat(x)
        sb, sm = self._segs(seg_begin, seg_model)
        if out is None:
            out = np.full(T, np.nan)
        if seg_sum is None:
            seg_sum = np.empty(len(sm))
        _chk(lib.gmmiv_llk_models(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), sb.ctypes.data_as(ct.c_void_p),
                                  sm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sm)), ct.c_double(min_llk), ct.c_double(max_llk), _ptr(out),
                                  _ptr(seg_sum)))
        return out, seg_sum

    def tv_stats(self, x, seg_begin, seg_model, N=None, F=None, seg_llk=None):
        """-> (N [nseg, C], F [nseg, C*D], seg_llk [nseg, 2] = (sum of log-likelihoods, frames in it))"""
        x, dt, T, ldx = _feat(x)
        sb, sm = self._segs(seg_begin, seg_model)
        if N is None:
            N = np.empty((len(sm), self.C)); F = np.empty((len(sm), self.C * self.D))
        if seg_llk is None:
            seg_llk = np.empty((len(sm), 2))
        _chk(lib.gmmiv_tv_stats_models(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), sb.ctypes.data_as(ct.c_void_p),
                                       sm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sm)), _ptr(N), _ptr(F), _ptr(seg_llk)))
        return N, F, seg_llk

    def em_stats(self, x, seg_begin, seg_model, N=None, F=None, S=None, seg_llk=None):
        """gmmiv_em_stats_models -> (N [nseg, C], F [nseg, C*D], S [nseg, C*D] = sum g x^2, seg_llk [nseg, 2])"""
        x, dt, T, ldx = _feat(x)
        sb, sm = self._segs(seg_begin, seg_model)
        if N is None:
            N = np.empty((len(sm), self.C)); F = np.empty((len(sm), self.C * self.D)); S = np.empty((len(sm), self.C * self.D))
        if seg_llk is None:
            seg_llk = np.empty((len(sm), 2))
        _chk(lib.gmmiv_em_stats_models(self.ctx._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), sb.ctypes.data_as(ct.c_void_p),
                                       sm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sm)), _ptr(N), _ptr(F), _ptr(S), _ptr(seg_llk)))
        return N, F, S, seg_llk

    def feat_compensate(self, x, seg_begin, seg_model, offsets, out=None, out_dtype=None):
        """gmmiv_feat_compensate_models: segment s of x is rewritten as out[t] = x[t] - sum_c gamma_tc offsets[seg_model[s]][c] with the
        full posteriors of model seg_model[s].  offsets: [C, D] (shared) or [G, C, D], numpy or torch device.  x, out as in
        Gmm.feat_compensate (row-strided views allowed, out=x is in place); frames of no segment are not touched: with out=None they
        are x's own (the fresh output starts as a copy of x in out_dtype)."""
        x, dt, T, ldx = _feat_view(x)
        sb, sm = self._segs(seg_begin, seg_model)
        if out is None:
            out = _feat_like(x, dt if out_dtype is None else out_dtype)
            if _is_torch(out):
                out.copy_(x)
            else:
                out[...] = x
        out, odt, To, ldo = _feat_view(out)
        assert To == T and out.shape[1] == x.shape[1] == self.D
        off = offsets if _is_torch(offsets) else np.ascontiguousarray(offsets, np.float64)
        _chk(lib.gmmiv_feat_compensate_models(self.ctx._h, self._h, _vptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), sb.ctypes.data_as(ct.c_void_p),
                                              sm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(sm)), _ptr(off),
                                              ct.c_int64(self._stride(off, self.C * self.D)), _vptr(out), odt, ct.c_int64(ldo)))
        return out

    def llr_trials(self, world, x, seg_begin, trial_seg, trial_model, ctop, complete=True, min_llk=-200.0, max_llk=200.0, llr=None, client_mean=None,
                   world_mean=None):
        """gmmiv_llr_trials: the GMM-UBM scores of the trials (trial_seg[i], trial_model[i]) -- segment of x, model of this batch -- against
        the single-model handle `world`, in one device pass -> (llr [ntrial], client_mean [ntrial], world_mean [nseg]).  The outputs are
        numpy arrays unless given.  With torch device tensors the results are written in the order of the context's stream: the call
        itself waits for that stream while it uploads its tables and inside the world pass, but NOT after its last kernels --
        ctx.sync() before reading the tensors on another stream.  seg_begin / trial_seg / trial_model are host lists."""
        x, dt, T, ldx = _feat(x)
        sb = np.ascontiguousarray(seg_begin, np.int64)
        ts = np.ascontiguousarray(trial_seg, np.int32)
        tm = np.ascontiguousarray(trial_model, np.int32)
        assert sb.ndim == 1 and len(sb) >= 1 and ts.shape == tm.shape and ts.ndim == 1
        if llr is None:
            llr = np.empty(len(ts))
        if client_mean is None:
            client_mean = np.empty(len(ts))
        if world_mean is None:
            world_mean = np.empty(len(sb) - 1)
        _chk(lib.gmmiv_llr_trials(self.ctx._h, world._h, self._h, _ptr(x), dt, ct.c_int64(T), ct.c_int64(ldx), sb.ctypes.data_as(ct.c_void_p),
                                  ct.c_int64(len(sb) - 1), ts.ctypes.data_as(ct.c_void_p), tm.ctypes.data_as(ct.c_void_p), ct.c_int64(len(ts)), int(ctop),
                                  TOP_COMPLETE if complete else TOP_PARTIAL, ct.c_double(min_llk), ct.c_double(max_llk), _ptr(llr), _ptr(client_mean),
                                  _ptr(world_mean)))
        return llr, client_mean, world_mean

    def map_adapt(self, N, F, count, w0, mean0, cur_mean, method="MAPOccDep", mean=True, weight=False, reg=(16.0, 16.0, 16.0), alpha_mean=0.75,
                  mean_out=None, w_out=None, count_stride=1, cur_stride=None):
        """computeMAP for the G statistics rows (gmmiv_map_adapt_models): -> (means [G, C*D], weights [G, C]).  reg = (mean, var, weight)
        like host_capi.compute_map; cur_mean [C*D] (shared) or [G, C*D]; count [G] (count_stride 1) or e.g. seg_llk[:, 1] as stride 2.
        cur_stride (doubles): cur_mean is then a pointer to model 0's means, model g at cur_mean + g * cur_stride."""
        G, C, D = self.G, self.C, self.D
        tor = _is_torch(N)
        if mean_out is None:
            if tor:
                import torch
                mean_out = torch.empty((G, C * D), dtype=torch.float64, device=N.device)
                w_out = torch.empty((G, C), dtype=torch.float64, device=N.device)
            else:
                mean_out = np.empty((G, C * D)); w_out = np.empty((G, C))
        cur = _f64(cur_mean)
        _chk(lib.gmmiv_map_adapt_models(self.ctx._h, G, C, D, _ptr(_f64(N)), _ptr(_f64(F)), _ptr(_f64(count)), ct.c_int64(count_stride), _ptr(_f64(w0)),
                                        _ptr(_f64(mean0)), _vptr(cur) if cur_stride is not None else _ptr(cur),
                                        ct.c_int64(self._stride(cur, C * D) if cur_stride is None else cur_stride), MAP_METHODS.get(method, 0), int(bool(mean)),
                                        int(bool(weight)), ct.c_double(reg[0]), ct.c_double(reg[2]), ct.c_double(alpha_mean), _ptr(mean_out),
                                        _ptr(w_out)))
        return mean_out, w_out

    def map_adapt_full(self, N, F, S, count, w0, mean0, cov0, cur_mean, cur_cov, method="MAPOccDep", mean=True, var=False, weight=False,
                       reg=(16.0, 16.0, 16.0), alpha_mean=0.75, count_stride=1, want=("mean", "cov", "w")):
        """computeMAP with the variance branch (gmmiv_map_adapt_models_full) -> (means [G, C*D], covs [G, C*D], weights [G, C], status [G]
        int32); an output not named in `want` is None.  S / cur_cov may be None when no branch reads them.  Outputs live where N lives."""
        G, C, D = self.G, self.C, self.D
        if _is_torch(N):
            import torch
            mk = lambda shape, dt=torch.float64: torch.empty(shape, dtype=dt, device=N.device)
            status = mk((G,), torch.int32)
        else:
            mk = lambda shape: np.empty(shape)
            status = np.empty(G, np.int32)
        mo = mk((G, C * D)) if "mean" in want else None
        co = mk((G, C * D)) if "cov" in want else None
        wo = mk((G, C)) if "w" in want else None
        cm = _f64(cur_mean)
        cc = None if cur_cov is None else _f64(cur_cov)
        opt = lambda a: ct.c_void_p(0) if a is None else _ptr(a)
        _chk(lib.gmmiv_map_adapt_models_full(self.ctx._h, G, C, D, _ptr(_f64(N)), _ptr(_f64(F)), opt(None if S is None else _f64(S)), _ptr(_f64(count)),
                                             ct.c_int64(count_stride), _ptr(_f64(w0)), _ptr(_f64(mean0)), _ptr(_f64(cov0)), _ptr(cm),
                                             ct.c_int64(self._stride(cm, C * D)), opt(cc), ct.c_int64(0 if cc is None else self._stride(cc, C * D)),
                                             MAP_METHODS.get(method, 0), int(bool(mean)), int(bool(var)), int(bool(weight)), ct.c_double(reg[0]),
                                             ct.c_double(reg[1]), ct.c_double(reg[2]), ct.c_double(alpha_mean), opt(mo), opt(co), opt(wo), _ptr(status)))
        return mo, co, wo, status

    def normalize(self, w, mean, cov, nb_it=1, mean_only=False):
        """normalizeMixture towards N(0, 1) for the G models IN PLACE (gmmiv_normalize_models): mean, cov [G, C*D] torch device tensors,
        w [C] (shared) or [G, C]"""
        assert _is_torch(mean) and _is_torch(cov)
        w = _f64(w)
        _chk(lib.gmmiv_normalize_models(self.ctx._h, self.G, self.C, self.D, _ptr(w), ct.c_int64(self._stride(w, self.C)), _ptr(mean), _ptr(cov),
                                        int(nb_it), int(bool(mean_only))))
        return mean, cov

    def mllr_adapt(self, N, F, mean0, cov0):
        """computeMLLR for the G statistics rows (gmmiv_mllr_adapt_models) -> (W [G, D, D + 1], means [G, C*D], status [G] int32)."""
        return mllr_adapt(self.ctx, N, F, mean0, cov0, C=self.C, D=self.D)


def mllr_adapt(ctx, N, F, mean0, cov0, C=None, D=None):
    """gmmiv_mllr_adapt_models: N [G, C], F [G, C*D] (statistics rows), mean0 / cov0 [C, D] the a-priori means and VARIANCES, numpy or
    torch device tensors -> (W [G, D, D + 1], means [G, C*D], status [G] int32; 0, or 1 + the first dimension whose system failed: that
    client has W = [0 | I] and means = mean0).  Outputs live where N lives; with device tensors the call only enqueues."""
    G = int(N.shape[0])
    C = int(N.shape[1]) if C is None else int(C)
    D = (int(F.shape[1]) // C) if D is None else int(D)
    if _is_torch(N):
        import torch
        W = torch.empty((G, D, D + 1), dtype=torch.float64, device=N.device)
        means = torch.empty((G, C * D), dtype=torch.float64, device=N.device)
        status = torch.empty((G,), dtype=torch.int32, device=N.device)
    else:
        W = np.empty((G, D, D + 1)); means = np.empty((G, C * D)); status = np.empty(G, np.int32)
    _chk(lib.gmmiv_mllr_adapt_models(ctx._h, G, C, D, _ptr(_f64(N)), _ptr(_f64(F)), _ptr(_f64(mean0)), _ptr(_f64(cov0)), _ptr(W), _ptr(means),
                                     _ptr(status)))
    return W, means, status
