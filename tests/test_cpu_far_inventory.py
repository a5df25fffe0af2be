"""The inventory of the far-addressing programme (tests/test_gpu_far_addressing.py): every function of every header under include/ that
takes a stride -- a parameter named ld*, sA / sB / sC or *_stride -- or a table of frame numbers is named in FAR with the capi method the
GPU module calls on frames beyond 2^32 bytes / 2^31 elements from its pointer, or sits in FAR_EXEMPT with a one-line reason.  A function
in neither table fails the test: a new strided entry point cannot arrive without one or the other."""
import os
import re

from conftest import ROOT
from test_cpu_ws_history import abi_functions, binding_calls

MODULE = "test_gpu_far_addressing"

STRIDE = re.compile(r"\b(ld[a-z0-9]*|s[ABC]|[a-z_]*_stride)\b\s*(?:,|$)")
# int64 tables whose entries are frame numbers of a frame matrix the same call takes (`x`, or `v` for the per-frame values)
FRAME_TABLE = re.compile(r"\bint64_t\s*\*\s*(runs|frame_idx|file_begin|seg_begin|utt_begin)\b")
FRAMES = re.compile(r"\bvoid\s*\*\s*x\b|\bconst\s+double\s*\*\s*v\b")

# ABI function -> (the capi method, the call of it in the GPU module: the receiver tells the single-model handle g from the batch b)
FAR = {
    "gmmiv_llk": ("llk", "g.llk("),
    "gmmiv_occ": ("occ", "g.occ("),
    "gmmiv_em_accumulate": ("em_accumulate", "g.em_accumulate("),
    "gmmiv_tv_stats": ("tv_stats", "g.tv_stats("),
    "gmmiv_tv_stats_lines": ("tv_stats_lines", "g.tv_stats_lines("),
    "gmmiv_llk_determine_top": ("llk_determine_top", "g.llk_determine_top("),
    "gmmiv_llk_use_top": ("llk_use_top", "clients[0].llk_use_top("),
    "gmmiv_llk_use_top_multi": ("llk_use_top_multi", ".llk_use_top_multi(clients,"),
    "gmmiv_topgauss_compute": ("topgauss_compute", "g.topgauss_compute("),
    "gmmiv_count_unusable_frames": ("count_unusable_frames", "ctx.count_unusable_frames(v)"),
    "gmmiv_frame_moments": ("frame_moments", "ctx.frame_moments(v)"),
    "gmmiv_llk_models": ("llk", "b.llk("),
    "gmmiv_tv_stats_models": ("tv_stats", "b.tv_stats("),
    "gmmiv_em_stats_models": ("em_stats", "b.em_stats("),
    "gmmiv_feat_compensate_models": ("feat_compensate", "b.feat_compensate("),
    "gmmiv_llr_trials": ("llr_trials", "b.llr_trials("),
    "gmmiv_gmm_batch_load": ("load", "got_b.load(wd, view,"),
    "gmmiv_map_adapt_models": ("map_adapt", "want_b.map_adapt(Nd, Fd, cnt, w, mean, view, cur_stride=stride"),
    "gmmiv_gather_frames": ("gather_frames", "ctx.gather_frames("),
    "gmmiv_gather_runs": ("gather_runs", "ctx.gather_runs("),
    "gmmiv_scatter_runs": ("scatter_runs", "ctx.scatter_runs("),
    "gmmiv_frame_moments_groups": ("frame_moments_groups", "ctx.frame_moments_groups("),
    "gmmiv_feat_norm_apply": ("feat_norm_apply", "ctx.feat_norm_apply("),
    "gmmiv_feat_norm_online": ("feat_norm_online", "ctx.feat_norm_online("),
    "gmmiv_feat_norm_window": ("feat_norm_window", "ctx.feat_norm_window("),
    "gmmiv_feat_compensate": ("feat_compensate", "g.feat_compensate("),
    "gmmiv_feat_map": ("feat_map", "g.feat_map("),
    "gmmiv_energy_train": ("energy_train", "ctx.energy_train("),
    "gmmiv_energy_select": ("energy_select", "ctx.energy_select("),
    "gmmiv_turn_curve": ("turn_curve", "ctx.turn_curve("),
    "gmmiv_segment_means": ("segment_means", "ctx.segment_means(view,"),
    "gmmiv_score_cohort_stats": ("score_cohort_stats", "ctx.score_cohort_stats(view,"),
    "gmmiv_dgemm": ("dgemm", "ctx.dgemm("),
}
_TWIN = "same launcher and stride arithmetic as %s, which is run far; its tables are C x D doubles per model"
_HOST = "pure host planner: integers in, integers out, no device pointer is offset"
FAR_EXEMPT = {
    "gmmiv_gmm_batch_load_cov": _TWIN % "gmmiv_gmm_batch_load (batch_load in capi_models.hip serves both)",
    "gmmiv_map_adapt_models_full": _TWIN % "gmmiv_map_adapt_models (mean_out / w_out are that function's bits by the header)",
    "gmmiv_normalize_models": "w_stride strides a [G x C] weight table read once per (model, dimension); held to shapes by test_gpu_em_models",
    "gmmiv_plan_model_tiles": _HOST, "gmmiv_plan_feat_tiles": _HOST, "gmmiv_plan_trial_tiles": _HOST, "gmmiv_plan_norm_windows": _HOST,
    "gmmiv_plan_turn_positions": _HOST,
    "gmmiv_turn_segments": "reads no frames: run bounds and decisions in, segment bounds out (64-bit integers throughout, judged exactly by test_gpu_turn)",
}


def concerned():
    out = {}
    for name, args in abi_functions().items():
        flat = " ".join(args.split())
        params = [p.strip() for p in flat.split(",")]
        stride = any(STRIDE.search(p) for p in params)
        table = bool(FRAME_TABLE.search(flat))
        if stride or table:
            out[name] = (stride, table, bool(FRAMES.search(flat)))
    return out


def test_the_rule_finds_the_strided_entry_points():
    c = concerned()
    assert len(c) >= 40
    for name in ("gmmiv_llk", "gmmiv_dgemm", "gmmiv_gmm_batch_load", "gmmiv_map_adapt_models", "gmmiv_segment_means", "gmmiv_score_cohort_stats",
                 "gmmiv_feat_norm_window", "gmmiv_turn_curve", "gmmiv_gather_frames", "gmmiv_feat_compensate_models"):
        assert name in c and c[name][0], name
    assert c["gmmiv_gather_runs"][1] and c["gmmiv_tv_stats"][1] and c["gmmiv_feat_norm_online"][1] and c["gmmiv_plan_model_tiles"][1]
    assert "gmmiv_score_normalize" not in c and "gmmiv_ctx_create" not in c and "gmmiv_turn_pick" not in c


def test_every_strided_entry_point_is_run_far_or_exempt():
    c = set(concerned())
    f = set(abi_functions())
    unknown = (set(FAR) | set(FAR_EXEMPT)) - f
    assert not unknown, "named here but in no header: %s" % sorted(unknown)
    both = set(FAR) & set(FAR_EXEMPT)
    assert not both, "run far AND exempt: %s" % sorted(both)
    missing = c - set(FAR) - set(FAR_EXEMPT)
    assert not missing, "entry points with a stride or a frame table that %s does not run far and FAR_EXEMPT does not name: %s" % (MODULE, sorted(missing))
    idle = set(FAR_EXEMPT) - c
    assert not idle, "exempt without a stride or a frame table: %s" % sorted(idle)
    for name, reason in FAR_EXEMPT.items():
        assert isinstance(reason, str) and len(reason) > 20 and "\n" not in reason, name


def test_the_gpu_module_calls_the_binding_of_every_far_function():
    calls = binding_calls()
    src = open(os.path.join(ROOT, "tests", MODULE + ".py")).read()
    assert "pytest.mark.gpu" in src
    bad = []
    for name, (method, call) in sorted(FAR.items()):
        if name not in calls.get(method, ()):
            bad.append("%s: capi.%s does not call it" % (name, method))
        if ".%s(" % method not in call or call not in src:
            bad.append("%s: %s does not hold the call %r" % (name, MODULE, call))
    assert not bad, "\n".join(bad)
