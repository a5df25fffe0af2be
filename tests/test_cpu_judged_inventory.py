"""The inventory of the per-element programme: every function of every header under include/ (gmmiv.h, gmmiv_feat_window.h,
gmmiv_iv_trials.h, gmmiv_turn.h; test_cpu_ws_history.HEADERS lists the directory) that produces numbers is named in JUDGED with the GPU test module that judges it per element (per frame, trial, system ..) against a derived bar, or
exactly -- or it sits in EXEMPT with one of four reasons.  A function in neither table fails the test, and so does a module that
does not mention the binding's method: a new entry point cannot arrive judged per array alone without this file saying so."""
import os
import re

from conftest import ROOT
from test_cpu_ws_history import abi_functions, binding_calls

# ABI function -> (the module under tests/ that judges it per element or exactly, the capi method the module calls)
JUDGED = {
    # GMM side
    "gmmiv_llk": ("test_gpu_gmm_elementwise", "llk"),
    "gmmiv_occ": ("test_gpu_gmm_elementwise", "occ"),
    "gmmiv_em_accumulate": ("test_gpu_gmm_elementwise", "em_accumulate"),
    "gmmiv_tv_stats": ("test_gpu_gmm_elementwise", "tv_stats"),
    "gmmiv_llk_determine_top": ("test_gpu_gmm_elementwise", "llk_determine_top"),
    "gmmiv_llk_use_top": ("test_gpu_topgauss_elementwise", "llk_use_top"),
    "gmmiv_llk_use_top_multi": ("test_gpu_topgauss_elementwise", "llk_use_top_multi"),
    "gmmiv_topgauss_compute": ("test_gpu_topgauss_elementwise", "topgauss_compute"),
    "gmmiv_llk_models": ("test_gpu_gmm_elementwise", "llk"),
    "gmmiv_tv_stats_models": ("test_gpu_gmm_elementwise", "tv_stats"),
    "gmmiv_tv_stats_lines": ("test_gpu_gmm_services_elementwise", "tv_stats_lines"),
    "gmmiv_segment_means": ("test_gpu_gmm_services_elementwise", "segment_means"),
    "gmmiv_em_get": ("test_gpu_gmm_services_elementwise", "em_get"),
    "gmmiv_variance_control": ("test_gpu_gmm_services_elementwise", "variance_control"),
    "gmmiv_count_unusable_frames": ("test_gpu_gmm_services_elementwise", "count_unusable_frames"),
    "gmmiv_llr_trials": ("test_gpu_trials_elementwise", "llr_trials"),
    # batched enrolment
    "gmmiv_em_stats_models": ("test_gpu_em_models", "em_stats"),
    "gmmiv_map_adapt_models": ("test_gpu_em_models", "map_adapt"),
    "gmmiv_map_adapt_models_full": ("test_gpu_em_models", "map_adapt_full"),
    "gmmiv_normalize_models": ("test_gpu_em_models", "normalize"),
    "gmmiv_mllr_adapt_models": ("test_gpu_mllr", "mllr_adapt"),
    # frames
    "gmmiv_frame_moments": ("test_gpu_feat_norm", "frame_moments"),
    "gmmiv_frame_moments_groups": ("test_gpu_feat_norm", "frame_moments_groups"),
    "gmmiv_frame_moments_stats": ("test_gpu_feat_norm", "frame_moments_stats"),
    "gmmiv_feat_norm_apply": ("test_gpu_feat_norm", "feat_norm_apply"),
    "gmmiv_feat_norm_online": ("test_gpu_feat_norm", "feat_norm_online"),
    "gmmiv_gather_frames": ("test_gpu_host", "gather_frames"),
    "gmmiv_gather_runs": ("test_gpu_host", "gather_runs"),
    "gmmiv_scatter_runs": ("test_gpu_feat_comp", "scatter_runs"),
    "gmmiv_feat_compensate": ("test_gpu_feat_comp", "feat_compensate"),
    "gmmiv_feat_map": ("test_gpu_feat_comp", "feat_map"),
    "gmmiv_feat_compensate_models": ("test_gpu_feat_comp_models", "feat_compensate"),
    "gmmiv_energy_train": ("test_gpu_energy", "energy_train"),
    "gmmiv_energy_select": ("test_gpu_energy", "energy_select"),
    # windowed NormFeat (the planner hands back doubles -- alpha -- so it is judged, exactly, not exempt) and TurnDetection
    "gmmiv_plan_norm_windows": ("test_gpu_normwin", "plan_norm_windows"),
    "gmmiv_feat_norm_window": ("test_gpu_normwin", "feat_norm_window"),
    "gmmiv_turn_curve": ("test_gpu_turn", "turn_curve"),
    "gmmiv_turn_pick": ("test_gpu_turn", "turn_pick"),
    "gmmiv_turn_segments": ("test_gpu_turn", "turn_segments"),
    # total variability: E- and M-step
    "gmmiv_tv_subtract_m": ("test_gpu_tv_elementwise", "tv_subtract_m"),
    "gmmiv_tv_subtract_m_to": ("test_gpu_tv_elementwise", "tv_subtract_m_to"),
    "gmmiv_tv_tett": ("test_gpu_tv_elementwise", "tv_tett"),
    "gmmiv_tv_estimate_w": ("test_gpu_tv_elementwise", "tv_estimate_w"),
    "gmmiv_tv_estimate_a_and_c": ("test_gpu_tv_elementwise", "tv_estimate_a_and_c"),
    "gmmiv_tv_update_t": ("test_gpu_tv_elementwise", "tv_update_t"),
    "gmmiv_tv_min_divergence": ("test_gpu_tv_elementwise", "tv_min_divergence"),
    "gmmiv_tv_orthonormalize_t": ("test_gpu_estimation_elementwise", "tv_orthonormalize_t"),
    # back end
    "gmmiv_tv_norm_statistics": ("test_gpu_backend_elementwise", "tv_norm_statistics"),
    "gmmiv_tv_subtract_m_plus_tw": ("test_gpu_backend_elementwise", "tv_subtract_m_plus_tw"),
    "gmmiv_tv_norm_t": ("test_gpu_backend_elementwise", "tv_norm_t"),
    "gmmiv_tv_weighted_cov": ("test_gpu_backend_elementwise", "tv_weighted_cov"),
    "gmmiv_tv_approximate_tctc": ("test_gpu_backend_elementwise", "tv_approximate_tctc"),
    "gmmiv_tv_estimate_w_ubm_weight": ("test_gpu_backend_elementwise", "tv_estimate_w_ubm_weight"),
    "gmmiv_tv_estimate_w_eigen": ("test_gpu_backend_elementwise", "tv_estimate_w_eigen"),
    "gmmiv_iv_normalize": ("test_gpu_backend_elementwise", "iv_normalize"),
    "gmmiv_dev_means": ("test_gpu_backend_elementwise", "dev_means"),
    "gmmiv_dev_cov_mat": ("test_gpu_backend_elementwise", "dev_cov_mat"),
    "gmmiv_dev_scatter_mat": ("test_gpu_backend_elementwise", "dev_scatter_mat"),
    "gmmiv_dev_wccn_chol": ("test_gpu_estimation_elementwise", "dev_wccn_chol"),
    "gmmiv_dev_mahalanobis": ("test_gpu_estimation_elementwise", "dev_mahalanobis"),
    "gmmiv_sym_eigen": ("test_gpu_estimation_elementwise", "sym_eigen"),
    "gmmiv_dev_efr_matrix": ("test_gpu_estimation_elementwise", "dev_efr_matrix"),
    "gmmiv_dev_lda": ("test_gpu_estimation_elementwise", "dev_lda"),
    "gmmiv_plda_em_iteration": ("test_gpu_estimation_elementwise", "plda_em_iteration"),
    "gmmiv_plda_precompute": ("test_gpu_estimation_elementwise", "plda_precompute"),
    "gmmiv_twocov_model": ("test_gpu_estimation_elementwise", "twocov_model"),
    "gmmiv_score_cosine": ("test_gpu_backend_elementwise", "score_cosine"),
    "gmmiv_score_mahalanobis": ("test_gpu_backend_elementwise", "score_mahalanobis"),
    "gmmiv_score_twocov": ("test_gpu_backend_elementwise", "score_twocov"),
    "gmmiv_score_plda": ("test_gpu_backend_elementwise", "score_plda"),
    "gmmiv_score_twocov_mix_part": ("test_gpu_backend_elementwise", "score_twocov_mix_part"),
    "gmmiv_score_apply_trials": ("test_gpu_backend_elementwise", "score_apply_trials"),
    "gmmiv_score_cosine_trials": ("test_gpu_iv_trials", "score_cosine_trials"),
    "gmmiv_score_mahalanobis_trials": ("test_gpu_iv_trials", "score_mahalanobis_trials"),
    "gmmiv_score_twocov_trials": ("test_gpu_iv_trials", "score_twocov_trials"),
    "gmmiv_score_plda_trials": ("test_gpu_iv_trials", "score_plda_trials"),
    "gmmiv_jfa_subtract": ("test_gpu_backend_elementwise", "jfa_subtract"),
    "gmmiv_jfa_subtract_sessions": ("test_gpu_backend_elementwise", "jfa_subtract_sessions"),
    "gmmiv_jfa_estimate_z": ("test_gpu_backend_elementwise", "jfa_estimate_z"),
    "gmmiv_jfa_estimate_z_and_d": ("test_gpu_backend_elementwise", "jfa_estimate_z_and_d"),
    # score normalisation, the GEMM
    "gmmiv_score_cohort_stats": ("test_gpu_score_norm", "score_cohort_stats"),
    "gmmiv_score_normalize": ("test_gpu_score_norm", "score_normalize"),
    "gmmiv_score_list_stats": ("test_gpu_score_lists", "score_list_stats"),
    "gmmiv_score_normalize_list": ("test_gpu_score_lists", "score_normalize_list"),
    "gmmiv_dgemm": ("test_gpu_dgemm", "dgemm"),
}

_CTX = "context: creation, stream, options, hooks, timers, messages -- no numerical result"
_COMM = "communicator: collectives over ranks, held to the single-rank results in test_gpu_comm.py / test_gpu_multirank.py"
_PLAN = "planner: a host function of integers (tile tables, lengths, ranges), tested exactly on the CPU"
_HANDLE = "handle: creates, loads, reads back or destroys a model; what it holds is judged through the entry points that read it"
EXEMPT_REASONS = (_CTX, _COMM, _PLAN, _HANDLE)
EXEMPT = {
    "gmmiv_ctx_create": _CTX, "gmmiv_ctx_destroy": _CTX, "gmmiv_ctx_sync": _CTX, "gmmiv_ctx_stream": _CTX, "gmmiv_last_error": _CTX,
    "gmmiv_version": _CTX, "gmmiv_ctx_set_option": _CTX, "gmmiv_ctx_set_hook": _CTX, "gmmiv_ctx_last_kernel_ms": _CTX,
    "gmmiv_ctx_kernel_ms": _CTX, "gmmiv_ctx_kernel_launches": _CTX, "gmmiv_ctx_workspace_bytes": _CTX,
    "gmmiv_gmm_create": _HANDLE, "gmmiv_gmm_set": _HANDLE, "gmmiv_gmm_set_cov": _HANDLE, "gmmiv_gmm_destroy": _HANDLE,
    "gmmiv_gmm_batch_create": _HANDLE, "gmmiv_gmm_batch_load": _HANDLE, "gmmiv_gmm_batch_load_cov": _HANDLE,
    "gmmiv_gmm_batch_destroy": _HANDLE, "gmmiv_gmm_batch_packed": _HANDLE,
    "gmmiv_em_acc_len": _PLAN, "gmmiv_tv_packed_len": _PLAN, "gmmiv_shard_range": _PLAN, "gmmiv_energy_stage_frames": _PLAN,
    "gmmiv_plan_model_tiles": _PLAN, "gmmiv_plan_feat_tiles": _PLAN, "gmmiv_plan_trial_tiles": _PLAN, "gmmiv_trial_piece": _PLAN,
    "gmmiv_score_list_class": _PLAN, "gmmiv_plan_score_lists": _PLAN, "gmmiv_iv_trial_piece": _PLAN, "gmmiv_iv_trial_anchor": _PLAN,
    "gmmiv_plan_iv_trial_tiles": _PLAN, "gmmiv_turn_tile_positions": _PLAN, "gmmiv_plan_turn_positions": _PLAN,
    "gmmiv_comm_get_unique_id": _COMM, "gmmiv_comm_get_unique_id_for": _COMM, "gmmiv_comm_exchange_id_file": _COMM,
    "gmmiv_comm_create": _COMM, "gmmiv_comm_destroy": _COMM, "gmmiv_comm_world": _COMM, "gmmiv_comm_rank": _COMM,
    "gmmiv_comm_backend": _COMM, "gmmiv_comm_info": _COMM, "gmmiv_comm_take_bytes": _COMM, "gmmiv_allreduce_f64": _COMM,
    "gmmiv_reduce_scatter_f64": _COMM, "gmmiv_allgather_f64": _COMM, "gmmiv_broadcast_f64": _COMM, "gmmiv_allreduce_f64_begin": _COMM,
    "gmmiv_reduce_scatter_f64_begin": _COMM, "gmmiv_allgather_f64_begin": _COMM, "gmmiv_comm_join": _COMM,
}


def test_every_abi_function_is_judged_or_exempt():
    f = set(abi_functions())
    assert len(f) > 100
    unknown = (set(JUDGED) | set(EXEMPT)) - f
    assert not unknown, "named here but in no header: %s" % sorted(unknown)
    both = set(JUDGED) & set(EXEMPT)
    assert not both, "judged AND exempt: %s" % sorted(both)
    missing = f - set(JUDGED) - set(EXEMPT)
    assert not missing, "ABI functions that no module judges per element and EXEMPT does not name: %s" % sorted(missing)
    for name, reason in EXEMPT.items():
        assert reason in EXEMPT_REASONS, (name, reason)
    # an exemption is never a function that hands numbers computed on the device back to the caller by pointer
    abi = abi_functions()
    for name, reason in EXEMPT.items():
        if reason in (_CTX, _PLAN):
            assert not re.search(r"(?<!const )\bdouble\s*\*", abi[name]), "%s writes doubles and is exempt as %r" % (name, reason)


def test_the_named_module_calls_the_binding_of_the_function():
    calls = binding_calls()
    bad = []
    for name, (module, method) in sorted(JUDGED.items()):
        path = os.path.join(ROOT, "tests", module + ".py")
        if not os.path.exists(path):
            bad.append("%s: no module %s" % (name, module))
            continue
        if name not in calls.get(method, ()):
            bad.append("%s: capi.%s does not call it" % (name, method))
        src = open(path).read()
        if not re.search(r"\.%s\b" % re.escape(method), src):
            bad.append("%s: %s never mentions .%s" % (name, module, method))
        if "pytest.mark.gpu" not in src:
            bad.append("%s: %s is not a GPU module" % (name, module))
    assert not bad, "\n".join(bad)
