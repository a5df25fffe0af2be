"""What tests/test_gpu_ws_history.py relies on, checked without a GPU: the large cases dominate the judged ones in every quantity
that sizes a workspace -- those of the i-vector back end included -- and do not align with them; every judged back-end shape is a row
of its reference module's own table; the degenerate frames are where the table says; the run tables of windowed NormFeat and
TurnDetection are valid and hold the runs they are there for; and the programme reaches every function of every header under
include/ (gmmiv.h, gmmiv_feat_window.h, gmmiv_iv_trials.h, gmmiv_turn.h today; HEADERS lists the directory, so a new header is read
too) that takes a context, model or batch handle -- or names it in EXEMPT with a reason -- so a new ABI function with neither
fails here."""
import ast
import inspect
import os
import re

import numpy as np

import backend_ref as br
import estimation_ref as es
import tv_ref as tr
import ws_history as wh
from conftest import ROOT


def test_every_judged_case_is_dominated_by_a_large_case_that_does_not_align_with_it():
    for small in wh.SMALL:
        s = wh.sizes(small)
        found = []
        for large in wh.LARGE:
            l = wh.sizes(large)
            if all(l[k] >= s[k] for k in s):
                Cs, Ds, Ts, _ = small["gcase"]
                Cl, Dl, Tl, _ = large["gcase"]
                if Cl % Cs or Dl % Ds or Tl % Ts:
                    found.append(large["name"])
        assert found, "no large case dominates %s: %s" % (small["name"], s)
    # the segment, trial and file tables, which size the WS_MB_* / WS_TR_* / WS_NORM_* slots, and the energy / score inputs
    for small in wh.SMALL:
        for large in wh.LARGE:
            assert len(wh.seg_table(large)[1]) >= len(wh.seg_table(small)[1]) and len(wh.trial_table(large)[0]) >= len(wh.trial_table(small)[0])
            assert max(np.diff(wh.file_table(large))) >= max(np.diff(wh.file_table(small)))
            assert sum(large["energy"]) >= sum(small["energy"]) and sum(large["lists"]) >= sum(small["lists"])
            # windowed NormFeat and TurnDetection: every quantity of run_sizes, and no chain of a judged case can fill more segments
            # than the dirtying tables have runs (a run yields at least one)
            ls, ss = wh.run_sizes(large), wh.run_sizes(small)
            assert set(ls) == set(ss) == {"nrun", "npos", "nsteps", "nrun_D", "seg_room"} <= set(wh.sizes(small))
            assert all(ls[k] >= ss[k] for k in ss), (large["name"], small["name"], ls, ss)
            assert large["nfiles"] >= small["nfiles"] and ls["nrun"] >= ss["nrun"] + ss["npos"]
            assert ls["nrun"] % ss["nrun"] and ls["npos"] % ss["npos"]                      # the run and position counts are no multiples
    files = lambda c: np.bincount(wh.run_table(c)[0][:, 2], minlength=c["nfiles"])
    assert max(wh.run_sizes(c)["nrun"] for c in wh.LARGE) > 2 * 1024                        # k_turn_tiles: three chunks of 1024 runs
    assert max(files(c).max() for c in wh.LARGE) > 2 * 256                                  # k_turn_segments: a file of more than two strides of 256
    assert all(c["plant"] for c in wh.LARGE)                                                # non-finite frames: neither family screens them
    assert max(c["gcase"][2] for c in wh.LARGE) > 4096 and wh.Z_MB_530 >= 1              # more than one chunk of the smallest scratch
    assert max(np.diff(wh.file_table(wh.LARGE[0]))) >= 2500 > 2 * 1024                     # the online scan: more than two chunks
    assert all(c["cohort"] == 100003 for c in wh.LARGE)
    # the online scan with a device table is sized by the allocation that holds x (ws_history.s_norm_online)
    most = max(wh.TORCH_SMALL_BLOCK // (4 * c["gcase"][1]) + 1 for c in wh.SMALL)
    assert all(c["online_rows"] >= most and c["online_rows"] * c["gcase"][1] * 4 > wh.TORCH_SMALL_BLOCK for c in wh.LARGE)
    assert max(c["online_rows"] * c["gcase"][1] for c in wh.LARGE) >= max((wh.TORCH_SMALL_BLOCK // (4 * c["gcase"][1]) + 2048) * c["gcase"][1] for c in wh.SMALL)
    assert {c["gcase"][:3] for c in wh.SMALL} == {(37, 13, 65), (129, 60, 257), (40, 97, 66)}
    assert 70 in wh.CASES["s129x60x257"]["ctops"] and {10, 17} <= set(wh.SMALL[0]["ctops"])


def test_the_dirtying_back_end_shapes_dominate_the_judged_ones_and_do_not_align_with_them():
    """every large case on its own, in every quantity of iv_sizes -- a judged slot request that a dirtying one does not cover would be
    handed out fresh (and cleared) in the small pass; and no dirtying set is the judged one scaled: of the quantities that give a
    buffer its row length, none is a multiple of the judged value in at least one dirtying case"""
    strides = ("tv_CD", "tv_R", "tv_P", "tv_U", "score_dim", "score_M", "score_S", "ivn_in", "ivn_n", "dev_dim", "dev_sessions", "plda_dim", "eig",
               "ortho_SV", "jfa_CD", "jfa_sessions", "em_sessions", "gemm_N")
    aligned = {}
    for large in wh.LARGE:
        l = wh.iv_sizes(large)
        assert set(strides) <= set(l)
        for small in wh.SMALL:
            s = wh.iv_sizes(small)
            assert set(s) == set(l)
            short = {k: (s[k], l[k]) for k in s if l[k] < s[k]}
            assert not short, "%s does not dominate %s: %s" % (large["name"], small["name"], short)
            aligned.setdefault(small["name"], []).append([k for k in strides if l[k] % s[k] == 0])
        # finite: the large pass stays a comparison of complete results; NaN enters through nan_calls alone
        for _, key, p in wh.chains(large):
            assert all(np.isfinite(v).all() for v in p.values() if isinstance(v, np.ndarray)), key
        assert np.isfinite(wh.dev_data(large)[0]).all() and all(np.isfinite(a).all() for a in wh.em_state(large, 0))
        assert all(np.isfinite(v).all() for v in wh.jfa_data(large).values() if isinstance(v, np.ndarray))
        M, S = large["iv"]["score"][1:]
        assert M % 2 and S % 2 and min(M, S) > 257 and l["dev_speakers"] > 257 and l["dev_longest"] > 600
    # some dirtying case aligns with the judged one in none of these -- but for the smallest judged set, whose 1, 2 and 3 (jfa C D = 3,
    # n = 7 vectors) divide too much to be avoided: two there
    assert [min(len(a) for a in aligned[c["name"]]) for c in wh.SMALL] == [2, 0, 0], aligned
    # one even and one odd rank, the first a row of tv_ref.ESTEP_CASES; the NaN calls run at the odd one and at dirtying sizes
    assert [c["iv"]["tv"][0][2] % 2 for c in wh.LARGE] == [0, 1]
    assert wh.LARGE[0]["iv"]["tv"][0] in {c[:3] + (u,) for c in tr.ESTEP_CASES for u in c[3]}
    assert wh.NAN_TV == wh.LARGE[1]["iv"]["tv"][0] and wh.NAN_TV[2] % 2 and wh.NAN_DEV == wh.LARGE[1]["iv"]["dev"] and wh.NAN_DEV[0] % 2
    assert wh.NAN_IVN == wh.LARGE[1]["iv"]["ivn"] and wh.NAN_SCORE == wh.LARGE[1]["iv"]["score"] and wh.NAN_EM == wh.LARGE[1]["iv"]["em"][0]
    j = wh.jfa_data(wh.LARGE[1])
    assert wh.NAN_JFA == (j["C"], j["D"], j["R"], j["nspk"], j["nsess"]) and all(n % 2 for n in wh.NAN_SCORE + wh.NAN_IVN)


def test_every_judged_back_end_shape_is_a_row_of_its_reference_table():
    estep = {c[:3] + (u,) for c in tr.ESTEP_CASES for u in c[3]}
    scores = {(d,) + c for d in br.SCORE_DIMS for c in br.SCORE_COUNTS}
    want = dict(tv=[((5, 3, 2, 7),), ((8, 12, 35, 20),), ((16, 12, 40, 75), (6, 4, 70, 65))], dev=["3x[1,2,1]", "33x257", "8x[600,1,2]"],
                plda=[(5, 2, 1), (33, 7, 3), (34, 5, 5)], score=[(5, 3, 7), (33, 33, 31), (130, 131, 129)], ivn=[(5, 3, 7), (60, 40, 33), (33, 33, 130)],
                jfa=[(3, 1, 1), (6, 5, 3), (5, 13, 7)], eig=[2, 33, 65])
    for k, rows in want.items():
        assert [c["iv"][k] for c in wh.SMALL] == rows, k
    for case in wh.SMALL:
        iv = case["iv"]
        assert set(iv["tv"]) <= estep and iv["dev"] in br.DEV_CASES and iv["dev"] in es.DEV_SETS and iv["plda"] in es.PRECOMPUTE_CASES
        assert iv["score"] in scores and iv["ivn"] in br.IVN_SHAPES and iv["jfa"] in br.JFA_SHAPES and iv["eig"] in es.EIGEN_ORDERS
        assert ("spd", iv["eig"], wh.EIG_COND) in es.eigen_matrices() and ("spd", iv["eig"], wh.EIG_COND) in es.lda_matrices()
        assert (iv["eig"], wh.EIG_COND) in es.TWOCOV_CASES and set(iv["ortho"]) <= set(es.ORTHO_CASES) and set(iv["em"]) <= set(es.EM_CASES)
        assert all(k[:2] in es.ORTHO_SHAPES for k in iv["ortho"])
        for name in iv["em"]:                                                               # of matching size: the PLDA shape or the development set
            dim, rf, rg, sps = es.EM_CASES[name]
            assert (dim, rf, rg) == iv["plda"] or name.split()[-1] == iv["dev"].split("x")[-1], name
    assert [c["iv"]["ortho"][0][:2] for c in wh.SMALL] == [(2, 3), (33, 520), (24, 1000)]
    # both routes of tv_orthonormalize_t, told from the 80-bit factor
    routes = [es.ortho_route(k) for k in wh.SMALL[2]["iv"]["ortho"]]
    assert routes == ["gram", "step"] and wh.SMALL[2]["iv"]["ortho"][1][2] in es.ORTHO_RATIOS
    assert all([es.ortho_route(k) for k in c["iv"]["ortho"]] == ["gram", "step"] for c in wh.LARGE)


def test_both_spd_routes_the_short_batches_and_the_pad_copies_are_in_the_judged_table():
    """the timer names no kernel of SpdBatch, so the route is told from the order: even orders take the left-looking kernels, odd ones
    (and every order under chol_gemm 1) unpack and take the GEMM-built factorisation (capi_tv_util.h)"""
    ranks = [t[2] for c in wh.SMALL for t in c["iv"]["tv"]]
    assert 35 in ranks and 70 in ranks and 70 % 32 and any(r % 2 == 0 and r < 32 for r in ranks)
    assert {c["iv"]["eig"] % 2 for c in wh.SMALL} == {0, 1} and {c["iv"]["plda"][0] % 2 for c in wh.SMALL} == {0, 1}
    opts = {s.name: s.opts for s in wh.PROGRAMME}
    assert opts["tv e-step [tv_batch 16 tv_acc_mb 0]"] == {"tv_batch": 16, "tv_acc_mb": 0} and opts["tv e-step [chol_gemm 1]"] == {"chol_gemm": 1}
    assert opts["tv tett [tv_tett_direct 0]"] == {"tv_tett_direct": 0} and opts["tv update_t [tv_mstep_solve 0]"] == {"tv_mstep_solve": 0}
    assert opts["tv min_divergence [tv_md_device 0]"] == {"tv_md_device": 0} and opts["dgemm split-K [gemm_nt80 0]"] == {"gemm_nt80": 0}
    # (16, 12, 40, 75) in two calls of 37 + 38 utterances under tv_batch 16: 16 + 16 + 5 and 16 + 16 + 6; (6, 4, 70, 65) crosses 64 utterances
    assert (16, 12, 40, 75) in wh.SMALL[2]["iv"]["tv"] and 75 // 2 % wh.TV_BATCH and (75 - 75 // 2) % wh.TV_BATCH
    assert any(t[3] > 64 > t[3] // 2 for t in wh.SMALL[2]["iv"]["tv"])
    assert wh.estep_batches(wh.LARGE[0], wh.TV_BATCH) == [4, 5] and wh.estep_batches(wh.LARGE[0], 1024) == [1, 1]
    # odd counts on both sides: ScoreArgs::even_stride copies both matrices; the PLDA runs of odd length are gathered with a pad
    for c in wh.SMALL[1:]:
        dim, M, S = c["iv"]["score"]
        assert M % 2 and S % 2
        runs = np.diff(np.flatnonzero(np.diff(np.r_[-1, wh.score_data(c)["nsess"], -1])))
        assert (runs % 2).any()
    # the split-K product: layers of 48 and a short last one; two shapes take the 128 x 80 tile unless "gemm_nt80" is 0
    for c in wh.SMALL + wh.LARGE:
        M, N, K, nz = c["iv"]["gemm"]
        kc = ((K + nz - 1) // nz + 15) // 16 * 16
        assert kc == 48 and (K + kc - 1) // kc == nz >= 3 and 0 < K % kc < kc
    nt80 = [c["name"] for c in wh.SMALL + wh.LARGE if c["iv"]["gemm"][0] % 128 == 0 and c["iv"]["gemm"][1] % 80 == 0 and c["iv"]["gemm"][1] % 128
            and c["iv"]["gemm"][2] % 16 == 0]
    assert nt80 == ["s129x60x257", "L530x60x4300"]
    # FTJF B differs from A in one element, and stays a model
    for c in wh.SMALL:
        A, B = wh.ftjf_pair(c)
        assert (A != B).sum() == 1 and np.linalg.eigvalsh(B + np.eye(len(B))).min() > 0


def test_tables_are_valid_and_have_an_empty_segment():
    for case in wh.SMALL + wh.LARGE:
        T = case["gcase"][2]
        sb, sm = wh.seg_table(case)
        assert len(sb) == case["nseg"] + 1 and sb[0] >= 0 and sb[-1] <= T and np.all(np.diff(sb) >= 0) and (np.diff(sb) == 0).sum() == 1
        assert sm.min() >= 0 and sm.max() < case["G"] and len(set(sm.tolist())) == case["G"]
        ts, tm = wh.trial_table(case)
        assert len(ts) == case["ntrial"] and ts.max() < case["nseg"] and tm.max() < case["G"] and ts.min() >= 0 and tm.min() >= 0
        fb = wh.file_table(case)
        assert fb[-1] <= T and np.all(np.diff(fb) >= 0)
        assert all(c <= 64 for c in case["trial_ctops"])                                   # gmmiv_llr_trials: ctop <= 64
        check_run_tables(case)
    kinds = [run_kinds(c) for c in wh.SMALL]
    assert all({0, 1} <= set(k["positions"]) and k["short"] and k["empty_files"] for k in kinds), kinds
    assert any(k["P + 1"] for k in kinds), "no judged case holds a run of P + 1 positions"
    assert wh.SMALL[0]["nseg"] == 5 and wh.SMALL[0]["G"] == 3 and wh.SMALL[0]["ntrial"] == 6
    assert wh.LARGE[0]["nseg"] == 40 and wh.LARGE[0]["G"] == 7 and wh.LARGE[0]["ntrial"] == 60


def check_run_tables(case):
    """the run table of the two new steps: accepted by both planners, inside the files of file_table, and turn_table's CSR, decisions
    and room are what turn_ref says"""
    from lia_ral_amd import capi
    import turn_ref as tn
    T, nf, W, S = case["gcase"][2], case["nfiles"], wh.TURN_W, wh.TURN_S
    runs, first = wh.run_table(case)
    fb = wh.file_table(case)
    assert runs.dtype == np.int64 and runs.shape[1] == 3 and np.array_equal(first, fb[:-1])
    assert np.all(np.diff(runs[:, 2]) >= 0) and runs[:, 2].min() >= 0 and runs[:, 2].max() < nf
    assert np.all(runs[:, 1] >= 1) and np.all(runs[:, 0] >= fb[runs[:, 2]]) and np.all(runs[:, 0] + runs[:, 1] <= fb[runs[:, 2] + 1]) and fb[-1] <= T
    assert np.all(runs[1:, 0] >= runs[:-1, 0] + runs[:-1, 1])                               # no overlap, begins strictly increasing
    assert (np.bincount(runs[:, 2], minlength=nf) == 0).sum() == 1                          # a file without runs
    off, st, al = capi.plan_norm_windows(runs, nf, first, *wh.NORMWIN)                      # the planner accepts the table ...
    ref = wh._window_plan(case["name"])                                                     # ... and sizes() counts its steps
    assert np.array_equal(off, ref[0]) and np.array_equal(st, ref[1]) and len(al) == len(ref[2]) == wh.run_sizes(case)["nsteps"] > 0
    t = wh.turn_table(case)
    po = capi.plan_turn_positions(runs, nf, W, S)
    want = [tn.positions_as_written(int(L), W, S) for L in runs[:, 1]]
    assert np.array_equal(po, t["pos_off"]) and list(np.diff(po)) == want and po[-1] == wh.run_sizes(case)["npos"]
    assert capi.turn_tile_positions(wh.turn_cols(case), W, S) == case["runs"]["P"] >= 2
    npos = int(po[-1])
    assert t["curve"].shape == (npos,) and np.isnan(t["curve"]).sum() == 1 and not (t["curve"] == -0.5).any()
    assert np.array_equal(t["curve"][np.isfinite(t["curve"])], np.round(t["curve"][np.isfinite(t["curve"])]))
    assert t["dec"].shape == (npos,) and t["dec"].dtype == np.uint8 and 0 < t["dec"].sum() < npos
    room = np.diff(t["seg_off"])
    assert t["seg_off"][0] == 0 and list(room - t["seg_count"]) == [-2] + [0] * (nf - 2) + [3] and t["seg_count"].sum() >= len(runs)


def run_kinds(case):
    runs, _ = wh.run_table(case)
    t = wh.turn_table(case)
    n = np.diff(t["pos_off"])
    return {"positions": sorted(set(n.tolist())), "short": bool((runs[:, 1] <= 2 * wh.TURN_W).any()), "P + 1": bool((n == case["runs"]["P"] + 1).any()),
            "empty_files": int((np.bincount(runs[:, 2], minlength=case["nfiles"]) == 0).sum())}


def test_the_planted_frames_are_where_the_table_says_and_the_large_host_frames_are_float64():
    for case in wh.LARGE:
        C, D, T, _ = case["gcase"]
        k1, k2 = wh.planted(case)
        assert len(k1) == 8 and len(k2) == 2
        rows = sorted(list(k1) + list(k2))
        assert sum(1 for t in rows if t >= T - 16) >= 4 and sum(1 for t in rows if t < 16) >= 4          # the last 16 rows, the first block
        for form, dtype in (("host", np.float64), ("device", np.float32)):
            x = wh.frames(case, form)
            assert x.dtype == dtype and x.shape == (T, D) and not x.flags.writeable
            bad = ~(np.isfinite(x) & (np.abs(x) <= 1e18)).all(1)
            assert sorted(np.nonzero(bad)[0].tolist()) == sorted(k1)
            for t, v in k1.items():
                col = (7 * t) % D
                assert (np.isnan(x[t, col]) if np.isnan(v) else x[t, col] == dtype(v)) and np.isfinite(np.delete(x[t], col)).all()
            assert {np.inf, -np.inf, 1e30} <= set(k1.values()) and any(np.isnan(v) for v in k1.values())
            for t in k2:
                assert np.all(x[t] == dtype(wh.FAR_VALUE))
            # kind 2: the largest logit of a far frame lies below GMMIV_ZERO_LLK by a wide margin
            w, mean, iv = wh.gr.model(case["gcase"])
            z = np.log(w) + 0.5 * np.log(iv).sum(1) - 0.5 * D * np.log(2 * np.pi) - 0.5 * (((x[k2[0]].astype(np.float64) - mean) ** 2) * iv).sum(1)
            assert z.max() < 10 * wh.gr.ZERO_LLK
    for case in wh.SMALL:
        assert wh.planted(case) == ({}, ()) and np.isfinite(wh.frames(case, "host")).all()


# ---------------------------------------------------------------------------------------------------------------- coverage
HANDLE = re.compile(r"\bgmmiv_(ctx|gmm|gmm_batch)\s*\*")


HEADERS = tuple(sorted(h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h")))      # every header: a new one cannot stay outside
assert {"gmmiv.h", "gmmiv_feat_window.h", "gmmiv_iv_trials.h", "gmmiv_turn.h"} <= set(HEADERS), HEADERS


def abi_functions():
    """{name: argument text} of every function prototype of every header under include/"""
    src = "\n".join(open(os.path.join(ROOT, "include", h)).read() for h in HEADERS)
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = "\n".join(l for l in src.split("\n") if not l.lstrip().startswith("#"))
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(gmmiv_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", src)}


def binding_calls():
    """capi.py by source: {function or method name: the lib.gmmiv_* calls in its body}, following self.method() one level"""
    src = open(os.path.join(ROOT, "lia_ral_amd", "capi.py")).read()
    tree = ast.parse(src)
    direct, inner = {}, {}
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef):
            libs, calls = set(), set()
            for n in ast.walk(node):
                if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == "lib" and n.attr.startswith("gmmiv_"):
                    libs.add(n.attr)
                if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute) and isinstance(n.func.value, ast.Name) and n.func.value.id == "self":
                    calls.add(n.func.attr)
                if isinstance(n, ast.Call) and isinstance(n.func, ast.Name):
                    calls.add(n.func.id)
            direct.setdefault(node.name, set()).update(libs)
            inner.setdefault(node.name, set()).update(calls)
    return {name: libs.union(*[direct.get(c, set()) for c in inner[name]]) for name, libs in direct.items()}


def source_of(fn, seen=None):
    """the source of a step function and of the module-level helpers of ws_history it names"""
    seen = set() if seen is None else seen
    if fn in seen:
        return ""
    seen.add(fn)
    text = inspect.getsource(fn)
    for name in fn.__code__.co_names:
        g = getattr(wh, name, None)
        if inspect.isfunction(g) and g.__module__ == wh.__name__:
            text += source_of(g, seen)
        elif inspect.isclass(g) and g.__module__ == wh.__name__:
            text += inspect.getsource(g)
    return text


def test_the_abi_is_parsed():
    f = abi_functions()
    assert len(f) > 100 and "gmmiv_llk" in f and "gmmiv_ctx_stream" in f and "gmmiv_llr_trials" in f
    assert {"gmmiv_score_cosine_trials", "gmmiv_score_mahalanobis_trials", "gmmiv_score_twocov_trials", "gmmiv_score_plda_trials"} <= set(f)
    assert HANDLE.search(f["gmmiv_score_plda_trials"]) and HANDLE.search(f["gmmiv_iv_trial_piece"]) and not HANDLE.search(f["gmmiv_plan_iv_trial_tiles"])
    assert HANDLE.search(f["gmmiv_llk"]) and not HANDLE.search(f["gmmiv_em_acc_len"]) and not HANDLE.search(f["gmmiv_allreduce_f64"])
    new = {"gmmiv_plan_norm_windows", "gmmiv_feat_norm_window", "gmmiv_turn_tile_positions", "gmmiv_plan_turn_positions", "gmmiv_turn_curve",
           "gmmiv_turn_pick", "gmmiv_turn_segments"}
    assert new <= set(f) and {n for n in new if HANDLE.search(f[n])} == {"gmmiv_feat_norm_window", "gmmiv_turn_curve", "gmmiv_turn_pick", "gmmiv_turn_segments"}
    assert len(HEADERS) >= 4 and list(HEADERS) == sorted(HEADERS)


def test_every_abi_function_with_a_handle_is_reached_or_exempt():
    f = abi_functions()
    subject = {n for n, args in f.items() if HANDLE.search(args)}
    reached = {e for s in wh.PROGRAMME for e in s.reaches} | set(wh.PLUMBING) | set(wh.HANDLE_TESTS)
    unknown = (reached | set(wh.EXEMPT)) - set(f)
    assert not unknown, "named by the programme but in neither header: %s" % sorted(unknown)
    both = reached & set(wh.EXEMPT)
    assert not both, "reached AND exempt: %s" % sorted(both)
    missing = subject - reached - set(wh.EXEMPT)
    assert not missing, "ABI functions with a handle that no step reaches and EXEMPT does not name: %s" % sorted(missing)
    for name, reason in wh.EXEMPT.items():
        assert reason in wh.EXEMPT_REASONS, (name, reason)
    # the i-vector back end is IN the programme: only functions without a workspace and the communicator stay outside
    assert set(wh.EXEMPT_REASONS) == {wh._NO_WS, wh._COMM}
    back_end = {n for n in subject if re.match(r"gmmiv_(tv|jfa|dev|score|plda|twocov|sym_eigen|iv_normalize)", n)}
    assert len(back_end) >= 45 and back_end <= {e for s in wh.PROGRAMME for e in s.reaches}, sorted(back_end - {e for s in wh.PROGRAMME for e in s.reaches})
    # "no workspace" is checked: the body of such a function holds no scratch( and no DevIn / DevOut
    csrc = os.path.join(ROOT, "lia_ral_amd", "csrc")
    text = "".join(open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".cpp")))
    for name, reason in wh.EXEMPT.items():
        if reason != wh._NO_WS:
            continue
        m = re.search(r"\b%s\s*\([^;{)]*\)\s*\{" % name, text)
        assert m, "no definition of %s found" % name
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[i], 0)
            i += 1
        body = text[m.end():i]
        assert "scratch(" not in body and "DevIn" not in body and "DevOut" not in body, name


def test_every_step_calls_the_bindings_of_the_entry_points_it_names():
    calls = binding_calls()
    wrappers = {}                                   # C entry point -> the binding functions that call it
    for fn, libs in calls.items():
        for l in libs:
            wrappers.setdefault(l, set()).add(fn)
    for step in wh.PROGRAMME:
        text = source_of(step.fn)
        assert step.reaches, step.name
        for entry in step.reaches:
            assert entry in wrappers, "%s: capi.py has no lib.%s call" % (step.name, entry)
            assert any(re.search(r"\.%s\(" % w, text) for w in wrappers[entry]), \
                "step %r names %s but calls none of its bindings %s" % (step.name, entry, sorted(wrappers[entry]))
    plumbing = "".join(inspect.getsource(o) for o in (wh.Handles, wh.Step, wh.nan_calls, wh.workspace_table, wh.run_sequence, wh.counters, wh.s_em, wh.s_tv))
    for entry in wh.PLUMBING:
        names = {"__init__": {"Context", "gmm", "gmm_batch"}, "__del__": {"close"}}
        ws = set().union(*[names.get(w, {w}) for w in wrappers[entry]])
        assert any(re.search(r"\b%s\(" % w, plumbing) for w in ws), (entry, sorted(ws))
    gpu_test = open(os.path.join(ROOT, "tests", "test_gpu_ws_history.py")).read()
    for entry, method in wh.HANDLE_TESTS.items():
        assert method in wrappers[entry] and re.search(r"\.%s\(" % method, gpu_test), entry


def test_step_names_are_unique_and_both_forms_exist():
    names = [s.name for s in wh.PROGRAMME]
    assert len(names) == len(set(names)) and set(wh.STEPS) == set(names)
    for s in wh.PROGRAMME:
        assert s.forms == wh.FORMS, "%s: every binding this step calls accepts device tensors, so both forms run" % s.name
        assert "form" in inspect.signature(s.fn).parameters
        assert any(s.applies(c) for c in wh.SMALL) and any(s.applies(c) for c in wh.LARGE)
    # the options of the programme have defaults in the shared bracket
    from elementwise_judge import DEFAULTS
    for s in wh.PROGRAMME:
        assert set(s.opts) <= set(DEFAULTS)
    for c in wh.SMALL + wh.LARGE:
        assert set(c["opts"]) <= set(DEFAULTS)
    # a sequence is a list of passes over SMALL or LARGE
    assert set(wh.SEQUENCES) >= {"fresh_small", "fresh_small_again", "fresh_large", "large_then_small", "large_then_small_reversed", "small_then_large"}
    assert [i[1].name for i in wh.plan(wh.SMALL, True)] == [i[1].name for i in wh.plan(wh.SMALL)][::-1]
