"""Per-system errors of the batched Cholesky family (chol_fused.hip, the GEMM-built path of tv_kernels.hip) on every shipped
variant, against the 80-bit reference of tests/spd_ref.py, next to the double-precision oracle's errors on the same systems.
tests/test_gpu_chol_family.py asserts on the records this module produces; run as a program it writes them to
profiles/r11/chol_family_errors.json with the sha256 of the library they were measured on.

    python tools/chol_family_errors.py [out.json]

A record: order, variant, entry ("estimate_w/W", "estimate_a_and_c/W|A|Rm", "update_t/D=..,mstep=.."), and per system (per
Gaussian and 16-column block for update_t) cond, err_oracle, err_gpu, eta_oracle, eta_gpu (eta: solves only).
"""
import contextlib
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import spd_ref  # noqa: E402

ORDERS = (2, 34, 130, 258, 492, 494, 496, 530, 33, 131)
LADDER_ORDERS = (494, 496)
MSTEP_ORDERS = (34, 130, 494, 496, 131)
DEFAULTS = {"chol_flow": 1, "chol_lds": 1, "chol_waves": 8, "chol_gemm": 0, "tv_mstep_solve": 1, "tv_batch": 1024, "tv_acc_mb": 8192}
LAST_LDS_ORDER = 494         # chol_lds(n) of chol_fused.hip: 32 (n & 2 ? n : n + 2) 8 + 36 KB <= 160 KB


def variants(n):
    """(name, {option: value}) that apply at order n."""
    v = [("defaults", {})]
    if n <= LAST_LDS_ORDER:
        v += [("chol_flow 0", {"chol_flow": 0}), ("chol_lds 0", {"chol_lds": 0}), ("chol_waves 16", {"chol_waves": 16})]
    if n % 2 == 0 and n <= 258:
        v.append(("chol_gemm 1", {"chol_gemm": 1}))
    return v


@contextlib.contextmanager
def options(ctx, opts):
    """Set, run, restore; set_option must hand back the value that was there (the default going in, ours coming out)."""
    try:
        for k, val in opts.items():
            prev = ctx.set_option(k, val)
            assert prev == DEFAULTS[k], "option %s was %r, expected the default %r" % (k, prev, DEFAULTS[k])
        yield
    finally:
        for k, val in opts.items():
            back = ctx.set_option(k, DEFAULTS[k])
            assert back == val, "option %s read back %r after it was set to %r" % (k, back, val)


def _f(x):
    return None if x is None else float("%.4e" % x)


def _records(order, variant, conds, err_o, err_g, eta_o, eta_g):
    out = []
    for entry in err_g:
        n = len(err_g[entry])
        out.append(dict(order=order, variant=variant, entry=entry, cond=list(conds)[:n] if n > 1 else None,
                        err_oracle=[_f(e) for e in err_o[entry]], err_gpu=[_f(e) for e in err_g[entry]],
                        eta_oracle=[_f(e) for e in eta_o[entry]] if entry in eta_o else None,
                        eta_gpu=[_f(e) for e in eta_g[entry]] if entry in eta_g else None))
    return out


def estep_records(ctx, batch, variant, opts, tag=""):
    with options(ctx, opts):
        err, eta, raw = spd_ref.run_batch(ctx, batch)
    return _records(batch.n, variant + tag, batch.conds, batch.err_oracle, err, batch.eta_oracle, eta), raw


# order 130 a second time: seven distinct systems in batches of three, E_u flushed per batch (tv_acc_mb 0: super-batches 3 + 3 + 1)
SEVEN_CONDS = (1e1, 1e3, 1e6, 1e3, 1e2, 1e5, 1e4)
SEVEN_OCCS = (1.0, 2.0, 4.0, 0.5, 8.0, 0.25, 16.0)
SEVEN_OPTS = {"tv_batch": 3, "tv_acc_mb": 0}


def mstep_records(ctx, m, D, mstep):
    """tv_update_t on the first D columns of every Gaussian's block, tv_mstep_solve = mstep -> (records, T)."""
    with options(ctx, {"tv_mstep_solve": mstep} if mstep != DEFAULTS["tv_mstep_solve"] else {}):
        T = ctx.tv_update_t(m.A_packed, m.cmx(D), m.C, D)
    eo, ho = m.oracle_errors(D)
    eg, hg = m.errors(T, D), m.etas(T, D)
    entry = "update_t/D=%d,mstep=%d" % (D, mstep)
    rec = dict(order=m.R, variant="defaults", entry=entry, cond=[m.conds[c] for c, _, _ in m.blocks(D)],
               err_oracle=[_f(e) for e in eo], err_gpu=[_f(e) for e in eg], eta_oracle=[_f(e) for e in ho], eta_gpu=[_f(e) for e in hg])
    return [rec], T


def failures(records):
    """Every system of every record that misses the bar of spd_ref.accept; prints each figure first."""
    bad = []
    for r in records:
        for i, (eg, eo) in enumerate(zip(r["err_gpu"], r["err_oracle"])):
            line = "order %d, %s, %s, system %d: err_gpu %.3e err_oracle %.3e bar %.3e" % (r["order"], r["variant"], r["entry"], i, eg, eo, spd_ref.bar(eo))
            if r["eta_gpu"]:
                line += "  eta_gpu %.2e eta_oracle %.2e" % (r["eta_gpu"][i], r["eta_oracle"][i])
            print(line)
            if not spd_ref.accept(eg, eo):
                bad.append(line)
    return bad


def all_records(ctx, log=print):
    recs = []
    for n in ORDERS:
        t = time.time()
        b = spd_ref.Batch(n)
        for name, opts in variants(n):
            recs += estep_records(ctx, b, name, opts)[0]
        if n == 130:
            b7 = spd_ref.Batch(n, SEVEN_CONDS, SEVEN_OCCS, seed=1)
            for name, opts in variants(n):
                recs += estep_records(ctx, b7, name, dict(opts, **SEVEN_OPTS), tag=", U=7 tv_batch 3")[0]
        log("order %d: %.1f s" % (n, time.time() - t))
    for n in LADDER_ORDERS:
        b = spd_ref.Batch(n, (1e8, 1e8), (1.0, 2.0), seed=8)
        recs += estep_records(ctx, b, "defaults", {}, tag=", ladder")[0]
    for R in MSTEP_ORDERS:
        m = spd_ref.MStep(R)
        for D in spd_ref.MSTEP_D:
            for ms in (1, 0):
                recs += mstep_records(ctx, m, D, ms)[0]
        log("update_t order %d done" % R)
    return recs


def worst_ratios(recs):
    """Per variant (update_t: per route): the worst err_gpu / max(err_oracle, 64 u) and the worst eta_gpu / eta_oracle, and where; the
    worst eta ratio per order as well."""
    out = {}
    for r in recs:
        key = r["variant"].split(",")[0] if not r["entry"].startswith("update_t") else "update_t " + r["entry"].split(",")[1]
        o = out.setdefault(key, dict(err_ratio=0.0, err_at=None, eta_ratio=0.0, eta_at=None, eta_gpu_max=0.0, eta_ratio_by_order={}))
        for i, (eg, eo) in enumerate(zip(r["err_gpu"], r["err_oracle"])):
            q = eg / max(eo, 64 * spd_ref.U_DOUBLE)
            if q > o["err_ratio"]:
                o["err_ratio"], o["err_at"] = _f(q), "order %d %s system %d" % (r["order"], r["entry"], i)
        if r["eta_gpu"]:
            for i, (hg, ho) in enumerate(zip(r["eta_gpu"], r["eta_oracle"])):
                o["eta_gpu_max"] = max(o["eta_gpu_max"], hg)
                by = o["eta_ratio_by_order"]
                by[str(r["order"])] = max(by.get(str(r["order"]), 0.0), _f(hg / ho))
                if hg / ho > o["eta_ratio"]:
                    o["eta_ratio"], o["eta_at"] = _f(hg / ho), "order %d %s system %d" % (r["order"], r["entry"], i)
    return out


def main():
    from lia_ral_amd import capi
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11", "chol_family_errors.json")
    if not spd_ref.HAVE_LONGDOUBLE:
        sys.exit(spd_ref.SKIP_MESSAGE)
    sha = hashlib.sha256(open(capi.LIB_PATH, "rb").read()).hexdigest()
    ctx = capi.Context(0)
    t = time.time()
    recs = all_records(ctx)
    ctx.close()
    bad = failures(recs)
    doc = {"_comment": "tools/chol_family_errors.py: per-system errors of the batched Cholesky family against the 80-bit reference of "
                       "tests/spd_ref.py; err_* = forward (W, update_t) / Frobenius (A, Rm) relative errors, eta = normwise backward error "
                       "of the solves; bar: err_gpu <= 16 max(err_oracle, 64 * 2^-53).",
           "libgmmiv_sha256": sha, "wall_s": round(time.time() - t, 1), "systems_over_the_bar": bad,
           "worst_ratios": worst_ratios(recs), "records": recs}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("{\n")
        for k in ("_comment", "libgmmiv_sha256", "wall_s", "systems_over_the_bar", "worst_ratios"):
            f.write(" %s: %s,\n" % (json.dumps(k), json.dumps(doc[k], indent=1 if k == "worst_ratios" else None)))
        f.write(' "records": [\n' + ",\n".join("  " + json.dumps(r) for r in recs) + "\n ]\n}\n")
    print(json.dumps(doc["worst_ratios"], indent=1))
    print("%d records, %d systems over the bar, %.1f s -> %s" % (len(recs), len(bad), doc["wall_s"], out))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
