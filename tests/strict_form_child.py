"""Child process of tests/test_strict_two_solve_gpu.py: the engine reads HMOGP_STRICT_FORM once per process, so the
evaluations that force a form of the strict q(f) mode run here, with the switch set by the parent in this process's environment.

    python tests/strict_form_child.py <jobs.json> <out.npz>

jobs.json: a list of [case tag of tests/rowpass_cases.py, options]; options (all optional):
    engine      keyword arguments of Engine beside strict_qf=True (chunk_rows, ...): jobs with the same case and the same engine
                options share one engine, in the order given
    group_mask  name of a group mask of hetmogp_amd._lib
    row_begin, row_end   a row shard
    predict     false: q(f) through hmogp_predict_f is not read
    inject      path of a .npy float64 bundle written over the engine's own between hmogp_step_begin and hmogp_step_finish; the
                outputs of the tail (and hmogp_posterior_u) are stored instead of the bundle
Every evaluation is made twice.  out.npz: "<i>/<kind>" (lists per function: "<i>/m/<d>"), "<i>/same" (whether the two evaluations
agreed bit for bit in every stored array), "<i>/cond_est", "<i>/rungs"; "form" = the switch as this process saw it."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import rowpass_cases as rc  # noqa: E402
import rowpass_ref as rr  # noqa: E402

TAIL_OUT = ("g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z")


def evaluate(e, case, opt):
    """One evaluation -> {name: array}."""
    from hetmogp_amd import _lib
    prm, prob, X, Y, rungs = case
    T, Df = prob["T"], prob["Df"]
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"], forced_rung=rungs)
    if "group_mask" in opt:
        args["group_mask"] = getattr(_lib, opt["group_mask"])
    if "row_begin" in opt:
        args.update(row_begin=list(opt["row_begin"]), row_end=list(opt["row_end"]))
    got = {}
    e.step_begin(**args)
    if "inject" in opt:
        e.stats_write(np.load(opt["inject"]))
        out = e.step_finish(want_dL_dS=True)
        for k in TAIL_OUT:
            got[k] = np.array(out[k], dtype=np.float64, copy=True)
        got["elbo"], got["kl"], got["dL_dS"] = np.array([out["elbo"]]), np.array(out["kl"], copy=True), np.array(out["dL_dS"], copy=True)
        got["wv"], got["winv"] = e.posterior_u()
    else:
        stats = e.stats_read()
        out = e.step_finish()
        got.update(rr.split_bundle(stats, prob))
    assert out["rungs"] == rungs and not out["v_negative"], (out["rungs"], out["v_negative"])
    got["cond_est"], got["rungs"] = np.array(out["cond_est"], dtype=np.float64), np.array(out["rungs"])
    if opt.get("predict", True):
        b = opt.get("row_begin") or [0] * T
        en = opt.get("row_end") or [x.shape[0] for x in X]
        for t in range(T):
            m, v = e.predict_f(X[t][b[t]:en[t]])
            for d in range(Df):
                if prob["f_index"][d] == t:
                    got["m/%d" % d], got["v/%d" % d] = m[:, d].copy(), v[:, d].copy()
    return got


def main(jobs_path, out_path):
    from hetmogp_amd.engine import Engine
    with open(jobs_path) as f:
        jobs = json.load(f)
    out = {"form": np.array(os.environ.get("HMOGP_STRICT_FORM", ""))}
    engines, cases = {}, {}
    for i, (tag, opt) in enumerate(jobs):
        if tag not in cases:
            cases[tag] = rc.dense_case(tag)
        case = cases[tag]
        key = (tag, json.dumps(opt.get("engine", {}), sort_keys=True))
        if key not in engines:
            prob = case[1]
            engines[key] = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], strict_qf=True, **opt.get("engine", {}))
            engines[key].set_data(case[2], case[3])
        first, second = evaluate(engines[key], case, opt), evaluate(engines[key], case, opt)
        same = sorted(first) == sorted(second) and all(np.array_equal(first[k], second[k]) for k in first)
        out["%d/same" % i] = np.array(same)
        for k, a in first.items():
            out["%d/%s" % (i, k)] = np.asarray(a)
        print("[strict2] child job %d %s %s done, same bits %s" % (i, tag, json.dumps(opt, sort_keys=True), same), flush=True)
    for e in engines.values():
        e.close()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
