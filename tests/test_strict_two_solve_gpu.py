"""GPU: the TWO-SOLVE form of the strict q(f) mode, element by element.  The strict mode takes its one-solve form up to a
condition estimate of 1e6 and the two-solve form beyond; every dense case of 9c sits at rung 6 (estimate 1), so the two-solve code --
`trsm_panel_kernel<1, STATS>` with `st_K` (p = A m, rowsum(A .* K^) in the backward direction's epilogue, m_u read at stride Q),
`launch_trsm_stats_combine`, the `w3 == nullptr` branches of `strict_rowstats_kernel<P>`, T = A L_q and P~ = A (S K^-1 - I) against
L / D2, the Gram of A, `colstats_kernel<P, true, ...>` fed A, the `strict && strict_two` branch of the tail, `predict_f` after such an
evaluation -- is reached only by forcing the form with the documented switch HMOGP_STRICT_FORM=2.  The engine reads the switch once per
process: the forced evaluations run in ONE child process (tests/strict_form_child.py), started once per module, and are held here to

    |got - R| <= C_KERNEL[kind] * 2^-52 * S      per element, R, S of the case's `strict2` variant (tests/rowpass_ref.py, strict="two").

In this process, with no switch set: q(f) through hmogp_predict_f after a ONE-solve strict evaluation (D, G, H, J); case K, where the
engine picks the two-solve form by itself; and the form following the parameters, not the engine's history.
Every test prints its worst ratios as `[strict2] <case> <kind> ...`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import rowpass_cases as rc
import rowpass_ref as rr
import strict_form_child as sc

pytestmark = pytest.mark.gpu

MV = rr.BUNDLE_KINDS + ("m", "v")
# name -> (case, options of the child, variant of the reference, kinds)
JOBS = {
    "J": ("J", {}, "strict2", MV),
    "D one pool": ("D", {}, "strict2", MV),
    "D chunk_rows=300": ("D", {"engine": {"chunk_rows": 300}}, "strict2", MV),
    "D chunk_rows=1100": ("D", {"engine": {"chunk_rows": 1100}}, "strict2", MV),
    "D GROUP_QU": ("D", {"group_mask": "GROUP_QU", "predict": False}, "strict2", ("ve", "sgv", "H", "r")),
    "D row shard": ("D", {"row_begin": list(rc.D_SHARD[0]), "row_end": list(rc.D_SHARD[1])}, "strict2_shard", MV),
    "B": ("B", {}, "strict2", MV),
    "G": ("G", {}, "strict2", MV),
    "H": ("H", {}, "strict2", MV),
    "D tail": ("D", {"inject": None, "predict": False}, "strict2", None),
}
CHILD_TIMEOUT = 120          # seconds: ten engines' worth of HIP start-up and twenty small evaluations take about ten


@pytest.fixture(scope="module")
def refs():
    return rc.references()


@pytest.fixture(scope="module")
def child(refs, tmp_path_factory):
    """The child process, once: {job name: {kind: array(s)}}.  Any failure of the child raises here, for every dependent test; it is
    not started again."""
    import tail_cases as tc
    d = tmp_path_factory.mktemp("strict2")
    bundle = str(d / "bundle.npy")
    np.save(bundle, tc.dense_bundle(refs, "D", "strict2"))
    jobs = [[tag, dict(opt, inject=bundle) if "inject" in opt else opt] for tag, opt, _, _ in JOBS.values()]
    with open(str(d / "jobs.json"), "w") as f:
        json.dump(jobs, f)
    out = str(d / "out.npz")
    p = subprocess.run([sys.executable, sc.__file__, str(d / "jobs.json"), out], env=dict(os.environ, HMOGP_STRICT_FORM="2"),
                       timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    print(p.stdout)
    assert p.returncode == 0, ("the child ended with %r" % p.returncode, p.stdout[-4000:])
    z = np.load(out)
    assert str(z["form"]) == "2"
    res = {}
    for i, name in enumerate(JOBS):
        Df = rc.dense_case(JOBS[name][0])[1]["Df"]
        g = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("%d/" % i) and k.count("/") == 1}
        for k in ("m", "v"):
            if "%d/%s/0" % (i, k) in z.files:
                g[k] = [z["%d/%s/%d" % (i, k, dd)] for dd in range(Df)]
        res[name] = g
    return res


def ck(tag):
    return rr.c_kernel_wide() if tag in rc.WIDE_TAGS else rr.c_kernel()


def held(name, got, R, S, C, kinds):
    w = rr.check(name, got, R, S, C, kinds)
    for k in kinds:
        print("[strict2] %-20s %-4s worst |got - R| / (2^-52 S) = %-10.4g (C = %g)" % (name, k, w[k], C[k]))
    return w


def as_kinds(flat, prob):
    """The flat result of sc.evaluate as the criterion's dict (m, v as lists per function)."""
    g = {k: v for k, v in flat.items() if "/" not in k}
    for k in ("m", "v"):
        if k + "/0" in flat:
            g[k] = [flat["%s/%d" % (k, d)] for d in range(prob["Df"])]
    return g


def strict_engine(case, **kw):
    from hetmogp_amd.engine import Engine
    prob = case[1]
    e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], strict_qf=True, **kw)
    e.set_data(case[2], case[3])
    return e


# ------------------------------------------------------------------------------------------------ the forced two-solve form (child)
@pytest.mark.parametrize("name", [n for n in JOBS if JOBS[n][3] is not None])
def test_two_solve_form_vs_extended_precision(refs, child, name):
    """The bundle and q(f) of a forced two-solve evaluation, every element, against the `strict2` reference; evaluated twice in the
    child with the same bits."""
    tag, _, variant, kinds = JOBS[name]
    R, S = refs[tag][variant]
    got = child[name]
    assert bool(got["same"]), "two identical evaluations differ in their bits"
    held(name + " strict2", got, R, S, ck(tag), kinds)
    assert float(got["nneg"][0]) == float(R["nneg"][0])


def test_case_D_pools_of_300_equal_the_one_pool_run(refs, child):
    """chunk_rows = 300 (every pool below 1024 rows: the substitution path and `strict_rowstats_kernel` phase 0 with t2) and
    chunk_rows = 1100 (one panel pool and one short pool in one evaluation) against the one-pool run (the panel kernels): the two are
    different kernels for the same numbers and must agree within the constants, element by element."""
    _, S = refs["D"]["strict2"]
    one = child["D one pool"]
    for name in ("D chunk_rows=300", "D chunk_rows=1100"):
        held(name + " vs one pool", child[name], one, S, ck("D"), MV)


def test_case_D_two_solve_tail(refs, child):
    """The injected `strict2` bundle of D through hmogp_step_finish on a forced two-solve engine: the `strict && strict_two` branch of
    the tail takes the bundle's H and r as dVE_dS and dVE_dmu directly; every kind of tests/tail_ref.py under C_KERNEL_TWO (C_KERNEL
    but for dL_dS and g_L_u, which the oracle's own measurement on this variant moved by a factor 2: tail_ref.py)."""
    import tail_cases as tc
    import tail_ref as tr
    o = tc.references()["D"]["strict2"]
    got = child["D tail"]
    assert bool(got["same"])
    w = tr.check("D strict2", got, o["R"], o["S"], tr.c_kernel_two())
    for k in tr.KINDS:
        print("[strict2] %-20s %-13s worst |got - R| / (2^-52 S) = %-10.4g (C = %g)" % ("D tail strict2", k, w[k], tr.c_kernel_two()[k]))


# ------------------------------------------------------------------------------------------------ this process: no switch set
@pytest.mark.parametrize("tag", ["D", "G", "H", "J"])
def test_one_solve_form_q_f_through_predict_f(refs, tag):
    """strict_qf=True at rung 6 (the one-solve form): m and v through hmogp_predict_f after the evaluation, and the bundle."""
    assert "HMOGP_STRICT_FORM" not in os.environ
    case = rc.dense_case(tag)
    R, S = refs[tag]["strict"]
    e = strict_engine(case)
    try:
        got = as_kinds(sc.evaluate(e, case, {}), case[1])
    finally:
        e.close()
    assert float(got["cond_est"].max()) <= 1e6
    held(tag + " strict (one-solve)", got, R, S, ck(tag), MV)


def k_params(kind):
    """Case K and its neighbours on the same data: "K", "one" (latent 0 at 1 h: the one-solve form), "m_u" (K with another m_u)."""
    prm, prob, X, Y, rungs = rc.auto_case()
    if kind == "one":
        prm = dict(prm, lengthscale=rc.auto_case(cs0=1.0)[0]["lengthscale"])
    if kind == "m_u":
        prm = dict(prm, m_u=prm["m_u"] * 1.5 + 0.01)
    return prm, prob, X, Y, rungs


def test_case_K_takes_the_two_solve_form_by_itself(refs):
    """Case K (estimate about 4e6 on latent 0, forced rungs [-1, 6]): the engine picks the two-solve form with no switch set.  The
    bundle's H is the two-solve one (close to A^T diag(beta) A, O(1) away from X^T diag(beta) X); closeness to R is
    conditioning-limited: every kind within 16 x the float64 oracle's own array-norm distance (rc.K_ORACLE_DIST, measured on the CPU)."""
    assert "HMOGP_STRICT_FORM" not in os.environ
    case = k_params("K")
    e = strict_engine(case)
    try:
        got = as_kinds(sc.evaluate(e, case, {}), case[1])
    finally:
        e.close()
    R2, R1 = refs["K"]["two"][0], refs["K"]["one"][0]
    print("[strict2] K cond_est %s rungs %s" % (got["cond_est"], got["rungs"]))
    assert got["cond_est"][0] > 1e6 and got["cond_est"][1] <= 1e3 and list(got["rungs"]) == rc.K_RUNGS
    lo = np.tril(np.ones((case[1]["M"],) * 2, dtype=bool))          # (the bundle's H_q is valid in its lower triangle)
    H = np.asarray(got["H"], dtype=np.float64)[:, lo]
    d2, d1 = [float(np.linalg.norm(H - np.asarray(r["H"], dtype=np.float64)[:, lo]) / np.linalg.norm(np.asarray(r["H"], dtype=np.float64)[:, lo]))
              for r in (R2, R1)]
    print("[strict2] K H    |H - A^T b A| / |A^T b A| = %.3g   |H - X^T b X| / |X^T b X| = %.3g" % (d2, d1))
    assert d2 < 1e-3 and d1 > 0.5
    dist = rc.array_distances(got, R2)
    for k in rc.K_KINDS:
        print("[strict2] K %-4s max|got - R| / max|R| = %-10.3g (16 x oracle = %.3g)" % (k, dist[k], 16 * rc.K_ORACLE_DIST[k]))
    bad = {k: dist[k] for k in rc.K_KINDS if not dist[k] <= 16 * rc.K_ORACLE_DIST[k]}
    assert not bad, bad


def test_form_follows_the_parameters_not_the_history():
    """One strict engine with a cached K_uu chain: K (two-solve), the 1 h neighbour (one-solve), K again, K with m_u changed only (a
    cached chain: the form must survive it).  Every evaluation gives the bits of the same evaluation on a fresh engine."""
    assert "HMOGP_STRICT_FORM" not in os.environ
    order = ["K", "one", "K", "m_u"]
    cases = {k: k_params(k) for k in set(order)}
    e = strict_engine(cases["K"], cache_kuu=True)
    try:
        seen = [sc.evaluate(e, cases[k], {}) for k in order]
    finally:
        e.close()
    for i, k in enumerate(order):
        f = strict_engine(cases[k], cache_kuu=True)
        try:
            fresh = sc.evaluate(f, cases[k], {})
        finally:
            f.close()
        two = bool(fresh["cond_est"][0] > 1e6)
        print("[strict2] history step %d %-4s cond_est %s two-solve %s" % (i + 1, k, fresh["cond_est"], two))
        assert two == (k != "one")
        assert sorted(seen[i]) == sorted(fresh)
        diff = [n for n in fresh if not np.array_equal(seen[i][n], fresh[n])]
        assert not diff, ("step %d (%s) differs from a fresh engine in" % (i + 1, k), diff)
