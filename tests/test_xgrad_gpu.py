"""GPU: gradients of q(f) with respect to the new inputs (`hmogp_qf_input_grad` / `hmogp_predict_f_grad`) against the 50-digit grid
tests/golden/xgradgrid.npz and the restatements of tests/xgrad_ref.py -- the building block over the kernel's own boundaries, exact row
independence, the engine path in the default and the strict mode on the small-model and the regular path, chunks, the refusals, the facade.

Criterion (xgrad_ref's docstring): |got - R| <= C (2^-52 S + 2^-1022 F), C = max(16, 4 C_ORACLE) = 16 for dm and dv; every row of every case
is also held to the float64 restatement with C_KERNEL + C_ORACLE = 16.5 / 16.125.  The strict engine path is held to the 50-digit chain from the raw
parameters at M = 16 with the scale S x the engine's cond_est and its own constant (16).  Measured on the MI355X, 2026-10-21: building
block against 50 digits dm 0.383, dv 0.087 (M2_N63); every row against float64 dm 0.431, dv 0.128; the engine's default mode equals the
building block bit for bit; strict mode against the 50-digit chain dm 0.819, dv 0.015 (s_N129).  Every case and figure: DESIGN 9t."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import joint_ref as jr            # noqa: E402
import xgrad_ref as xr            # noqa: E402

pytestmark = pytest.mark.gpu

GRID = xr.load_grid()
NAMES = [c["name"] for c in xr.CASES]
_CACHE = {}


def rows_of(inp, exact, X=None, W=None):
    from hetmogp_amd import engine
    return engine.qf_input_grad_rows(inp["X"] if X is None else X, inp["Z"], inp["variance"], inp["lengthscale"], inp["a"], inp["C"],
                                     inp["W"] if W is None else W, exact=exact, device=0)


def block(name):
    """(inputs, dm, dv) of one designed case on the device: computed once, left unchanged."""
    if name not in _CACHE:
        c = xr.CASE_BY_NAME[name]
        inp = xr.make_inputs(c)
        _CACHE[name] = (inp,) + rows_of(inp, c["exact"])
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_building_block_against_both_restatements(name):
    c = xr.CASE_BY_NAME[name]
    inp, dm, dv = block(name)
    assert dm.shape == dv.shape == (c["N"], c["Df"], c["P"])
    rm, rv = xr.case_ratios(GRID[name], dm, dv)
    fm, fv, sm, sv, Fm, Fv = xr.input_grad(inp, return_scale=True)
    qm, qv = float(np.max(xr.ratios(dm, fm, sm, Fm))), float(np.max(xr.ratios(dv, fv, sv, Fv)))
    print("%s: against 50 digits dm %.3f dv %.3f (C %g); every row against float64 dm %.3f dv %.3f (C %g)" %
          (name, rm, rv, xr.c_kernel("dm"), qm, qv, xr.c_sum("dm")))
    assert rm <= xr.c_kernel("dm") and rv <= xr.c_kernel("dv")
    assert qm <= xr.c_sum("dm") and qv <= xr.c_sum("dv")
    on, far = xr.special_rows(c)
    if far is not None:                                  # every k underflows: exactly 0, or within the floor
        assert np.all(np.abs(dm[far]) <= xr.c_kernel("dm") * xr.TINY * Fm[far]) and np.all(np.abs(dv[far]) <= xr.c_kernel("dv") * xr.TINY * Fv[far])
    if c["Q"] * c["Df"] > 1 and c["Q"] == 1:             # the function whose only weight is exactly 0
        assert np.all(dm[:, 0] == 0.0) and np.all(dv[:, 0] == 0.0)


@pytest.mark.parametrize("name", ["M65_N257", "M128_N257", "M129_N64", "M2_N63"])
def test_row_independence(name):
    """A row's bits depend on that row's own inputs alone: a permuted subset of rows, every leading block of 1, 63, 64, 65, 257 rows, a
    sub-list of functions."""
    c = xr.CASE_BY_NAME[name]
    inp, dm, dv = block(name)
    N = c["N"]
    perm = np.random.RandomState(4).permutation(N)[:max(1, (2 * N) // 3)]
    pm, pv = rows_of(inp, c["exact"], X=inp["X"][perm])
    assert np.array_equal(pm, dm[perm]) and np.array_equal(pv, dv[perm])
    for n in (1, 63, 64, 65, 257):
        if n < N:
            hm, hv = rows_of(inp, c["exact"], X=inp["X"][:n])
            assert np.array_equal(hm, dm[:n]) and np.array_equal(hv, dv[:n]), n
            tm, tv = rows_of(inp, c["exact"], X=inp["X"][N - n:])
            assert np.array_equal(tm, dm[N - n:]) and np.array_equal(tv, dv[N - n:]), n
    sub = [2, 0]
    sm, sv = rows_of(inp, c["exact"], W=np.ascontiguousarray(inp["W"][:, sub]))
    assert np.array_equal(sm, dm[:, sub]) and np.array_equal(sv, dv[:, sub])


# ------------------------------------------------------------------------------------------------------------ the engine path
def engine_for(prm, case, **ekw):
    from hetmogp_amd.engine import Engine
    X, Y = jr.train_data(case)
    e = Engine(jr.SPECS, prm["variance"].shape[0], prm["Z"].shape[0], case["P"], device=0, **ekw)
    e.set_data(X, Y)
    out = e.elbo_grad(**prm)
    assert all(r == -1 for r in out["rungs"])              # K_uu of the designed cases factorises without jitter
    return e, out


@pytest.mark.parametrize("name,ekw", [("r_N129", {}), ("s_N65", {}), ("s_N129", {}), ("r_N129", {"chunk_rows": 48}), ("s_N63", {"strict_qf": True}),
                                      ("s_N65", {"strict_qf": True}), ("s_N129", {"strict_qf": True}), ("r_N129", {"strict_qf": True})],
                         ids=["regular", "small-model-Q3-P4", "small-model", "chunks-of-48", "strict-s_N63", "strict-s_N65", "strict-s_N129",
                              "strict-regular"])
def test_engine_path(name, ekw):
    import make_xgrad_grid as mg
    case = jr.CASE_BY_NAME[name]
    prm, Xnew = jr.make_params(case)
    strict = bool(ekw.get("strict_qf"))
    e, out = engine_for(prm, case, **ekw)
    dm, dv = e.predict_f_grad(Xnew)
    m, v, dm2, dv2 = e.predict_f_grad(Xnew, return_mv=True)
    pm, pv = e.predict_f(Xnew)
    assert np.array_equal(m, pm) and np.array_equal(v, pv)                     # the bits of predict_f
    assert np.array_equal(dm, dm2) and np.array_equal(dv, dv2)
    assert dm.shape == dv.shape == (case["N"], jr.DF, case["P"]) and np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
    # chunks of 48 rows against the unchunked call: the same bits
    e48, _ = (engine_for(prm, case, **dict(ekw, chunk_rows=48)) if "chunk_rows" not in ekw else engine_for(prm, case))
    cm, cv = e48.predict_f_grad(Xnew)
    assert np.array_equal(cm, dm) and np.array_equal(cv, dv)
    e48.close()
    wv, wi = e.posterior_u()
    inp = dict(X=Xnew, Z=prm["Z"], variance=prm["variance"], lengthscale=prm["lengthscale"], a=wv, C=-wi, W=prm["W"])
    _, _, sm, sv, Fm, Fv = xr.input_grad(inp, return_scale=True)
    if not strict:
        # the building block fed with posterior_u()'s (woodbury_vector, -woodbury_inv) and the engine's hyper-parameters
        bm, bv = rows_of(inp, exact=False)
        rm, rv = float(np.max(xr.ratios(dm, bm, sm, Fm))), float(np.max(xr.ratios(dv, bv, sv, Fv)))
        print("%s %s: against the building block dm %.3f dv %.3f (2 C = %g)" % (name, ekw, rm, rv, 2.0 * xr.c_kernel("dm")))
        assert rm <= 2.0 * xr.c_kernel("dm") and rv <= 2.0 * xr.c_kernel("dv")
    if name in mg.CHAIN_CASES:
        # the whole chain from (Z, m_u, L_flat, hypers) at 50 digits; scale S x the engine's returned cond_est
        g = mg.load_chain(name)
        cond = float(np.max(out["cond_est"]))
        rm = float(np.max(xr.ratios(dm[g["rows"]], g["dm"], cond * g["S_dm"], g["F_dm"])))
        rv = float(np.max(xr.ratios(dv[g["rows"]], g["dv"], cond * g["S_dv"], g["F_dv"])))
        print("%s %s: against the 50-digit chain dm %.3f dv %.3f of S x cond_est (%.1f); C %g" % (name, ekw, rm, rv, cond, xr.c_kernel("dm", True)))
        if strict:
            assert rm <= xr.c_kernel("dm", True) and rv <= xr.c_kernel("dv", True)
    e.close()


def test_refusals():
    """E_STATE before the first evaluation; every refusal is followed by a valid call that returns the same bits as before."""
    from hetmogp_amd import _lib, engine
    from hetmogp_amd.engine import Engine
    case = jr.CASE_BY_NAME["s_N64"]
    prm, Xnew = jr.make_params(case)
    Xnew = np.ascontiguousarray(Xnew[:5])
    X, Y = jr.train_data(case)
    e = Engine(jr.SPECS, case["Q"], case["M"], case["P"], device=0)
    e.set_data(X, Y)
    with pytest.raises(_lib.HetMOGPError) as ei:
        e.predict_f_grad(Xnew)
    assert ei.value.code == _lib.E_STATE
    e.elbo_grad(**prm)
    good = e.predict_f_grad(Xnew)
    P, Df = case["P"], jr.DF
    xp = Xnew.ctypes.data_as(_lib.c_double_p)
    b1, b2 = np.zeros((5, Df, P)), np.zeros((5, Df, P))
    p1, p2 = b1.ctypes.data_as(_lib.c_double_p), b2.ctypes.data_as(_lib.c_double_p)

    def still_fine():
        dm, dv = e.predict_f_grad(Xnew)
        assert np.array_equal(dm, good[0]) and np.array_equal(dv, good[1])

    for args in ((None, 5, None, None, p1, p2), (xp, 5, None, None, None, p2), (xp, 5, None, None, p1, None), (xp, -1, None, None, p1, p2)):
        assert _lib.lib.hmogp_predict_f_grad(e._h, *args) == _lib.E_INVALID
        still_fine()
    assert _lib.lib.hmogp_predict_f_grad(None, xp, 5, None, None, p1, p2) == _lib.E_INVALID
    assert _lib.lib.hmogp_predict_f_grad(e._h, None, 0, None, None, None, None) == 0          # N = 0 returns at once
    assert e.predict_f_grad(np.zeros((0, P)))[0].shape == (0, Df, P)
    assert _lib.lib.hmogp_predict_f_grad(e._h, xp, 5, None, None, p1, p2) == 0 and np.array_equal(b1, good[0]) and np.array_equal(b2, good[1])
    still_fine()
    # the building block: a refusal, then a valid call
    c = xr.CASE_BY_NAME["M2_N63"]
    inp, dm, dv = block("M2_N63")
    for bad in (dict(variance=-inp["variance"]), dict(lengthscale=inp["lengthscale"] * np.nan), dict(a=inp["a"][:, :1]), dict(X=np.zeros((3, 5)))):
        with pytest.raises(_lib.InvalidArgument):
            rows_of(dict(inp, **bad), c["exact"])
        gm, gv = rows_of(inp, c["exact"])
        assert np.array_equal(gm, dm) and np.array_equal(gv, dv)
    with pytest.raises(_lib.HetMOGPError) as ei:
        engine.qf_input_grad_rows(inp["X"], inp["Z"], inp["variance"], inp["lengthscale"], inp["a"], inp["C"], inp["W"], device=1 << 20)
    assert ei.value.code == _lib.E_NO_DEVICE
    e.close()


# ------------------------------------------------------------------------------------------------------------ the facade
@pytest.fixture(scope="module")
def model():
    """The designed sensitivity case as a model: 2-D inputs, q(u)'s mean a function of column 0 of the inducing inputs only, small S."""
    import hetmogp_amd as H
    rng = np.random.RandomState(5)
    prm, _ = xr.sensitivity_case()
    Q, P, n = 1, 2, 40
    M = prm["Z"].shape[0]
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.4), H.HetGaussian(), H.Poisson()])
    md = likelihood.generate_metadata()
    kern_list = H.latent_functions_prior(Q, lenghtscale=[float(prm["lengthscale"][0])], variance=[1.0], input_dim=P)
    X = [rng.rand(n, P) for _ in range(3)]
    Y = [rng.randn(n, 1), rng.randn(n, 1), rng.poisson(2.0, (n, 1)).astype(float)]
    m = H.SVMOGP(X=X, Y=Y, Z=prm["Z"], kern_list=kern_list, likelihood=likelihood, Y_metadata=md)
    m.q_u_means[...] = prm["m_u"]
    m.q_u_chols[...] = prm["L_flat"]
    m.parameters_changed()
    return m


def test_facade_shapes_and_ordering(model):
    X = np.random.RandomState(2).rand(9, 2)
    Df = model.num_output_funcs
    assert Df == 4
    dm, dv = model.predictive_gradients(X)
    assert dm.shape == dv.shape == (9, Df, 2) and np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
    e0, e1 = model._engine.predict_f_grad(X)
    assert np.array_equal(dm, e0) and np.array_equal(dv, e1)
    sm, sv = model.predictive_gradients(X, functions=[2, 0])
    assert sm.shape == (9, 2, 2) and np.array_equal(sm, dm[:, [2, 0]]) and np.array_equal(sv, dv[:, [2, 0]])
    with pytest.raises(ValueError):
        model.predictive_gradients(X, functions=[Df])


def test_facade_input_sensitivity(model):
    s = model.input_sensitivity()
    pooled = np.concatenate(model.Xmulti_all, 0)
    dm, _ = model.predictive_gradients(pooled)
    assert s.shape == (4, 2) and np.array_equal(s, np.sqrt(np.mean(dm * dm, axis=0)))
    X = np.random.RandomState(3).rand(30, 2)
    s2 = model.input_sensitivity(X, functions=[3, 1])
    d2, _ = model.predictive_gradients(X, functions=[3, 1])
    assert s2.shape == (2, 2) and np.array_equal(s2, np.sqrt(np.mean(d2 * d2, axis=0)))
    print("input sensitivity (functions x columns):\n%s" % s)
    assert np.all(s[:, 0] >= 5.0 * s[:, 1]) and np.all(s[:, 0] > 0.0)          # the designed case: column 0 matters, column 1 does not


def test_facade_strict_auto_model_gives_finite_gradients():
    """A model whose strict_qf="auto" has switched to the strict mode (the jitter-ladder regime of tests/golden/lad_h_mix_M128_ladder.npz)."""
    from test_facade_gpu import build_model
    g = np.load(os.path.join(HERE, "golden", "lad_h_mix_M128_ladder.npz"))
    m = build_model(g, None, strict_qf="auto")
    m.parameters_changed()
    assert m.strict_switches >= 1 and m._strict_now
    X = np.ascontiguousarray(np.concatenate(m.Xmulti_all, 0)[:70])
    dm, dv = m.predictive_gradients(X)
    assert dm.shape == dv.shape == (70, m.num_output_funcs, m.Xdim) and np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
    assert np.any(dm != 0.0) and np.any(dv != 0.0)
    s = m.input_sensitivity(X)
    assert s.shape == (m.num_output_funcs, m.Xdim) and np.all(np.isfinite(s))
