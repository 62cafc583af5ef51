"""GPU: gradients of posterior sample paths with respect to new inputs (`hmogp_paths_eval_grad`) against the 50-digit restatement
tests/pathsgrad_ref_mp.py evaluated from the device's OWN state and the float64 restatement tests/pathsgrad_ref.py -- the ten designed cases
and the two P = 3 cases beyond them (M odd, M even) from a default-mode and a strict-mode evaluation, the values' bits, independence of rows, chunks, S, the list of functions
and whether the values are asked for, one set of bits in both modes, the snapshot, the mean of the gradients against `predict_f_grad`, central
differences of the device's own paths, a call beyond the joint route's bound, the refusals, the facade.

Criterion (pathsgrad_ref's docstring): |got - R| <= C 2^-52 scale_G; C = max(16, 4 C_ORACLE) = 16 with C_ORACLE = 1 (raw 0.483, 2026-10-21).
Finite differences (h = 2^-10 l_min): the float64 restatement's own difference quotient misses the 50-digit gradient by 6.3e-07 (s_N64) and
5.5e-07 (r_N65) of max |G| -- the truncation term; the device is allowed 4 times that, 2.52e-06 and 2.2e-06, and measures
6.287e-07 and 5.437e-07 (MI355X, 2026-10-21): the truncation term again.  The device's ratios per case, the statistical worst |z| (1.96 of 5.53)
and the timing table: DESIGN 9w."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import paths_ref as pr            # noqa: E402
import pathsgrad_ref as gr        # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in gr.CASES]
ALL = dict(gr.CASE_BY_NAME, **{c["name"]: c for c in gr.EXTRA_CASES})
EXTRA = [c["name"] for c in gr.EXTRA_CASES]
MODES = [False, True]
N_EVAL = 24                        # entries per case the gradient is held to 50 digits on
_ENG, _RES, _REF = {}, {}, {}


def ids(strict):
    return "strict" if strict else "default"


def engine(name, strict=False, **kw):
    """One engine per (case, mode, options), with the case's parameters evaluated once."""
    key = (name, strict, tuple(sorted(kw.items())))
    if key not in _ENG:
        from hetmogp_amd.engine import Engine
        case = ALL[name]
        prm, _ = gr.make_params(case)
        X, Y = gr.train_data(case)
        e = Engine(gr.SPECS, case["Q"], case["M"], case["P"], device=0, strict_qf=strict, **kw)
        e.set_data(X, Y)
        out = e.elbo_grad(**prm)
        assert all(r == -1 for r in out["rungs"])
        _ENG[key] = e
    return _ENG[key]


def result(name, strict):
    """The designed path set of one (case, mode): state, values and gradients, computed once, left unchanged."""
    key = (name, strict)
    if key not in _RES:
        c = ALL[name]
        prm, Xnew = gr.make_params(c)
        e = engine(name, strict)
        sid = e.paths_create(c["functions"], size=c["S"], num_features=c["Lf"], seed=gr.GRID_SEED)
        G = e.paths_eval_grad(sid, Xnew)                   # (the set's first gradient call, before any paths_eval)
        _RES[key] = dict(engine=e, sid=sid, prm=prm, Xnew=Xnew, state=e.paths_state(sid), G=G, F=e.paths_eval(sid, Xnew))
    return _RES[key]


def reference(name):
    """(indices, R, scale): the 50-digit gradient from the device's own state (the default mode's; the strict one's is the same bits)."""
    if name not in _REF:
        import pathsgrad_ref_mp as gm
        c, r = ALL[name], result(name, False)
        size = r["G"].size
        idx = np.sort(np.random.RandomState(9700 + c["seed"]).choice(size, min(size, N_EVAL), replace=False))
        _REF[name] = (idx,) + gm.evaluate_grad(r["state"], r["prm"], c["P"], r["Xnew"], idx)
    return _REF[name]


@pytest.mark.parametrize("name", NAMES + EXTRA)
def test_gradient_against_50_digits_from_the_own_state(name):
    c = ALL[name]
    idx, R, sc = reference(name)
    for strict in MODES:
        r = result(name, strict)
        assert r["G"].shape == (c["S"], len(c["functions"]), c["N"], c["P"]) and np.all(np.isfinite(r["G"]))
        ratio = float(np.max(gr.ratios(gr.pick(r["G"], idx), R, sc)))
        print("%s %s: G %.3f (C %g) on %d entries" % (name, ids(strict), ratio, gr.c_kernel(), len(idx)))
        assert ratio <= gr.c_kernel()
    # ... and every entry against the float64 restatement from the same state: each within its own constant of the 50-digit value
    r = result(name, False)
    G64, s64 = gr.evaluate_grad(r["state"], r["prm"], c["P"], r["Xnew"], return_scale=True)
    worst = float(np.max(gr.ratios(r["G"], G64, s64)))
    print("%s: against the float64 restatement %.3f (C %g) on %d entries" % (name, worst, gr.c_sum(), G64.size))
    assert worst <= gr.c_sum()


@pytest.mark.parametrize("name", NAMES + EXTRA)
def test_values_are_paths_eval_bits_and_modes_agree(name):
    a, b = result(name, False), result(name, True)
    for r in (a, b):
        F, G = r["engine"].paths_eval_grad(r["sid"], r["Xnew"], values=True)
        assert np.array_equal(F, r["F"]) and np.array_equal(F, r["engine"].paths_eval(r["sid"], r["Xnew"]))
        assert np.array_equal(G, r["G"])                   # the same with F = NULL and with F given
    assert np.array_equal(a["G"], b["G"]) and np.array_equal(a["F"], b["F"])          # one set of bits in both modes
    assert all(np.array_equal(a["state"][k], b["state"][k]) for k in a["state"])


@pytest.mark.parametrize("N", [1, 63, 65, 257])
@pytest.mark.parametrize("name", ["s_N64", "r_N65"] + EXTRA)
def test_row_independence(name, N):
    """The rows of a call equal the same rows evaluated alone (N = 1), in two halves, and in a second call."""
    c = ALL[name]
    r = result(name, False)
    e, sid = r["engine"], r["sid"]
    X = np.random.RandomState(100 + N).rand(N, c["P"])
    G = e.paths_eval_grad(sid, X)
    assert G.shape == (c["S"], len(c["functions"]), N, c["P"]) and np.all(np.isfinite(G))
    assert np.array_equal(G, e.paths_eval_grad(sid, X))
    for i in sorted({0, N // 2, N - 1}):
        assert np.array_equal(G[:, :, i:i + 1], e.paths_eval_grad(sid, X[i:i + 1]))
    h = (N + 1) // 2
    assert np.array_equal(G[:, :, :h], e.paths_eval_grad(sid, X[:h])) and np.array_equal(G[:, :, h:], e.paths_eval_grad(sid, X[h:]))
    rows = [0, N - 1, N // 3]                                # the same rows alone, in another order
    assert np.array_equal(G[:, :, rows], e.paths_eval_grad(sid, X[rows]))


@pytest.mark.parametrize("name", ["s_N129", "r_N129"])
def test_forced_chunks_give_the_same_bits(name):
    """Chunks of 48 rows over 129 against the unchunked call, values and gradients."""
    c = ALL[name]
    r = result(name, False)
    e48 = engine(name, False, chunk_rows=48)
    sid = e48.paths_create(c["functions"], size=c["S"], num_features=c["Lf"], seed=gr.GRID_SEED)
    F, G = e48.paths_eval_grad(sid, r["Xnew"], values=True)
    assert np.array_equal(G, r["G"]) and np.array_equal(F, r["F"])
    e48.paths_free(sid)


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", ["s_N64", "r_N65"])
def test_samples_and_functions(name, strict):
    c = ALL[name]
    e = engine(name, strict)
    d = list(c["functions"])
    X = result(name, strict)["Xnew"]
    sets = {S: e.paths_create(d, size=S, num_features=c["Lf"], seed=3) for S in (1, 3, 8)}
    G = {S: e.paths_eval_grad(sid, X) for S, sid in sets.items()}
    for S in (1, 3):                                        # sample s does not depend on S
        assert np.array_equal(G[S], G[8][:S])
    sub = [len(d) - 1, 0]                                   # positions in d: a sub-list, in another order
    sid = e.paths_create([d[j] for j in sub], size=8, num_features=c["Lf"], seed=3)
    assert np.array_equal(e.paths_eval_grad(sid, X), G[8][:, sub])
    for s in list(sets.values()) + [sid]:
        e.paths_free(s)


def test_a_set_is_a_snapshot():
    """A later evaluation with other parameters, a q(u) update and hmogp_set_lik_params do not change a set's gradients -- whether the
    rotated operand was built before them (set `old`) or is built after them (set `late`, first differentiated at the end)."""
    name = "s_N63"
    c = ALL[name]
    from hetmogp_amd.engine import Engine
    prm, Xnew = gr.make_params(c)
    X, Y = gr.train_data(c)
    e = Engine(gr.SPECS, c["Q"], c["M"], c["P"], device=0)
    e.set_data(X, Y)
    e.elbo_grad(**prm)
    old = e.paths_create(c["functions"], size=3, num_features=8, seed=1)
    late = e.paths_create(c["functions"], size=3, num_features=8, seed=1)
    G0 = e.paths_eval_grad(old, Xnew)
    prm2 = dict(prm, m_u=prm["m_u"] + 0.1, lengthscale=prm["lengthscale"] * 1.1, variance=prm["variance"] * 0.9, W=prm["W"] * 1.2,
                Z=prm["Z"] + 0.001)
    e.elbo_grad(**prm2)
    assert np.array_equal(e.paths_eval_grad(old, Xnew), G0)
    e.qu_load(prm2["m_u"], prm2["L_flat"])
    e.elbo_grad(**dict(prm2, m_u=None, L_flat=None))
    e.qu_natgrad(0.1)
    e.elbo_grad(**dict(prm2, m_u=None, L_flat=None))        # (after a q(u) step every posterior call asks for a fresh evaluation: HMOGP_E_STATE)
    assert np.array_equal(e.paths_eval_grad(old, Xnew), G0)
    e.set_lik_params(0, [0.8])
    assert np.array_equal(e.paths_eval_grad(old, Xnew), G0)
    assert np.array_equal(e.paths_eval_grad(late, Xnew), G0)
    new = e.paths_create(c["functions"], size=3, num_features=8, seed=1)
    assert not np.any(e.paths_eval_grad(new, Xnew) == G0)
    e.close()


def test_mean_of_the_gradients_is_the_gradient_of_the_mean():
    """n = 8 rows, P = 2, S = 4096 (two single-function sets of one seed, as DESIGN 9v splits it), Lf = 64: given the frequencies the mean of G
    over the samples is predict_f_grad's dm; the per-entry standard deviation comes from the paths' own linear map in the restatement."""
    prm, Xnew, d = gr.stat_case()
    name = "s_N64"
    assert all(np.array_equal(prm[k], gr.make_params(ALL[name])[0][k]) for k in prm)
    e = engine(name)
    sids = [e.paths_create([dj], size=gr.STAT_DRAWS, num_features=gr.STAT_FEATURES, seed=gr.STAT_SEED) for dj in d]
    G = np.concatenate([e.paths_eval_grad(s, Xnew) for s in sids], 1).reshape(gr.STAT_DRAWS, -1)
    omega = e.paths_state(sids[0])["omega"]
    for s in sids:
        e.paths_free(s)
    dm = np.transpose(e.predict_f_grad(Xnew)[0][:, list(d)], (1, 0, 2)).reshape(-1)
    B = gr.grad_linear_map(omega, prm, Xnew.shape[1], d, Xnew)
    sd = np.sqrt((B * B).sum(1))
    z, count = gr.stat_mean_z(G, dm, sd)
    t = pr.z_threshold(count)
    print("worst |z| %.2f over %d statistics, threshold %.2f" % (z, count, t))
    assert count == 32 and z <= t


@pytest.mark.parametrize("name", gr.FD_CASES)
def test_finite_differences_of_the_own_paths(name):
    """Central differences of paths_eval (h = 2^-10 l_min) against the 50-digit gradient from the device's own state, on the entries and in
    the statistic the tolerance was measured with (tools/make_pathsgrad_grid.py: fd_error)."""
    import make_pathsgrad_grid as mk
    import pathsgrad_ref_mp as gm
    c, r = ALL[name], result(name, False)
    e, sid = r["engine"], r["sid"]
    quo = mk.fd_quotient(lambda X: e.paths_eval(sid, X), r["Xnew"], float(np.min(r["prm"]["lengthscale"])), c["P"])
    idx = mk.fd_entries(c)
    R, _ = gm.evaluate_grad(r["state"], r["prm"], c["P"], r["Xnew"], idx)
    err = float(np.max(np.abs(gr.pick(quo, idx) - R)) / np.max(np.abs(R)))
    tol = gr.FD_FACTOR * gr.FD_MEASURED[name]
    print("%s: finite differences miss by %.3e of max |G| (restatement %.3e, tolerance %.3e)" % (name, err, gr.FD_MEASURED[name], tol))
    assert err <= tol


def test_beyond_the_joint_bound():
    name = "s_N64"
    c = ALL[name]
    e = engine(name)
    X = np.random.RandomState(8).rand(10000, c["P"])
    sid = e.paths_create([0], size=2, num_features=16, seed=2)
    F, G = e.paths_eval_grad(sid, X, values=True)
    assert G.shape == (2, 1, 10000, c["P"]) and np.all(np.isfinite(G)) and np.array_equal(F, e.paths_eval(sid, X))
    for r0 in range(0, 10000, 1000):
        assert np.array_equal(G[:, :, r0:r0 + 1000], e.paths_eval_grad(sid, X[r0:r0 + 1000]))
    e.paths_free(sid)


def test_refusals():
    """Every refusal is HMOGP_E_INVALID (HMOGP_E_STATE before the first evaluation) and is followed by a valid call on the same engine."""
    import ctypes as C
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine
    case = ALL["s_N64"]
    prm, Xnew = gr.make_params(case)
    Xnew = np.ascontiguousarray(Xnew[:5])
    X, Y = gr.train_data(case)
    e = Engine(gr.SPECS, case["Q"], case["M"], case["P"], device=0)
    e.set_data(X, Y)
    h = e._h
    xp = Xnew.ctypes.data_as(_lib.c_double_p)
    buf = np.full(64, 7.0)
    bp = buf.ctypes.data_as(_lib.c_double_p)
    f = _lib.lib.hmogp_paths_eval_grad
    assert f(h, 0, xp, 5, None, bp) == _lib.E_STATE                                                # before the first evaluation
    e.elbo_grad(**prm)
    good_id = e.paths_create([0, 3], size=2, num_features=8, seed=1)
    good = e.paths_eval_grad(good_id, Xnew)

    def still_fine():
        assert np.array_equal(e.paths_eval_grad(good_id, Xnew), good)

    for bad_id in (-1, _lib.PATHS_MAXSETS, good_id + 1):                                          # unknown ids
        assert f(h, bad_id, xp, 5, None, bp) == _lib.E_INVALID
        still_fine()
    for args in ((good_id, xp, -1, None, bp), (good_id, None, 5, None, bp), (good_id, xp, 5, None, None), (good_id, xp, 5, bp, None)):
        assert f(h, *args) == _lib.E_INVALID
        still_fine()
    assert np.all(buf == 7.0)                                                                      # no refusal wrote anything
    assert f(h, good_id, None, 0, None, bp) == 0 and f(h, good_id, None, 0, None, None) == 0       # Nnew = 0 returns at once ...
    assert np.all(buf == 7.0)                                                                      # ... without touching G
    assert e.paths_eval_grad(good_id, np.zeros((0, case["P"]))).shape == (2, 2, 0, case["P"])
    still_fine()
    gone = e.paths_create([1], size=1, num_features=2, seed=1)
    e.paths_eval_grad(gone, Xnew)
    e.paths_free(gone)
    assert f(h, gone, xp, 5, None, bp) == _lib.E_INVALID                                           # a freed id
    with pytest.raises(_lib.InvalidArgument, match="unknown or freed"):
        e.paths_eval_grad(gone, Xnew)
    still_fine()
    e.paths_free(good_id)                                                                          # the last live set: the workspace goes
    again = e.paths_create([0, 3], size=2, num_features=8, seed=1)
    assert np.array_equal(e.paths_eval_grad(again, Xnew), good)
    e.close()


# ------------------------------------------------------------------------------------------------------------ the facade
@pytest.fixture(scope="module")
def model():
    import hetmogp_amd as H
    rng = np.random.RandomState(5)
    Q, P, M, n = 2, 1, 12, 40
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.4), H.HetGaussian(), H.Poisson()])
    md = likelihood.generate_metadata()
    kern_list = H.latent_functions_prior(Q, lenghtscale=[0.12, 0.2], variance=[1.0, 0.7], input_dim=P)
    X = [np.sort(rng.rand(n, P), 0) for _ in range(3)]
    Y = [rng.randn(n, 1), rng.randn(n, 1), rng.poisson(2.0, (n, 1)).astype(float)]
    m = H.SVMOGP(X=X, Y=Y, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood, Y_metadata=md)
    m.q_u_means[...] = 0.6 * rng.randn(M, Q)
    r, c = np.tril_indices(M)
    m.q_u_chols[...] = np.stack([(0.5 * np.eye(M) + 0.05 * np.tril(rng.randn(M, M), -1))[r, c] for _ in range(Q)], 1)
    m.parameters_changed()
    return m


def test_facade_grad_and_value_and_grad(model):
    X = np.linspace(0.05, 0.95, 6)[:, None]
    Df = model.num_output_funcs
    paths = model.sample_paths(size=5, num_features=32, seed=3)
    G = paths.grad(X)
    assert G.shape == (5, 6, Df, 1) and np.all(np.isfinite(G)) and np.array_equal(G, paths.grad(X))
    F, G2 = paths.value_and_grad(X)
    assert F.shape == (5, 6, Df) and np.array_equal(F, paths(X)) and np.array_equal(G2, G)
    Fe, Ge = paths._engine.paths_eval_grad(paths._id, X, values=True)                 # the engine's values after the axis move
    assert np.array_equal(np.transpose(Ge, (0, 2, 1, 3)), G) and np.array_equal(np.transpose(Fe, (0, 2, 1)), F)
    assert np.array_equal(paths.grad(X[2:4]), G[:, 2:4])
    with model.sample_paths(size=2, functions=[2, 1], num_features=32, seed=3) as sub:
        assert np.array_equal(sub.grad(X), G[:2][:, :, [2, 1]])
    with pytest.raises(ValueError):
        sub.grad(X)                                         # closed by the context manager
    paths.close()
    with pytest.raises(ValueError):
        paths.grad(X)
    with pytest.raises(ValueError):
        paths.value_and_grad(X)
