"""GPU: the heteroscedastic Negative Binomial likelihood through every layer -- the row kernel against the high-precision
grid tests/golden/nbgrid.npz under the criterion of tests/likgrid.py and against the float64 restatement tests/negbin_ref.py, the
closed-form predictive, the sampler, the Monte-Carlo log predictive, the refusal of observations that are no counts, the whole ELBO +
gradient against the oracle (the checks of tests/model_cases.py) on the default, several-pool, minibatch, small-model and strict q(f)
paths, the model facade end to end, and the split step.

The oracle covers the family through a module-scoped fixture that registers tests/negbin_ref.py with oracle.likelihoods_oracle for
the duration of this module (`oracle/` is not edited): cases are drawn by model_cases.synth with Gamma standing in for the new task
(same dim_f), whose observations are then replaced by seeded Negative Binomial draws.

Kernel figures on nbgrid.npz, worst |kernel - R| / (2^-52 S) per class and kind (ve / dm / dv), measured 2026-10-19 on an MI355X:
see DESIGN 9h."""
import warnings

import numpy as np
import pytest
from scipy import stats

import likgrid
import model_cases as mc
import negbin_ref as nr
from conftest import assert_parity
from test_negbin_cpu import KIND, assert_grid, bulk_rows, c_kernel, c_kernel_vs_float64, load_grid

pytestmark = pytest.mark.gpu

NB = ("NegBinomial", {})
LIK_ID = 11


@pytest.fixture(scope="module", autouse=True)
def negbin_in_the_oracle():
    """tests/negbin_ref.py as the oracle's contract module of the family, its id, and dim_f = 2 -- undone at teardown."""
    from oracle import likelihoods_oracle as lo
    patch = pytest.MonkeyPatch()
    patch.setitem(lo._CONTRACT, "NegBinomial", nr)
    patch.setitem(lo.LIK_IDS, "NegBinomial", LIK_ID)
    dim_f = lo.dim_f
    patch.setattr(lo, "dim_f", lambda name, K=None: 2 if name == "NegBinomial" else dim_f(name, K))
    yield
    patch.undo()


def _gpu_var_exp(y, m, v):
    from hetmogp_amd.engine import var_exp
    return likgrid.pack(*var_exp("NegBinomial", y, m, v), len(y))


# ------------------------------------------------------------------------------------------------ the row kernel
def test_var_exp_on_the_high_precision_grid():
    """Every element of every row within C_KERNEL = max(16, 4 C_ORACLE) of its class and kind; no exceptions list."""
    g = load_grid()
    got = _gpu_var_exp(g["y"], g["m"], g["v"])
    assert np.all(np.isfinite(got))
    assert_grid(g, got, c_kernel(), "kernel on nbgrid")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_var_exp_wave_and_block_tails(N):
    """N rows of the grid in one call (one wave per row, four rows per block): the tails of the wave / block grid."""
    g = load_grid()
    rows = (np.arange(N) * 7 + N) % len(g["y"])
    got = _gpu_var_exp(g["y"][rows], g["m"][rows], g["v"][rows])
    assert_grid(g, got, c_kernel(), "kernel on %d rows of nbgrid" % N, rows)


def test_var_exp_matches_restatement_on_seeded_bulk_rows():
    """3000 bulk rows, y ~ NB at the row's mean parameters: kernel and float64 restatement each sit within their own bulk constant of
    the true value in units of 2^-52 S (S from the restatement), so they differ by at most the sum of the two."""
    from hetmogp_amd import NegBinomial
    y, m, v = bulk_rows(np.random.RandomState(5), 3000)
    got, want = _gpu_var_exp(y, m, v), likgrid.pack(*nr.var_exp(y, m, v), len(y))
    likgrid.assert_rows(got, want, nr.var_exp_scale(y, m, v), np.zeros(got.shape, np.uint8), KIND, np.zeros(len(y), np.uint8),
                        c_kernel_vs_float64(), "kernel against negbin_ref, 3000 bulk rows")
    assert np.array_equal(NegBinomial().var_exp(y[:100], m[:100], v[:100])[:, 0], got[:100, 0])   # the descriptor runs the same kernel


# ------------------------------------------------------------------------------------------------ predictive, sample, log predictive
def test_predictive_closed_form():
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import NegBinomial
    rng = np.random.RandomState(5)
    N = 300
    m = rng.uniform(-3.0, 4.0, (N, 2))
    v = 10.0 ** rng.uniform(-6.0, 0.5, (N, 2))
    v[:5, 0] = 0.0
    mean, var = predictive("NegBinomial", m, v)
    wm, wv = nr.predictive(m, v)
    assert mean.shape == (N, 1) and var.shape == (N, 1)
    assert np.allclose(mean, wm, rtol=1e-12, atol=0) and np.allclose(var, wv, rtol=1e-12, atol=0)
    m2, v2 = NegBinomial().predictive(m, v)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    mean, var = predictive("NegBinomial", np.array([[800.0, 0.0]]), np.array([[1.0, 1.0]]))    # overflow is +inf, not clipped
    assert np.isposinf(mean[0, 0]) and np.isposinf(var[0, 0])


def test_sample_moments():
    """2e5 draws at three (f0, f1): sample mean and variance within 5 standard errors of mu and mu + mu^2 / r; se(mean) = sqrt(var / N),
    se(variance) = var sqrt((excess kurtosis + 2) / N).  The third point has r < 1: the boost branch of the Gamma sampler."""
    from hetmogp_amd.engine import sample
    from hetmogp_amd import NegBinomial
    N = 200000
    for seed, (f0, f1) in enumerate(((1.0, 0.5), (3.0, 2.0), (0.5, -1.0))):
        y = sample("NegBinomial", np.tile([[f0, f1]], (N, 1)), seed=500 + seed)[:, 0]
        assert y.shape == (N,) and np.all(np.isfinite(y)) and np.all(y >= 0.0) and np.all(y == np.floor(y))
        mu, vr = nr.moments(f0, f1)
        r = np.exp(f1)
        kurt = float(stats.nbinom(r, r / (r + mu)).stats("k"))
        zm, zv = abs(y.mean() - mu) / np.sqrt(vr / N), abs(y.var() - vr) / (vr * np.sqrt((kurt + 2.0) / N))
        print("sample f = (%.1f, %.1f): |mean - mu| / se = %.2f, |variance - .| / se = %.2f" % (f0, f1, zm, zv))
        assert zm <= 5.0 and zv <= 5.0, (f0, f1, zm, zv)
    ys = NegBinomial().samples(np.zeros((50, 2)), seed=5)
    assert ys.shape == (50, 1) and np.all(ys == np.floor(ys))


def test_log_predictive_at_vanishing_variance():
    """v = 0: every Monte-Carlo sample is f = m, so the per-row log predictive is log p(y | m) exactly."""
    from hetmogp_amd.engine import log_predictive_rows
    from hetmogp_amd import NegBinomial
    rng = np.random.RandomState(11)
    N = 500
    y, m, _ = bulk_rows(rng, N)
    m[:50, 1] = rng.uniform(15.0, 25.0, 50)                                     # r up to the clip: the stable G in the sampler's log p
    y[:25] += 40.0                                                              # ... on both sides of y = 32
    v = np.zeros_like(m)
    got = log_predictive_rows("NegBinomial", y, m, v, num_samples=128, seed=4)
    want = nr.logpdf_and_derivatives(y, m[:, 0], m[:, 1])[0]
    assert got.shape == (N,) and np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10
    lp = NegBinomial().log_predictive(y[:, None], m, v, 64, seed=1)
    assert abs(lp - want.sum() / 64.0) < 1e-10 * abs(want.sum() / 64.0)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [-1.0, 2.5, float("nan"), float("inf")], ids=["negative", "fraction", "nan", "inf"])
def test_observations_that_are_no_counts_are_refused(bad):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    good = np.array([0.0, 3.0, 7.0])
    y = good.copy()
    y[1] = bad
    m, v, X = np.zeros((3, 2)), np.ones((3, 2)), np.linspace(0, 1, 3)[:, None]
    e = Engine([NB], 1, 8, 1)
    e.set_data([X], [good])
    for call in (lambda: var_exp("NegBinomial", y, m, v), lambda: log_predictive_rows("NegBinomial", y, m, v, num_samples=8),
                 lambda: e.set_data([X[:2]], [y[:2]])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "NegBinomial" in str(ei.value)
    assert e.N[0] == 3                                                           # refused before the task's state changed
    assert np.all(np.isfinite(var_exp("NegBinomial", good, m, v)[0]))            # a valid call right after succeeds
    e.close()


def test_the_family_has_no_parameters_of_its_own():
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp_dparam
    with pytest.raises(_lib.InvalidArgument) as ei:
        var_exp_dparam("NegBinomial", np.array([1.0, 2.0]), np.zeros((2, 2)), np.ones((2, 2)))
    assert "no parameters of its own" in str(ei.value)
    e = Engine([NB], 1, 8, 1)
    assert e.lik_param_count(0) == 0
    e.close()


# ------------------------------------------------------------------------------------------------ whole model vs oracle
SET_N = [NB]
SET_GNB = [("Gaussian", {"sigma": 0.5}), NB, ("Bernoulli", {})]
SET_NCH = [NB, ("Categorical", {"K": 3}), ("HetGaussian", {})]
SET_MIX = [NB, ("Student", {"deg_free": 4.0}), ("Ordinal", {"K": 4}), ("Dirichlet", {"K": 3})]


def _case(seed, specs, Ns, M, Q, P):
    """model_cases.family_case with Gamma standing in for every Negative Binomial task; then, from RandomState(seed + 2) in task
    order, its observations are replaced by counts with mean 3 and size 2, and the problem is made for the real specs."""
    from oracle import svmogp_oracle as so
    prm, _, X, Y = mc.family_case(seed, [("Gamma", {}) if s == NB else s for s in specs], Ns, M, Q, P)
    rng = np.random.RandomState(seed + 2)
    for t, s in enumerate(specs):
        if s == NB:
            Y[t] = rng.poisson(3.0 * rng.gamma(2.0, 0.5, (Ns[t], 1))).astype(float)
    return prm, so.make_problem(specs, Q, M, P), X, Y


SHAPES = [(16, 1, 1), (100, 3, 1), (128, 3, 2), (256, 1, 2)]
CASES = [(s, M, Q, P) for s in (SET_N, SET_GNB, SET_NCH) for M, Q, P in SHAPES]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n for n, _ in c[0]), c[1], c[2], c[3]) for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    Ns = [300, 257, 129][:len(specs)]
    mc.check_vs_oracle(_case(3100 + M + 7 * Q + P, specs, Ns, M, Q, P), Ns)


def test_small_model_path_carries_negbinomial():
    """M = 48: the family's singleton instantiation of quad_multi_kernel and the captured graph, against the regular kernels."""
    Ns = [300, 257, 129]
    mc.check_small_vs_regular(_case(377, SET_GNB, Ns, 48, 2, 1), Ns, ([60, 50, 20], [160, 137, 129]))


def test_strict_qf_with_negbinomial_vs_literal_oracle():
    mc.check_strict_vs_literal(_case(331, SET_NCH, [400, 300, 257], 128, 2, 1))


@pytest.mark.parametrize("M", [16, 128])
def test_mixed_with_the_other_table_families(M):
    """Negative Binomial, Student, Ordinal and Dirichlet(3) in one model: a set outside the baseline masks, so launch_quad_multi takes its
    generic path with the four singleton instantiations behind each other."""
    from oracle import svmogp_oracle as so
    Ns = [300, 257, 129, 200]
    prm, prob, X, Y = _case(3500 + M, SET_MIX, Ns, M, 2, 1)
    want = so.elbo_grad_fused(prm, prob, X, Y)
    e = mc.make_engine(prob, X, Y)
    mc._parity(mc.run(e, prm), want, "mixed M = %d " % M)
    e.close()


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed):
    rng = np.random.RandomState(seed)
    Xc, Xb = np.sort(rng.rand(400, 1), 0), np.sort(rng.rand(300, 1), 0)
    mu = np.exp(1.0 + 1.2 * np.sin(2.0 * np.pi * Xc))
    r = np.exp(0.5 + np.cos(2.0 * np.pi * Xc))
    Yc = rng.poisson(mu * rng.gamma(r) / r).astype(float)
    Yb = (rng.rand(300, 1) < 1.0 / (1.0 + np.exp(-3.0 * np.cos(4.0 * Xb)))).astype(float)
    return [Xc, Xb], [Yc, Yb]


def _model_prm(model):
    return dict(Z=model.Z.values, m_u=model.q_u_means.values, L_flat=model.q_u_chols.values,
                variance=np.array([float(k.variance[0]) for k in model.kern_list]),
                lengthscale=np.array([float(k.lengthscale[0]) for k in model.kern_list]),
                W=np.stack([np.ravel(B.W.values) for B in model.B_list]), kappa=np.stack([np.ravel(B.kappa.values) for B in model.B_list]))


def test_facade_negbinomial_and_bernoulli_end_to_end():
    import hetmogp_amd as H
    from oracle import svmogp_oracle as so
    X, Y = _toy(21)
    likelihood = H.HetLikelihood([H.NegBinomial(), H.Bernoulli()])
    md = likelihood.generate_metadata()
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.array([0.9, 0.1, 0.5])[:, None], np.array([0.1, 0.9, 0.5])[:, None]]
    np.random.seed(0)
    model = H.HetMOGP(X=X, Y=Y, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list)
    model.parameters_changed()
    prm = _model_prm(model)
    want = so.elbo_grad_fused(prm, so.make_problem(likelihood.specs(), Q, M, 1), X, Y)
    assert_parity(model.log_likelihood(), want["elbo"], "elbo")
    for got, key in ((model.q_u_means.gradient, "g_m_u"), (model.q_u_chols.gradient, "g_L_u"), (model.Z.gradient, "g_Z"),
                     ([k.variance.gradient[0] for k in model.kern_list], "g_variance"),
                     ([k.lengthscale.gradient[0] for k in model.kern_list], "g_lengthscale"),
                     (np.stack([B.W.gradient.ravel() for B in model.B_list]), "g_W"),
                     (np.stack([B.kappa.gradient.ravel() for B in model.B_list]), "g_kappa")):
        assert_parity(np.asarray(got, float).reshape(np.shape(want[key])), want[key], key)
    e0 = float(model.log_likelihood()[0, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (the optimiser view's Logexp inverse of kappa = 0 is log(0): not this family's)
        model.optimize(max_iters=30)
    e1 = float(model.log_likelihood()[0, 0])
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    Xp = [np.linspace(0, 1, 37)[:, None]] * 2
    mean, var = model.predictive(Xp)
    assert all(np.all(np.isfinite(a)) for a in mean + var) and mean[0].shape == (37, 1)
    assert np.all(var[0] > mean[0]) and np.all(mean[0] > 0.0)                     # over-dispersed: the variance exceeds the mean
    nlpd = model.negative_log_predictive([x[:50] for x in X], [y[:50] for y in Y], num_samples=200, seed=3)
    assert np.isfinite(nlpd)


# ------------------------------------------------------------------------------------------------ the split step
def test_split_step_equals_the_plain_call_bit_for_bit():
    """hmogp_step_begin / hmogp_step_finish on one rank: the bundle carries nothing family-specific."""
    specs = [("Gaussian", {"sigma": 0.5}), NB]
    Ns = [300, 257]
    prm, prob, X, Y = _case(41, specs, Ns, 64, 2, 1)
    e = mc.make_engine(prob, X, Y, small_path=False)             # (a split step always takes the regular kernels)
    full = mc.run(e, prm)
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"], W=prm["W"],
                kappa=prm["kappa"])
    e.step_begin(**args)
    out = e.step_finish()
    for k in mc.KEYS:
        assert np.array_equal(np.asarray(out[k]), np.asarray(full[k])), k
    e.close()
