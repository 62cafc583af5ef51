"""GPU: the zero-inflated Poisson likelihood through every layer -- the row kernel against the high-precision grid
tests/golden/zipgrid.npz under the criterion of DESIGN 9a and against the float64 restatement tests/zip_ref.py, the independence of a
row from its neighbours in the launch, the tie of the y >= 1 rows to the Poisson and Bernoulli kernels, predictive, the sampler, both log
predictive routines, the refusal of observations that are no counts, the whole ELBO + gradient against the oracle (the checks of
tests/model_cases.py) on the default, several-pool, minibatch, small-model and strict q(f) paths, the model facade end to end, and the
split step.

The oracle covers the family through a module-scoped fixture that registers tests/zip_ref.py with oracle.likelihoods_oracle for the
duration of this module (`oracle/` is not edited): cases are drawn by model_cases.family_case with Gamma standing in for the new task
(same dim_f), whose observations are then replaced by seeded zero-inflated counts.

Kernel figures on zipgrid.npz, worst |kernel - R| / (2^-52 S) per class and output, measured on an MI355X: see DESIGN 9n."""
import warnings

import numpy as np
import pytest

import model_cases as mc
import zip_ref as zr
from conftest import assert_parity
from test_zip_cpu import PREDICTIVE_TOL

pytestmark = pytest.mark.gpu

ZIP = ("ZIPoisson", {})
BULK, EDGE = zr.BULK, zr.EDGE


@pytest.fixture(scope="module", autouse=True)
def zipoisson_in_the_oracle():
    with zr.in_the_oracle():
        yield


def _gpu_var_exp(y, m, v):
    from hetmogp_amd.engine import var_exp
    return zr.pack(*var_exp("ZIPoisson", y, m, v))


# ------------------------------------------------------------------------------------------------ the row kernel
def test_var_exp_on_the_high_precision_grid():
    """Every element of every row within C_KERNEL = max(16, 4 C_ORACLE) of its class and output; no exceptions list."""
    g = zr.load_grid()
    got = _gpu_var_exp(g["y"], g["m"], g["v"])
    assert np.all(np.isfinite(got))
    zr.assert_grid(g, got, zr.c_kernel, "kernel on zipgrid")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_a_row_does_not_depend_on_its_neighbours(N):
    """N rows in one call, zero and positive rows interleaved (one wave per row, four rows per block: both branches within a block),
    equal the single-row calls bit for bit."""
    g = zr.load_grid()
    zero, pos = np.where(g["y"] == 0.0)[0], np.where(g["y"] > 0.0)[0]
    rows = np.where(np.arange(N) % 2 == 0, zero[(np.arange(N) * 7 + N) % len(zero)], pos[(np.arange(N) * 5 + N) % len(pos)])
    together = _gpu_var_exp(g["y"][rows], g["m"][rows], g["v"][rows])
    uniq = np.unique(rows)
    alone = {int(r): _gpu_var_exp(g["y"][[r]], g["m"][[r]], g["v"][[r]])[0] for r in uniq[:: max(1, len(uniq) // 24)]}
    for i, r in enumerate(rows):
        if int(r) in alone:
            assert np.array_equal(together[i], alone[int(r)]), (N, i, int(r))
    zr.assert_grid(g, together, zr.c_kernel, "kernel on %d rows of zipgrid" % N, rows)


def test_var_exp_matches_restatement_on_seeded_bulk_rows():
    """3000 bulk rows, y from the model at the row's mean parameters: kernel and float64 restatement each sit within their own bulk
    constant of the true value in units of 2^-52 S (S from the restatement), so they differ by at most the sum of the two."""
    from hetmogp_amd import ZIPoisson
    y, m, v = zr.bulk_rows(np.random.RandomState(5), 3000)
    assert (y == 0).sum() >= 500 and (y > 0).sum() >= 500
    got, want = _gpu_var_exp(y, m, v), zr.pack(*zr.var_exp(y, m, v))
    zr.assert_rows(got, want, zr.var_exp_scale(y, m, v), np.zeros(len(y), np.uint8), zr.c_sum, "kernel against zip_ref, 3000 bulk rows")
    assert np.array_equal(ZIPoisson().var_exp(y[:100], m[:100], v[:100])[:, 0], got[:100, 0])   # the descriptor runs the same kernel


def test_positive_rows_are_tied_to_the_poisson_and_bernoulli_kernels():
    """y >= 1: dm_0, dv_0 are the Poisson kernel's on (y, m0, v0), dm_1, dv_1 the Bernoulli kernel's on (0, m1, v1), ve the sum of the two
    ve's -- each within the sum of the two kernels' own bulk constants (Poisson (4, 4, 4), Bernoulli (4, 8, 2), times four, at
    least 16) in units of 2^-52 S: the node values are the same expressions, only the order of the 20 additions differs (wave shuffles
    against one lane's loop).  Prints whether the tie holds bit for bit."""
    import likgrid
    from hetmogp_amd.engine import var_exp
    y, m, v = zr.bulk_rows(np.random.RandomState(6), 1500)
    pos = y > 0
    y, m, v = y[pos], m[pos], v[pos]
    assert len(y) >= 300
    got = _gpu_var_exp(y, m, v)
    pve, pdm, pdv = var_exp("Poisson", y, m[:, :1], v[:, :1])
    bve, bdm, bdv = var_exp("Bernoulli", np.zeros(len(y)), m[:, 1:], v[:, 1:])
    want = np.stack([np.ravel(pve) + np.ravel(bve), np.ravel(pdm), np.ravel(bdm), np.ravel(pdv), np.ravel(bdv)], 1)
    S = zr.var_exp_scale(y, m, v)
    kp, kb = likgrid.c_kernel("Poisson")[likgrid.BULK], likgrid.c_kernel("Bernoulli")[likgrid.BULK]
    own = np.array([zr.c_kernel(BULK, o) for o in range(5)])
    bound = own + np.array([kp[0] + kb[0], kp[1], kb[1], kp[2], kb[2]])
    r = zr.ratios(got, want, S)
    print("tie of the y >= 1 rows: worst ratio per output %s; bit for bit: %s" % (" ".join("%.3g" % x for x in r.max(0)),
                                                                                  " ".join(str(bool(np.array_equal(got[:, k], want[:, k]))) for k in range(5))))
    assert np.all(r.max(0) <= bound), (r.max(0), bound)


# ------------------------------------------------------------------------------------------------ predictive, sample, log predictive
def test_predictive():
    """The kernel against the restatement (the same T-node rule: 1e-12), for gh_T in {0, 10, 20}, and against 120-node rules of the
    conditional moments at the CPU test's tolerance."""
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import ZIPoisson
    rng = np.random.RandomState(8)
    N = 200
    m = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-3.0, 3.0, N)], 1)
    v = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (N, 2)))
    v[:5] = 0.0
    for T in (0, 10, 20):
        mean, var = predictive("ZIPoisson", m, v, gh_T=T)
        wm, wv = zr.predictive(m, v, T=T or 20)
        assert mean.shape == (N, 1) and var.shape == (N, 1)
        assert np.allclose(mean, wm, rtol=1e-12, atol=0) and np.allclose(var, wv, rtol=1e-10, atol=0), T
    mean, var = predictive("ZIPoisson", m, v)
    x, w = zr.gh(120)
    lam = np.exp(x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])
    eq = (1.0 - zr.zero_prob(x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[1]) @ w
    e1, e2 = lam @ w, (lam * lam) @ w
    assert np.max(np.abs(mean[:, 0] - eq * e1) / (eq * e1)) <= PREDICTIVE_TOL
    wv = eq * (e1 + e2) - (eq * e1) ** 2
    assert np.max(np.abs(var[:, 0] - wv) / wv) <= PREDICTIVE_TOL
    m2, v2 = ZIPoisson().predictive(m, v)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    mean, var = predictive("ZIPoisson", np.array([[800.0, 0.0]]), np.array([[1.0, 1.0]]))    # overflow is +inf, not clipped
    assert np.isposinf(mean[0, 0]) and np.isposinf(var[0, 0])


def test_sample_moments():
    """2e5 draws at three (f0, f1), one with pi = 0.9: sample mean, variance and zero share within 4 standard errors of the model's;
    se(mean) = sqrt(var / N), se(variance) = sqrt((mu4 - var^2) / N) with the fourth central moment summed from the pmf, se(zero share) =
    sqrt(p0 (1 - p0) / N)."""
    from scipy import stats
    from hetmogp_amd.engine import sample
    from hetmogp_amd import ZIPoisson
    N = 200000
    for seed, (f0, f1) in enumerate(((1.0, -0.5), (3.0, 0.5), (1.5, np.log(9.0)))):
        y = sample("ZIPoisson", np.tile([[f0, f1]], (N, 1)), seed=700 + seed)[:, 0]
        assert y.shape == (N,) and np.all(np.isfinite(y)) and np.all(y >= 0.0) and np.all(y == np.floor(y))
        mu, vr, p0 = zr.moments(f0, f1)
        ks = np.arange(0, 400, dtype=float)
        pi = zr.zero_prob(f1)[1]
        pmf = (1.0 - pi) * stats.poisson.pmf(ks, np.exp(f0)) + pi * (ks == 0)
        mu4 = ((ks - mu) ** 4 * pmf).sum()
        zm, zv = abs(y.mean() - mu) / np.sqrt(vr / N), abs(y.var() - vr) / np.sqrt((mu4 - vr * vr) / N)
        zz = abs(np.mean(y == 0.0) - p0) / np.sqrt(p0 * (1.0 - p0) / N)
        print("sample f = (%.1f, %.2f): |mean - .| / se = %.2f, |variance - .| / se = %.2f, |zero share - .| / se = %.2f" % (f0, f1, zm, zv, zz))
        assert zm <= 4.0 and zv <= 4.0 and zz <= 4.0, (f0, f1, zm, zv, zz)
    ys = ZIPoisson().samples(np.zeros((50, 2)), seed=5)
    assert ys.shape == (50, 1) and np.all(ys == np.floor(ys))


def test_log_predictive_at_vanishing_variance():
    """v = 0: every Monte-Carlo sample is f = m, so the per-row log predictive is log p(y | m) exactly; so is the deterministic one."""
    from hetmogp_amd.engine import log_predictive_rows, log_predictive_density_rows
    from hetmogp_amd import ZIPoisson
    y, m, _ = zr.bulk_rows(np.random.RandomState(11), 500)
    v = np.zeros_like(m)
    want = zr.logpdf(y, m)
    got = log_predictive_rows("ZIPoisson", y, m, v, num_samples=128, seed=4)
    assert got.shape == (500,) and np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10
    got = log_predictive_density_rows("ZIPoisson", y, m, v)
    assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10
    lp = ZIPoisson().log_predictive(y[:, None], m, v, 64, seed=1)
    assert abs(lp - want.sum() / 64.0) < 1e-10 * abs(want.sum() / 64.0)


def test_log_predictive_density_on_the_grid():
    """The 20 x 20 rule against the grid's lpd block under max(16, 4 C_ORACLE) of the restatement's own lpd figures, the effective number
    of nodes against the restatement's, and gh_T = 10 against the restatement's 10 x 10 rule."""
    from hetmogp_amd.engine import log_predictive_density_rows
    g = zr.load_grid()
    y, m, v = g["y"], g["m"], g["v"]
    lpd, ess = log_predictive_density_rows("ZIPoisson", y, m, v, return_ess=True)
    zr.assert_rows(lpd, g["lpd"], zr.lpd_scale(y, m, v), g["cls"], zr.c_kernel, "kernel lpd on zipgrid", outputs=("lpd",))
    b = g["cls"] == BULK
    assert np.allclose(ess[b], zr.lpd(y[b], m[b], v[b])[1], rtol=1e-9)
    l10, e10 = log_predictive_density_rows("ZIPoisson", y[b], m[b], v[b], gh_T=10, return_ess=True)
    w10 = zr.lpd(y[b], m[b], v[b], T=10)
    zr.assert_rows(l10, w10[0], zr.lpd_scale(y[b], m[b], v[b], T=10), g["cls"][b], zr.c_sum, "kernel lpd, gh_T = 10, against zip_ref", outputs=("lpd",))
    assert np.allclose(e10, w10[1], rtol=1e-9)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("bad", [-1.0, 2.5, float("nan"), float("inf")], ids=["negative", "fraction", "nan", "inf"])
def test_observations_that_are_no_counts_are_refused(bad):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows, log_predictive_density_rows
    good = np.array([0.0, 3.0, 7.0])
    y = good.copy()
    y[1] = bad
    m, v, X = np.zeros((3, 2)), np.ones((3, 2)), np.linspace(0, 1, 3)[:, None]
    e = Engine([ZIP], 1, 8, 1)
    e.set_data([X], [good])
    for call in (lambda: var_exp("ZIPoisson", y, m, v), lambda: log_predictive_rows("ZIPoisson", y, m, v, num_samples=8),
                 lambda: log_predictive_density_rows("ZIPoisson", y, m, v), lambda: e.set_data([X[:2]], [y[:2]])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "ZIPoisson" in str(ei.value)
    assert e.N[0] == 3                                                           # refused before the task's state changed
    assert np.all(np.isfinite(var_exp("ZIPoisson", good, m, v)[0]))              # a valid call right after succeeds
    e.close()


def test_the_family_has_no_parameters_of_its_own():
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp_dparam
    with pytest.raises(_lib.InvalidArgument) as ei:
        var_exp_dparam("ZIPoisson", np.array([1.0, 0.0]), np.zeros((2, 2)), np.ones((2, 2)))
    assert "no parameters of its own" in str(ei.value)
    e = Engine([ZIP], 1, 8, 1)
    assert e.lik_param_count(0) == 0
    e.close()


# ------------------------------------------------------------------------------------------------ whole model vs oracle
SET_GZ = [("Gaussian", {"sigma": 0.5}), ZIP]
SET_MIX = [ZIP, ("NegBinomial", {}), ("Student", {"deg_free": 4.0}), ("Ordinal", {"K": 4})]


def _case(seed, specs, Ns, M, Q, P):
    """model_cases.family_case with Gamma standing in for every count task; then, from RandomState(seed + 2) in task order, their
    observations are replaced -- zero-inflated counts (40 % structural zeros, rate 3) and Gamma-Poisson counts -- and the problem is
    made for the real specs."""
    from oracle import svmogp_oracle as so
    counts = ("ZIPoisson", "NegBinomial")
    prm, _, X, Y = mc.family_case(seed, [("Gamma", {}) if s[0] in counts else s for s in specs], Ns, M, Q, P)
    rng = np.random.RandomState(seed + 2)
    for t, s in enumerate(specs):
        if s[0] == "ZIPoisson":
            Y[t] = np.where(rng.rand(Ns[t], 1) < 0.4, 0.0, rng.poisson(3.0, (Ns[t], 1))).astype(float)
        elif s[0] == "NegBinomial":
            Y[t] = rng.poisson(3.0 * rng.gamma(2.0, 0.5, (Ns[t], 1))).astype(float)
    return prm, so.make_problem(specs, Q, M, P), X, Y


@pytest.fixture
def negbin_too():
    """tests/negbin_ref.py as the oracle's contract of the Negative Binomial task of SET_MIX, undone after the test."""
    import negbin_ref as nr
    from oracle import likelihoods_oracle as lo
    patch = pytest.MonkeyPatch()
    patch.setitem(lo._CONTRACT, "NegBinomial", nr)
    patch.setitem(lo.LIK_IDS, "NegBinomial", 11)
    dim_f = lo.dim_f
    patch.setattr(lo, "dim_f", lambda name, K=None: 2 if name == "NegBinomial" else dim_f(name, K))
    yield
    patch.undo()


@pytest.mark.parametrize("M,Q,P", [(16, 1, 1), (128, 3, 2)])
def test_elbo_grad_vs_oracle_gaussian_and_zipoisson(M, Q, P):
    """Default, several-pool and minibatch runs (model_cases.check_vs_oracle)."""
    Ns = [300, 257]
    mc.check_vs_oracle(_case(4100 + M + 7 * Q + P, SET_GZ, Ns, M, Q, P), Ns)


@pytest.mark.parametrize("M,Q,P", [(16, 1, 1), (128, 3, 2)])
def test_elbo_grad_vs_oracle_mixed_with_the_other_table_families(M, Q, P, negbin_too):
    """ZIPoisson, NegBinomial, Student and Ordinal in one model: a set outside the baseline masks, so launch_quad_multi takes its generic
    path with the singleton instantiations behind each other."""
    Ns = [300, 257, 129, 200]
    mc.check_vs_oracle(_case(4500 + M + 7 * Q + P, SET_MIX, Ns, M, Q, P), Ns)


def test_small_model_path_carries_zipoisson():
    """M = 48: the family's singleton instantiation of quad_multi_kernel and the captured graph, against the regular kernels."""
    Ns = [300, 257]
    mc.check_small_vs_regular(_case(477, SET_GZ, Ns, 48, 2, 1), Ns, ([60, 50], [160, 137]))


def test_strict_qf_with_zipoisson_vs_literal_oracle():
    mc.check_strict_vs_literal(_case(431, SET_GZ, [400, 300], 128, 2, 1))


def test_split_step_equals_the_plain_call_bit_for_bit():
    """hmogp_step_begin / hmogp_step_finish on one rank: the bundle carries nothing family-specific."""
    Ns = [300, 257]
    prm, prob, X, Y = _case(41, SET_GZ, Ns, 64, 2, 1)
    e = mc.make_engine(prob, X, Y, small_path=False)             # (a split step always takes the regular kernels)
    full = mc.run(e, prm)
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"], W=prm["W"],
                kappa=prm["kappa"])
    e.step_begin(**args)
    out = e.step_finish()
    for k in mc.KEYS:
        assert np.array_equal(np.asarray(out[k]), np.asarray(full[k])), k
    e.close()


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed):
    rng = np.random.RandomState(seed)
    Xc, Xb = np.sort(rng.rand(400, 1), 0), np.sort(rng.rand(300, 1), 0)
    lam = np.exp(1.0 + 1.2 * np.sin(2.0 * np.pi * Xc))
    pi = 1.0 / (1.0 + np.exp(-2.0 * np.cos(2.0 * np.pi * Xc)))
    Yc = np.where(rng.rand(400, 1) < pi, 0.0, rng.poisson(lam)).astype(float)
    Yb = (rng.rand(300, 1) < 1.0 / (1.0 + np.exp(-3.0 * np.cos(4.0 * Xb)))).astype(float)
    return [Xc, Xb], [Yc, Yb]


def _model_prm(model):
    return dict(Z=model.Z.values, m_u=model.q_u_means.values, L_flat=model.q_u_chols.values,
                variance=np.array([float(k.variance[0]) for k in model.kern_list]),
                lengthscale=np.array([float(k.lengthscale[0]) for k in model.kern_list]),
                W=np.stack([np.ravel(B.W.values) for B in model.B_list]), kappa=np.stack([np.ravel(B.kappa.values) for B in model.B_list]))


def test_facade_zipoisson_and_bernoulli_end_to_end():
    import hetmogp_amd as H
    from oracle import svmogp_oracle as so
    X, Y = _toy(21)
    likelihood = H.HetLikelihood([H.ZIPoisson(), H.Bernoulli()])
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
    model[".*.kappa"].fix()      # kappa = 0 is -inf in the optimiser's vector (Logexp's inverse): L-BFGS-B's first step from such a start is
    with warnings.catch_warnings():   # 1e10 |g| long, where this model's rates overflow and the search gives up; the SVI drivers fix kappa too
        warnings.simplefilter("ignore", RuntimeWarning)
        model.optimize(max_iters=30)
    e1 = float(model.log_likelihood()[0, 0])
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    Xp = [np.linspace(0, 1, 37)[:, None]] * 2
    mean, var = model.predictive(Xp)
    assert all(np.all(np.isfinite(a)) for a in mean + var) and mean[0].shape == (37, 1)
    assert np.all(var[0] > mean[0]) and np.all(mean[0] > 0.0)                     # zero inflation over-disperses: the variance exceeds the mean
    Xt, Yt = _toy(22)                                                             # rows the model has not seen, from the same law
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lpd = model.log_predictive_density(Xt, Yt)
        nlpd = model.negative_log_predictive(Xt, Yt, method="quadrature")
    assert np.shape(lpd[0])[0] == 400 and np.shape(lpd[1])[0] == 300 and all(np.all(np.isfinite(a)) and np.all(np.asarray(a) <= 0.0) for a in lpd)
    assert np.isfinite(nlpd)
    with pytest.raises(NotImplementedError, match="ZIPoisson"):
        model.predict_quantiles(Xp, tasks=None)
