"""GPU: the heteroscedastic Student-t likelihood through every layer -- the building blocks (var_exp, predictive,
sample, log_predictive) against the NumPy restatement in oracle/lik_student.py and against closed forms, the refusal of an invalid
deg_free, the whole ELBO + gradient against the oracle (the checks of tests/model_cases.py) on the default, several-pool, minibatch,
small-model and strict q(f) paths, and the model facade end to end, including the robustness the family is for."""
import warnings

import numpy as np
import pytest
from scipy import stats

import model_cases as mc
from conftest import elementwise_excess
from oracle import lik_student

pytestmark = pytest.mark.gpu


def _rows(rng, N, r_max=50.0):
    """y, m [N, 2], v [N, 2]: residuals up to r_max (outlier regime), variances spanning 1e-6 ... 3."""
    y = rng.randn(N) * 2.0
    r = r_max * (2.0 * rng.rand(N) - 1.0) * (rng.rand(N) < 0.3) + rng.randn(N)
    m = np.stack([y - r, rng.uniform(-2.0, 1.5, N)], 1)
    v = 10.0 ** rng.uniform(-6.0, np.log10(3.0), (N, 2))
    return y, m, v


# ------------------------------------------------------------------------------------------------ building blocks
@pytest.mark.parametrize("N", [1, 63, 64, 65, 10000])
@pytest.mark.parametrize("nu", [1.0, 2.5, 5.0, 30.0])
def test_var_exp_matches_numpy_tensor_rule(nu, N):
    from hetmogp_amd.engine import var_exp
    rng = np.random.RandomState(int(10 * nu) * 100003 + N)
    y, m, v = _rows(rng, N)
    if N == 1:
        m[0, 0] = y[0] - 37.0                         # the single row is an outlier
    ve, dm, dv = var_exp("Student", y, m, v, deg_free=nu)
    want = lik_student.var_exp(y, m, v, deg_free=nu)
    for name, a, b in zip(("ve", "dm", "dv"), (ve, dm, dv), want):
        ex = elementwise_excess(a, b, rtol=1e-12, floor=1e-14)
        assert ex <= 1.0, (name, nu, N, ex)
    # the descriptor's reference-signature wrappers run the same kernel
    from hetmogp_amd import Student
    assert np.array_equal(Student(None, nu).var_exp(y, m, v)[:, 0], ve)


def test_var_exp_tends_to_het_gaussian_closed_form():
    """nu = 1e8: the family IS HetGaussian up to O(1/nu) -- checked against HetGaussian's closed form, not the restatement.
    Every entry to 1e-6 relative, except d/dm1 = (E[r^2 s] - 1) / 2, which vanishes where q(f) fits the data: it is held to
    1e-6 of its larger term, (E[r^2 s] + 1) / 2 = |dm1| + 1 at most."""
    from hetmogp_amd.engine import var_exp
    rng = np.random.RandomState(3)
    N = 2000
    y = rng.randn(N)
    m = np.stack([y + rng.uniform(-1.0, 1.0, N), rng.uniform(-1.0, 1.0, N)], 1)
    v = np.stack([rng.uniform(1e-4, 1.0, N), rng.uniform(1e-4, 0.5, N)], 1)
    (ve, dm, dv), (ve_h, dm_h, dv_h) = var_exp("Student", y, m, v, deg_free=1e8), var_exp("HetGaussian", y, m, v)
    for name, x, z in (("ve", ve, ve_h), ("dm0", dm[:, 0], dm_h[:, 0]), ("dv", dv, dv_h)):
        ex = elementwise_excess(x, z, rtol=1e-6, floor=1e-12)
        assert ex <= 1.0, (name, ex)
    assert np.all(np.abs(dm[:, 1] - dm_h[:, 1]) <= 1e-6 * (np.abs(dm_h[:, 1]) + 1.0))


def test_predictive_closed_form_and_missing_moments():
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import Student
    rng = np.random.RandomState(5)
    N = 300
    m = np.stack([rng.randn(N) * 3.0, rng.uniform(-3.0, 2.0, N)], 1)
    v = 10.0 ** rng.uniform(-6.0, 0.5, (N, 2))
    for nu in (2.5, 5.0, 30.0):
        mean, var = predictive("Student", m, v, deg_free=nu)
        wm, wv = lik_student.predictive(m, v, deg_free=nu)
        assert mean.shape == (N, 1) and var.shape == (N, 1)
        assert np.max(np.abs(mean - wm) / np.abs(wm)) <= 1e-13 and np.max(np.abs(var - wv) / wv) <= 1e-13, nu
    mean, var = predictive("Student", m, v, deg_free=2.0)             # 1 < nu <= 2: mean exists, variance does not
    assert np.array_equal(mean, m[:, :1]) and np.all(np.isposinf(var))
    for nu in (1.0, 0.5):                                              # nu <= 1: neither
        mean, var = predictive("Student", m, v, deg_free=nu)
        assert np.all(np.isnan(mean)) and np.all(np.isposinf(var))
    mean, var = Student(None, 5.0).predictive(m, v)
    assert np.array_equal(mean, m[:, :1])


def test_sample_distribution():
    from hetmogp_amd.engine import sample
    nu, N = 5.0, 2000000
    rng = np.random.RandomState(7)
    F = np.stack([rng.uniform(-3.0, 3.0, N), rng.uniform(-2.0, 1.0, N)], 1)
    y = sample("Student", F, seed=1234, deg_free=nu)[:, 0]
    assert y.shape == (N,) and np.all(np.isfinite(y))
    z = (y - F[:, 0]) / np.exp(0.5 * F[:, 1])                          # standardised: t(nu)
    var_t = nu / (nu - 2.0)
    se_mean = np.sqrt(var_t / N)
    se_var = var_t * np.sqrt((stats.t.stats(nu, moments="k") + 2.0) / N)   # sqrt((mu4 - sigma^4) / N)
    assert abs(z.mean()) < 4.0 * se_mean, (z.mean(), se_mean)
    assert abs(z.var() - var_t) < 4.0 * se_var, (z.var(), var_t, se_var)
    # heteroscedastic moments of y itself on one slice of constant f: mean f0, variance nu/(nu-2) exp(f1)
    f = np.tile([[0.7, np.log(0.5)]], (N // 4, 1))
    ys = sample("Student", f, seed=99, deg_free=nu)[:, 0]
    vs = var_t * 0.5
    assert abs(ys.mean() - 0.7) < 4.0 * np.sqrt(vs / ys.size)
    assert abs(ys.var() - vs) < 4.0 * vs * np.sqrt((stats.t.stats(nu, moments="k") + 2.0) / ys.size)
    tail = np.mean(np.abs(z) > 4.0)
    want = 2.0 * stats.t.sf(4.0, nu)
    assert abs(tail / want - 1.0) < 0.2, (tail, want)


def test_log_predictive_at_vanishing_variance():
    """v = 0: every Monte-Carlo sample is f = m, so the per-row log predictive is log p(y | m) exactly."""
    from hetmogp_amd.engine import log_predictive_rows
    from hetmogp_amd import Student
    rng = np.random.RandomState(11)
    N = 500
    y, m, _ = _rows(rng, N, r_max=30.0)
    v = np.zeros_like(m)
    for nu in (1.0, 5.0, 30.0):
        got = log_predictive_rows("Student", y, m, v, num_samples=256, seed=4, deg_free=nu)
        want = lik_student.logpdf_and_derivatives(y, m[:, 0], m[:, 1], nu)[0]
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10, nu
    lp = Student(None, 5.0).log_predictive(y[:, None], m, v, 64, seed=1)
    want = lik_student.logpdf_and_derivatives(y, m[:, 0], m[:, 1], 5.0)[0].sum() / 64.0
    assert abs(lp - want) < 1e-10 * abs(want)


@pytest.mark.parametrize("nu", [0.0, -1.0, float("nan"), float("inf")])
def test_invalid_deg_free_is_refused(nu):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, predictive, sample, log_predictive_rows
    y, m, v = np.zeros(4), np.zeros((4, 2)), np.ones((4, 2))
    for call in (lambda: var_exp("Student", y, m, v, deg_free=nu),
                 lambda: predictive("Student", m, v, deg_free=nu),
                 lambda: sample("Student", m, seed=0, deg_free=nu),
                 lambda: log_predictive_rows("Student", y, m, v, num_samples=8, deg_free=nu),
                 lambda: Engine([("Gaussian", {}), ("Student", {"deg_free": nu})], 1, 8, 1)):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "deg_free" in str(ei.value)


# ------------------------------------------------------------------------------------------------ whole model vs oracle
SET_S = [("Student", {"deg_free": 5.0})]
SET_GSB = [("Gaussian", {"sigma": 0.5}), ("Student", {"deg_free": 3.0}), ("Bernoulli", {})]
SET_SCH = [("Student", {"deg_free": 2.5}), ("Categorical", {"K": 3}), ("HetGaussian", {})]


CASES = [(SET_S, 16, 1, 1), (SET_GSB, 16, 3, 1), (SET_SCH, 100, 3, 1), (SET_GSB, 100, 1, 2), (SET_S, 128, 3, 2),
         (SET_SCH, 128, 1, 1), (SET_GSB, 256, 3, 1), (SET_SCH, 256, 1, 2)]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n for n, _ in c[0]), c[1], c[2], c[3])
                                                     for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    Ns = [300, 257, 129][:len(specs)]
    mc.check_vs_oracle(mc.family_case(900 + M + 7 * Q + P, specs, Ns, M, Q, P), Ns)


def test_small_model_path_carries_student():
    Ns = [300, 257, 129]
    mc.check_small_vs_regular(mc.family_case(77, SET_GSB, Ns, 48, 2, 1), Ns, ([60, 50, 20], [160, 137, 129]))


def test_strict_qf_with_student_vs_literal_oracle():
    mc.check_strict_vs_literal(mc.family_case(31, SET_SCH, [400, 300, 257], 128, 2, 1))


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed, N=400, outliers=0.1):
    rng = np.random.RandomState(seed)
    X = np.sort(rng.rand(N, 1), 0)
    loc = lambda x: np.sin(2.0 * np.pi * x) + 0.5 * x
    sigma = 0.2
    Y = loc(X) + sigma * rng.randn(N, 1)
    out = rng.rand(N, 1) < outliers
    Y = np.where(out, Y + 20.0 * sigma * np.sign(rng.randn(N, 1)), Y)
    return X, Y, loc


def _fit(lik, X_list, Y_list, vem_iters):
    import hetmogp_amd as H
    likelihood = H.HetLikelihood(lik)
    md = likelihood.generate_metadata()
    Q, M = 2, 12                                                        # K_uu condition ~1e2 at this lengthscale
    Df = len(md["function_index"])
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.eye(Q, Df)[q][:, None] * 0.9 + 0.1 for q in range(Q)]   # latent 0 -> the locations, latent 1 -> the scales
    Z = np.linspace(0, 1, M)[:, None]
    model = H.HetMOGP(X=X_list, Y=Y_list, Z=Z, kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list)
    e0 = float(model.log_likelihood()[0, 0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        H.vem_algorithm(model, stochastic=False, vem_iters=vem_iters)
    return model, e0, float(model.log_likelihood()[0, 0]), caught


def test_facade_student_and_bernoulli_end_to_end():
    import hetmogp_amd as H
    X, Y, _ = _toy(21, N=300)
    rng = np.random.RandomState(22)
    Xb = np.sort(rng.rand(250, 1), 0)
    Yb = (rng.rand(250, 1) < 1.0 / (1.0 + np.exp(-3.0 * np.cos(4.0 * Xb)))).astype(float)
    np.random.seed(0)
    model, e0, e1, caught = _fit([H.Student(), H.Bernoulli()], [X, Xb], [Y, Yb], vem_iters=1)
    # (the engine's K_uu conditioning notice -- DESIGN 6a -- concerns the prior once the M-step has moved the lengthscales, not
    #  the likelihood; every other warning fails the test)
    caught = [w for w in caught if "K_uu is ill-conditioned" not in str(w.message)]
    assert not caught, [str(w.message) for w in caught]
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    Xp = [np.linspace(0, 1, 37)[:, None]] * 2
    mean, var = model.predictive(Xp)
    assert all(np.all(np.isfinite(a)) for a in mean + var)
    assert mean[0].shape == (37, 1) and np.all(var[0] > 0)
    nlpd = model.negative_log_predictive([X[:50], Xb[:50]], [Y[:50], Yb[:50]], num_samples=200, seed=3)
    assert np.isfinite(nlpd)


def test_student_is_robust_to_gross_outliers():
    """10 % gross outliers at +-20 sigma: the Student model's predictive mean stays on the location function, HetGaussian's
    is pulled off it -- same data, same schedule."""
    import hetmogp_amd as H
    X, Y, loc = _toy(2024)
    Xt = np.linspace(0.02, 0.98, 200)[:, None]
    rmse = {}
    for name, lik in (("Student", H.Student()), ("HetGaussian", H.HetGaussian())):
        np.random.seed(0)
        model, e0, e1, _ = _fit([lik], [X], [Y], vem_iters=2)
        assert np.isfinite(e1) and e1 > e0, (name, e0, e1)
        mean, _ = model.predictive([Xt])
        rmse[name] = float(np.sqrt(np.mean((mean[0] - loc(Xt)) ** 2)))
    print("predictive-mean RMSE against the location function:", rmse)
    assert rmse["Student"] * 2.0 <= rmse["HetGaussian"], rmse
