"""GPU: the Ordinal (ordered probit) likelihood of DESIGN 9b through every layer -- the quadrature against the high-precision grid
tests/golden/ordgrid.npz (criterion and constants: tests/test_ordinal_cpu.py) and against the float64 restatement
oracle/lik_ordinal.py, the closed-form predictive, sampling statistics, the Monte-Carlo log predictive, the refusal of invalid
tables / ids / labels, the whole ELBO + gradient against the oracle (the checks of tests/model_cases.py) on the
default, several-pool, minibatch, small-model and strict q(f) paths, and the model facade end to end.

Kernel bounds = max(16, 4 C_ORACLE) of tests/test_ordinal_cpu.py: bulk 32 / 32 / 32, edge 2^19 / 2048 / 2048 (ve / dm / dv),
predictive 16 / 16.  Measured on one MI355X, 2026-10-16, largest |got - R| / (2^-52 S):
    bulk   6.15 / 6.12 / 6.23          edge   4.34e4 / 332 / 331          predictive (mean, variance)   1.13 / 0.87
no non-finite element, no exception list.  Facade: held-out MAE ratio model / training-median label 0.233."""
import warnings

import numpy as np
import pytest

import likgrid
import model_cases as mc
import test_ordinal_cpu as oc
from oracle import lik_ordinal

pytestmark = pytest.mark.gpu

EDGES = {2: [0.3], 3: [-0.8, 0.45], 5: [-2.0, -0.9, 0.1, 1.7], 11: [-4.0, -3.1, -2.5, -1.2, -0.9, 0.0, 0.4, 1.5, 2.6, 2.9]}


def _gpu_var_exp(y, m, v, **kw):
    from hetmogp_amd.engine import var_exp
    return var_exp("Ordinal", y, m, v, **kw)


# ------------------------------------------------------------------------------------------------ building blocks
def test_var_exp_on_the_high_precision_grid():
    g = oc.load_grid()
    got = oc.evaluate(g, _gpu_var_exp)
    assert np.all(np.isfinite(got))                    # the contract: finite inputs, finite outputs -- no row is marked non-finite
    likgrid.assert_rows(got, g["R"], g["S"], np.zeros(got.shape, np.uint8), oc.KIND, g["cls"], oc.c_kernel(), "Ordinal kernel on ordgrid")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 10000])
@pytest.mark.parametrize("K", [2, 3, 5, 11])
def test_var_exp_matches_restatement(K, N):
    """Bulk-range rows (m in [-3, 3] sigma, v in [1e-3, 4] sigma^2, bins of 0.3 ... 1.6 sigma).  Kernel and restatement each sit
    within their own bulk constant of the true value, so the two constants add (the rule of likgrid.c_kernel_vs_float64); the
    condition scale S of these rows is the restatement's float64 one (lik_ordinal.var_exp_scale)."""
    C = np.array(oc.c_kernel()[oc.BULK]) + np.array(oc.C_ORACLE[oc.BULK])
    for sigma in (0.3, 1.0, 4.0):
        rng = np.random.RandomState(K * 1009 + N + int(10 * sigma))
        e = np.array(EDGES[K]) * sigma
        y = rng.randint(1, K + 1, N).astype(float)
        m, v = rng.uniform(-3.0, 3.0, N) * sigma, 10.0 ** rng.uniform(-3.0, np.log10(4.0), N) * sigma ** 2
        got = _gpu_var_exp(y, m, v, bin_edges=e, sigma=sigma)
        assert got[0].shape == (N,) and got[1].shape == (N, 1) and got[2].shape == (N, 1)
        got = likgrid.pack(*got, N)
        want = likgrid.pack(*lik_ordinal.var_exp(y, m, v, bin_edges=e, sigma=sigma), N)
        r = np.abs(got - want) / (likgrid.EPS * lik_ordinal.var_exp_scale(y, m, v, bin_edges=e, sigma=sigma))
        assert np.all(np.isfinite(got)) and np.all(r <= C[None, :]), (K, N, sigma, r.max(0))
    from hetmogp_amd import Ordinal
    lik = Ordinal(bin_edges=e, sigma=sigma)
    assert np.array_equal(lik.var_exp(y, m, v)[:, 0], got[:, 0])
    dm, dv = lik.var_exp_derivatives(y, m, v)
    assert np.array_equal(dm, got[:, 1:2]) and np.array_equal(dv, got[:, 2:3])


def test_var_exp_is_row_position_independent():
    g = oc.load_grid()
    kw, idx = max(oc.grid_groups(g), key=lambda t: len(t[1]))
    y, m, v = g["y"][idx], g["m"][idx], g["v"][idx]
    base = likgrid.pack(*_gpu_var_exp(y, m, v, **kw), len(idx))
    rng = np.random.RandomState(0)
    for shift in (1, 63, 64, 257):
        perm = rng.permutation(len(idx))
        pad = np.concatenate([np.arange(shift) % len(idx), perm])
        out = likgrid.pack(*_gpu_var_exp(y[pad], m[pad], v[pad], **kw), len(pad))
        assert np.array_equal(out[shift:], base[perm]), shift


def test_predictive_against_high_precision_closed_form():
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import Ordinal
    g = oc.load_grid()
    got = np.empty((len(g["p_m"]), 2))
    for kw, idx in oc.grid_groups(g, "p_"):
        mean, var = predictive("Ordinal", g["p_m"][idx], g["p_v"][idx], **kw)
        assert mean.shape == (len(idx), 1) and var.shape == (len(idx), 1)
        got[idx] = np.concatenate([mean, var], 1)
        m2, v2 = Ordinal(**kw).predictive(g["p_m"][idx][:, None], g["p_v"][idx][:, None])
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)
        assert np.array_equal(predictive("Ordinal", g["p_m"][idx], g["p_v"][idx], gh_T=10, **kw)[0], mean)     # gh_T is ignored
    r = np.abs(got - g["p_R"]) / (likgrid.EPS * g["p_S"])
    print("[ordgrid] predictive kernel, worst |got - R| / (2^-52 S): mean %.3g variance %.3g" % tuple(r.max(0)))
    assert np.all(np.isfinite(got)) and np.all(r <= np.array(oc.c_kernel_pred())), r.max(0)


def test_sample_class_frequencies():
    """2e6 draws: every class frequency within 5 standard errors of the closed-form probability -- binomial at one f, and the
    Poisson-binomial sqrt(sum_n p_n (1 - p_n)) / N for rows whose f sweeps the whole range of the cut points (there every class
    of K = 11 expects thousands of draws, so the normal bound means something for each)."""
    from hetmogp_amd.engine import sample
    from hetmogp_amd import Ordinal
    N = 2000000
    for K, sigma, f in ((5, 1.0, 0.3), (2, 4.0, 1.0), (3, 0.3, 0.0), (2, 1.0, None), (3, 0.3, None), (5, 1.0, None), (11, 0.7, None)):
        e = np.array(EDGES[K])
        F = np.full(N, f) if f is not None else np.linspace(e[0] - 2.0 * sigma, e[-1] + 2.0 * sigma, N)
        y = sample("Ordinal", F[:, None], seed=100 + K, bin_edges=e, sigma=sigma)[:, 0]
        assert y.shape == (N,) and np.array_equal(y, np.round(y)) and y.min() >= 1 and y.max() <= K
        Fp = F if f is None else F[:1]                                  # (in slices: no N x K x several temporaries at once)
        P = np.concatenate([lik_ordinal.class_probs(Fp[i:i + 100000], np.zeros(len(Fp[i:i + 100000])), bin_edges=e, sigma=sigma)
                            for i in range(0, len(Fp), 100000)])
        p, se = P.mean(0), np.sqrt((P * (1.0 - P)).mean(0) / N)
        assert np.all(N * p >= 1000.0)                                  # the normal bound applies to every class
        freq = np.bincount(y.astype(int), minlength=K + 1)[1:] / N
        print("sample K = %d sigma = %g: worst |freq - p| / se = %.2f" % (K, sigma, np.max(np.abs(freq - p) / se)))
        assert np.all(np.abs(freq - p) <= 5.0 * se), (K, freq, p, se)
    y = Ordinal(K=5).samples(np.linspace(-3, 3, 50)[:, None], seed=5)
    assert y.shape == (50, 1) and y[0, 0] <= y[-1, 0]


def test_log_predictive():
    from hetmogp_amd.engine import log_predictive_rows
    rng = np.random.RandomState(11)
    N = 400
    for K, sigma in ((2, 1.0), (5, 0.3), (11, 4.0)):
        e = np.array(EDGES[K]) * sigma
        y = rng.randint(1, K + 1, N).astype(float)
        m = rng.uniform(-40.0, 40.0, N) * sigma                       # far tails included: un-clipped log p
        y0 = y
        got = log_predictive_rows("Ordinal", y, m, np.zeros(N), num_samples=128, seed=4, bin_edges=e, sigma=sigma)
        want = lik_ordinal.logpdf(y, m, bin_edges=e, sigma=sigma)     # v = 0: every sample is f = m
        assert np.all(np.isfinite(got)) and np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10, (K, sigma)
        # v > 0: within 5 Monte-Carlo standard errors (from the restatement's own samples) of the closed form log P_y(m, v)
        # (labels drawn from the closed-form probabilities, so that the estimator's own distribution is not a rare-event one)
        m2, v2 = rng.uniform(-2.5, 2.5, N) * sigma, 10.0 ** rng.uniform(-2.0, 0.0, N) * sigma ** 2
        cum = np.cumsum(lik_ordinal.class_probs(m2, v2, bin_edges=e, sigma=sigma), 1)
        y = np.minimum(1 + (rng.rand(N, 1) > cum).sum(1), K).astype(float)
        S = 16384
        got = log_predictive_rows("Ordinal", y, m2, v2, num_samples=S, seed=9, bin_edges=e, sigma=sigma)
        closed = lik_ordinal.log_prob(y, m2, v2, bin_edges=e, sigma=sigma)
        _, se = lik_ordinal.log_predictive_rows(y, m2, v2, S, np.random.RandomState(1), bin_edges=e, sigma=sigma)
        assert np.all(np.abs(got - closed) <= 5.0 * se + 1e-12), (K, sigma, np.max(np.abs(got - closed) / se))
    from hetmogp_amd import Ordinal
    lp = Ordinal(bin_edges=e, sigma=sigma).log_predictive(y0[:, None], m[:, None], np.zeros((N, 1)), 64, seed=1)
    assert abs(lp - want.sum() / 64.0) < 1e-10 * abs(want.sum() / 64.0)


def _entry_points(param, N=4):
    """The five entry points that take a table id, as calls."""
    from hetmogp_amd.engine import Engine, var_exp, predictive, sample, log_predictive_rows
    y, m, v = np.ones(N), np.zeros((N, 1)), np.ones((N, 1))
    return (lambda: var_exp("Ordinal", y, m, v, **param), lambda: predictive("Ordinal", m, v, **param),
            lambda: sample("Ordinal", m, seed=0, **param), lambda: log_predictive_rows("Ordinal", y, m, v, num_samples=8, **param),
            lambda: Engine([("Gaussian", {}), ("Ordinal", dict(param))], 1, 8, 1).close())


INF, NAN = float("inf"), float("nan")
BAD_TABLES = [dict(K=1), dict(K=33), dict(bin_edges=[]), dict(bin_edges=[0.0, 0.0]), dict(bin_edges=[1.0, -1.0]),
              dict(bin_edges=[0.0, INF]), dict(bin_edges=[NAN, 1.0]), dict(K=3, sigma=0.0), dict(K=3, sigma=-2.0),
              dict(K=3, sigma=INF), dict(K=3, sigma=NAN), dict(table_id=0.0), dict(table_id=1e9), dict(table_id=1.5),
              dict(table_id=-1.0), dict(table_id=NAN)]


@pytest.mark.parametrize("param", BAD_TABLES, ids=[str(p) for p in BAD_TABLES])
def test_invalid_table_is_refused_everywhere_and_the_device_stays_usable(param):
    from hetmogp_amd import _lib
    good = dict(K=4, sigma=0.5)
    for bad, ok in zip(_entry_points(param), _entry_points(good)):
        with pytest.raises(_lib.InvalidArgument) as ei:
            bad()
        assert "Ordinal" in str(ei.value)
        ok()                                                           # a valid call right after succeeds


@pytest.mark.parametrize("label", [0.0, 5.0, 2.5, -1.0, NAN, INF])
def test_label_outside_the_classes_is_refused(label):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    y, m, v = np.array([1.0, label, 4.0]), np.zeros((3, 1)), np.ones((3, 1))
    e = Engine([("Ordinal", {"K": 4})], 1, 8, 1)
    for call in (lambda: var_exp("Ordinal", y, m, v, K=4), lambda: log_predictive_rows("Ordinal", y, m, v, num_samples=8, K=4),
                 lambda: e.set_task_data(0, np.linspace(0, 1, 3)[:, None], y)):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "label" in str(ei.value)
    e.set_task_data(0, np.linspace(0, 1, 3)[:, None], np.array([1.0, 2.0, 4.0]))
    e.close()


# ------------------------------------------------------------------------------------------------ whole model vs oracle
ORD5 = ("Ordinal", {"K": 5, "bin_edges": EDGES[5], "sigma": 0.8})
ORD3 = ("Ordinal", {"K": 3, "bin_edges": EDGES[3], "sigma": 0.3})
ORD11 = ("Ordinal", {"K": 11})
SET_O = [ORD5]
SET_GOB = [("Gaussian", {"sigma": 0.5}), ORD5, ("Bernoulli", {})]
SET_OCG = [ORD11, ("Categorical", {"K": 3}), ("Gaussian", {"sigma": 0.7})]
SET_OO = [ORD3, ORD5]


CASES = [(SET_O, 16, 1, 1), (SET_GOB, 16, 3, 1), (SET_OCG, 100, 3, 1), (SET_GOB, 100, 1, 2), (SET_O, 128, 3, 2),
         (SET_OCG, 128, 1, 1), (SET_GOB, 256, 3, 1), (SET_OO, 256, 2, 1)]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n for n, _ in c[0]), c[1], c[2], c[3])
                                                     for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    Ns = [300, 257, 129][:len(specs)]
    mc.check_vs_oracle(mc.family_case(1900 + M + 7 * Q + P, specs, Ns, M, Q, P), Ns)


@pytest.mark.parametrize("specs", [SET_GOB, SET_OO], ids=["Gaussian+Ordinal+Bernoulli", "two-Ordinal-segments"])
def test_small_model_path_carries_ordinal(specs):
    """All segments in one quad_multi_kernel pass; the second set is two Ordinal segments with different tables."""
    n = len(specs)
    Ns = [300, 257, 129][:n]
    mc.check_small_vs_regular(mc.family_case(177, specs, Ns, 48, 2, 1), Ns, ([60, 50, 20][:n], [160, 137, 129][:n]))


def test_strict_qf_with_ordinal_vs_literal_oracle():
    mc.check_strict_vs_literal(mc.family_case(131, SET_OCG, [400, 300, 257], 128, 2, 1))


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed, N=500):
    """A Gaussian output and a K = 5 Ordinal output that is the binned, noisy version of a correlated latent function."""
    rng = np.random.RandomState(seed)
    lat = lambda x: 1.8 * np.sin(2.0 * np.pi * x) + 0.6 * np.cos(5.0 * x)
    edges, sigma = np.array([-1.5, -0.5, 0.5, 1.5]), 0.4
    Xg, Xo = np.sort(rng.rand(N, 1), 0), np.sort(rng.rand(N, 1), 0)
    Yg = 0.8 * lat(Xg) + 0.3 + 0.2 * rng.randn(N, 1)
    label = lambda x: (1 + (lat(x) + sigma * rng.randn(*x.shape) > edges[None, :]).sum(1, keepdims=True)).astype(float)
    Xt = np.sort(rng.rand(300, 1), 0)
    return Xg, Yg, Xo, label(Xo), Xt, label(Xt), edges, sigma


def test_facade_gaussian_and_ordinal_end_to_end():
    """The ELBO rises, and on held-out inputs the predictive mean label beats the constant "training median label" in mean
    absolute error.  Measured ratio MAE(model) / MAE(median) in DESIGN 9b; asserted: below 0.75 -- the model has to remove at least
    a quarter of the constant predictor's error (the label noise alone, sigma = 0.4 against unit bins, leaves an MAE of ~0.3
    where the median's is ~1.2, so a fitted model sits near 0.3 and an unfitted one near 1)."""
    import hetmogp_amd as H
    Xg, Yg, Xo, Yo, Xt, Yt, edges, sigma = _toy(5)
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.2), H.Ordinal(bin_edges=edges, sigma=sigma)])
    md = likelihood.generate_metadata()
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.eye(Q, 2)[q][:, None] * 0.9 + 0.1 for q in range(Q)]
    Z = np.linspace(0, 1, M)[:, None]
    np.random.seed(0)
    model = H.HetMOGP(X=[Xg, Xo], Y=[Yg, Yo], Z=Z, kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list)
    e0 = float(model.log_likelihood()[0, 0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        H.vem_algorithm(model, stochastic=False, vem_iters=2)
    caught = [w for w in caught if "K_uu is ill-conditioned" not in str(w.message)]
    assert not caught, [str(w.message) for w in caught]
    e1 = float(model.log_likelihood()[0, 0])
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    mean, var = model.predictive([Xt, Xt])
    assert mean[1].shape == (300, 1) and np.all(np.isfinite(mean[1])) and np.all(var[1] >= 0.0)
    assert np.all((mean[1] >= 1.0) & (mean[1] <= 5.0))
    mae_model = float(np.mean(np.abs(mean[1] - Yt)))
    mae_median = float(np.mean(np.abs(np.median(Yo) - Yt)))
    print("held-out MAE of the predictive mean label %.4f, of the training median label %.4f, ratio %.3f" %
          (mae_model, mae_median, mae_model / mae_median))
    assert mae_model < mae_median
    assert mae_model < 0.75 * mae_median
    nlpd = model.negative_log_predictive([Xg[:50], Xo[:50]], [Yg[:50], Yo[:50]], num_samples=200, seed=3)
    assert np.isfinite(nlpd)
