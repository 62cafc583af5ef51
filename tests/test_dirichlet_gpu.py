"""GPU: the Dirichlet likelihood of DESIGN 9d through every layer -- the wave-per-row quadrature against the high-precision grid
tests/golden/dirgrid.npz (criterion and constants: tests/test_dirichlet_cpu.py) and against the float64 restatement
oracle/lik_dirichlet.py, the predictive moments, sampling statistics, the Monte-Carlo log predictive, the refusal of an invalid K and of
rows off the open simplex, the whole ELBO + gradient against the oracle (the checks of tests/model_cases.py) on the
default, several-pool, minibatch, small-model, no-small-path and strict q(f) paths, and the model facade end to end.

Kernel bounds = max(16, 4 C_ORACLE) of tests/test_dirichlet_cpu.py: 16 for every class and output kind.  Measured on one MI355X,
2026-10-17, largest |got - R| / (2^-52 S), ve / dm / dv:
    bulk   0.88 / 1.71 / 1.40          edge   1.66 / 10.9 / 1.91
no non-finite element, no exception list.  Facade: held-out MAE ratio model / training-mean composition 0.553."""
import warnings

import numpy as np
import pytest
from scipy import stats

import likgrid
import model_cases as mc
import test_dirichlet_cpu as dc
from oracle import lik_dirichlet

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _gpu_var_exp(y, m, v, **kw):
    from hetmogp_amd.engine import var_exp
    return var_exp("Dirichlet", y, m, v, **kw)


def _bulk(rng, N, K, c=1.0):
    y = np.maximum(rng.dirichlet(np.full(K, c), N), 1e-300)
    return y / y.sum(1, keepdims=True), rng.uniform(-3.0, 3.0, (N, K)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, K)))


# ------------------------------------------------------------------------------------------------ building blocks
def test_var_exp_on_the_high_precision_grid():
    g = dc.load_grid()
    got = dc.evaluate(g, _gpu_var_exp)                 # (assert_grid: every element finite, no exception list)
    w = dc.assert_grid(g, got, dc.c_kernel(), "Dirichlet kernel on dirgrid")
    print("[dirgrid] Dirichlet kernel, worst |got - R| / (2^-52 S) over K = 2, 3, 4: bulk ve/dm/dv %s | edge %s" %
          (" ".join("%.3g" % a for a in w[dc.BULK]), " ".join("%.3g" % a for a in w[dc.EDGE])))


@pytest.mark.parametrize("N", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_var_exp_matches_restatement(K, N):
    """Bulk-range rows.  Four rows per block: 4 / 5 is the block edge; 100, 1000 and 10^4 nodes over 64 lanes all end in a ragged trip.
    Kernel and restatement each sit within their own bulk constant of the true value, so the two constants add (the rule of
    likgrid.c_kernel_vs_float64); the condition scale S of these rows is the restatement's float64 one."""
    C = (np.array(dc.c_kernel()[dc.BULK]) + np.array(dc.C_ORACLE[dc.BULK]))[dc.kind_of(K)]
    rng = np.random.RandomState(K * 1009 + N)
    y, m, v = _bulk(rng, N, K, (0.05, 1.0, 20.0)[N % 3])
    got = _gpu_var_exp(y, m, v, K=K)
    assert got[0].shape == (N,) and got[1].shape == (N, K) and got[2].shape == (N, K)
    got = likgrid.pack(*got, N)
    want = likgrid.pack(*lik_dirichlet.var_exp(y, m, v, K), N)
    r = np.abs(got - want) / (likgrid.EPS * lik_dirichlet.var_exp_scale(y, m, v, K))
    print("K = %d N = %d: worst |kernel - restatement| / (2^-52 S) = %.3g" % (K, N, r.max()))
    assert np.all(np.isfinite(got)) and np.all(r <= C[None, :]), (K, N, r.max(0))
    from hetmogp_amd import Dirichlet
    lik = Dirichlet(K)
    assert np.array_equal(lik.var_exp(y, m, v)[:, 0], got[:, 0])
    dm, dv = lik.var_exp_derivatives(y, m, v)
    assert np.array_equal(dm, got[:, 1:1 + K]) and np.array_equal(dv, got[:, 1 + K:])


@pytest.mark.parametrize("K", [2, 3, 4])
def test_var_exp_is_row_position_independent(K):
    g = dc.load_grid()
    idx = np.where(g["K"] == K)[0]
    y, m, v = g["y"][idx, :K], g["m"][idx, :K], g["v"][idx, :K]
    base = likgrid.pack(*_gpu_var_exp(y, m, v, K=K), len(idx))
    rng = np.random.RandomState(0)
    for shift in (1, 3, 4, 257):
        perm = rng.permutation(len(idx))
        pad = np.concatenate([np.arange(shift) % len(idx), perm])
        out = likgrid.pack(*_gpu_var_exp(y[pad], m[pad], v[pad], K=K), len(pad))
        assert np.array_equal(out[shift:], base[perm]), shift


@pytest.mark.parametrize("K,T", [(2, 20), (2, 10), (3, 20), (4, 10)])
def test_predictive_against_restatement(K, T):
    """Both sides evaluate the contract's three tensor sums in float64 with A summed in the same order.  Every addend of the mean and
    of E[(a/A)^2] is positive (S = the sum itself); the variance's scale is S = E[.] + E[(a/A)^2] + mean^2.  The bound: 64 units of
    2^-52 S (three roundings per node, up to T^K / 64 = 157 nodes per lane summed one after the other, a different order than NumPy's
    pairwise one) plus 4 x 2^-52 absolute on the variance: a_k (A - a_k) amplifies the last-place difference between the device's exp
    and NumPy's through the rounding of A, by at most 2^-52 / (A + 1) per node, and the weights sum to one."""
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import Dirichlet
    rng = np.random.RandomState(40 + K + T)
    N = 37
    m, v = rng.uniform(-3.0, 3.0, (N, K)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, K)))
    mean, var = predictive("Dirichlet", m, v, gh_T=T, K=K)
    assert mean.shape == (N, K) and var.shape == (N, K) and np.all(np.isfinite(mean)) and np.all(var > 0.0)
    wm, wv = lik_dirichlet.predictive(m, v, K, gh_T=T)
    rm = np.abs(mean - wm) / (likgrid.EPS * wm)
    Sv = wv + 2.0 * wm * wm
    rv = (np.abs(var - wv) - 4.0 * likgrid.EPS) / (likgrid.EPS * Sv)
    print("predictive K = %d T = %d: worst |kernel - restatement| / (2^-52 S): mean %.3g variance %.3g" % (K, T, rm.max(), rv.max()))
    assert np.all(rm <= 64.0) and np.all(rv <= 64.0)
    assert np.max(np.abs(mean.sum(1) - 1.0)) <= 64.0 * likgrid.EPS
    if T == 20:                                                                  # the default order, and the descriptor
        m2, v2 = Dirichlet(K).predictive(m, v)
        assert np.array_equal(m2, mean) and np.array_equal(v2, var)


def test_sample_moments():
    """2e5 draws per configuration: every part's sample mean and sample variance within 5 standard errors of a / A and
    a (A - a) / (A^2 (A + 1)).  A part is Beta(a, A - a): se(mean) = sqrt(var / N), se(variance) = var sqrt((excess kurtosis + 2) / N).
    The configurations cover shapes below 1 (the generator's boost), around 1 and large ones."""
    from hetmogp_amd.engine import sample
    from hetmogp_amd import Dirichlet
    N = 200000
    for seed, f in enumerate(([0.3, -0.5], [1.0, 0.0, -1.0], [0.5, 2.0, -1.0, 0.0], [-3.0, -2.0, -2.5], [4.0, 3.0, 5.0, 3.5], [-1.0, 3.0])):
        K = len(f)
        Y = sample("Dirichlet", np.tile(np.array(f), (N, 1)), seed=300 + seed, K=K)
        assert Y.shape == (N, K) and np.all(np.isfinite(Y)) and np.all(Y >= 0.0) and np.max(np.abs(Y.sum(1) - 1.0)) < 1e-12
        mu, vr = lik_dirichlet.moments(np.array(f))
        a = lik_dirichlet.alpha_of(np.array(f))
        kurt = np.array([float(stats.beta(ak, a.sum() - ak).stats("k")) for ak in a])
        zm = np.abs(Y.mean(0) - mu) / np.sqrt(vr / N)
        zv = np.abs(Y.var(0) - vr) / (vr * np.sqrt((kurt + 2.0) / N))
        print("sample f = %s: worst |mean - a/A| / se = %.2f, worst |variance - .| / se = %.2f" % (f, zm.max(), zv.max()))
        assert np.all(zm <= 5.0) and np.all(zv <= 5.0), (f, zm, zv)
    # all shapes at the lower clip: every draw is a vertex (the limit of the distribution), each with probability 1 / K
    Y = sample("Dirichlet", np.full((N, 3), -30.0), seed=9, K=3)
    assert np.all(np.isfinite(Y)) and np.all((Y == 0.0) | (Y == 1.0)) and np.all(Y.sum(1) == 1.0)
    assert np.all(np.abs(Y.mean(0) - 1.0 / 3.0) <= 5.0 * np.sqrt(2.0 / 9.0 / N))
    y = Dirichlet(3).samples(np.zeros((50, 3)), seed=5)
    assert y.shape == (50, 3) and np.allclose(y.sum(1), 1.0)


def test_log_predictive():
    from hetmogp_amd.engine import log_predictive_rows
    from hetmogp_amd import Dirichlet
    rng = np.random.RandomState(11)
    N = 200
    for K in (2, 3, 4):
        y, m, _ = _bulk(rng, N, K)
        m = rng.uniform(-25.0, 25.0, (N, K))                                   # both clips of alpha included
        got = log_predictive_rows("Dirichlet", y, m, np.zeros((N, K)), num_samples=128, seed=4, K=K)
        want = lik_dirichlet.logpdf(y, m)                                      # v = 0: every sample is f = m
        assert got.shape == (N,) and np.all(np.isfinite(got))
        assert np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10, K
        # v > 0: the kernel's estimate and the restatement's are two independent Monte-Carlo estimates of the same number from S
        # samples each, so they differ by less than 5 standard errors of their difference, sqrt 2 times the restatement's own
        # (observations drawn from the model at a draw of f, so that neither estimator is a rare-event one)
        m2, v2 = rng.uniform(-1.5, 1.5, (N, K)), 10.0 ** rng.uniform(-2.0, -0.5, (N, K))
        y2 = np.maximum(lik_dirichlet.samples(m2 + np.sqrt(v2) * rng.randn(N, K), rng), 1e-12)
        y2 = y2 / y2.sum(1, keepdims=True)
        S = 8192
        got = log_predictive_rows("Dirichlet", y2, m2, v2, num_samples=S, seed=9, K=K)
        est, se = lik_dirichlet.log_predictive_rows(y2, m2, v2, S, np.random.RandomState(1), K)
        z = np.abs(got - est) / (np.sqrt(2.0) * se)
        print("log predictive K = %d: worst |kernel - restatement| / se of the difference = %.2f" % (K, z.max()))
        assert np.all(np.abs(got - est) <= 5.0 * np.sqrt(2.0) * se + 1e-12), (K, z.max())
    lp = Dirichlet(K).log_predictive(y, m, np.zeros((N, K)), 64, seed=1)
    assert abs(lp - want.sum() / 64.0) < 1e-10 * abs(want.sum() / 64.0)


# ------------------------------------------------------------------------------------------------ refusals
def _entry_points(K, N=4):
    from hetmogp_amd.engine import Engine, var_exp, predictive, sample, log_predictive_rows
    k = max(int(K), 1)
    y, m, v = np.full((N, k), 1.0 / k), np.zeros((N, k)), np.ones((N, k))
    return (lambda: var_exp("Dirichlet", y, m, v, K=K), lambda: predictive("Dirichlet", m, v, K=K),
            lambda: sample("Dirichlet", m, seed=0, K=K), lambda: log_predictive_rows("Dirichlet", y, m, v, num_samples=8, K=K),
            lambda: Engine([("Gaussian", {}), ("Dirichlet", {"K": K})], 1, 8, 1).close())


@pytest.mark.parametrize("K", [1, 5])
def test_invalid_k_is_refused_everywhere_and_the_device_stays_usable(K):
    from hetmogp_amd import _lib
    for bad, ok in zip(_entry_points(K), _entry_points(3)):
        with pytest.raises(_lib.InvalidArgument):
            bad()
        ok()                                                           # a valid call right after succeeds


def test_fractional_k_is_refused():
    from hetmogp_amd import _lib
    y, m, v = np.full((4, 2), 0.5), np.zeros((4, 2)), np.ones((4, 2))
    with pytest.raises(_lib.InvalidArgument) as ei:
        _lib.check(_lib.lib.hmogp_var_exp(0, _lib.LIK_DIRICHLET, 2.5, 4, y.ctypes.data_as(_lib.c_double_p), m.ctypes.data_as(_lib.c_double_p),
                                          v.ctypes.data_as(_lib.c_double_p), np.zeros(4).ctypes.data_as(_lib.c_double_p),
                                          np.zeros((4, 2)).ctypes.data_as(_lib.c_double_p), np.zeros((4, 2)).ctypes.data_as(_lib.c_double_p)))
    assert "Dirichlet" in str(ei.value)


BAD_ROWS = {"zero": [0.0, 0.4, 0.6], "negative": [-0.1, 0.5, 0.6], "nan": [NAN, 0.5, 0.5], "inf": [float("inf"), 0.5, 0.5],
            "sum": [0.2, 0.3, 0.5 + 1e-3]}


@pytest.mark.parametrize("row", list(BAD_ROWS), ids=list(BAD_ROWS))
def test_row_off_the_open_simplex_is_refused(row):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    good = np.array([[0.2, 0.3, 0.5], [0.1, 0.1, 0.8], [0.3, 0.3, 0.4]])
    y = good.copy()
    y[1] = BAD_ROWS[row]
    m, v, X = np.zeros((3, 3)), np.ones((3, 3)), np.linspace(0, 1, 3)[:, None]
    e = Engine([("Dirichlet", {"K": 3})], 1, 8, 1)
    e.set_task_data(0, X, good)
    for call in (lambda: var_exp("Dirichlet", y, m, v, K=3), lambda: log_predictive_rows("Dirichlet", y, m, v, num_samples=8, K=3),
                 lambda: e.set_task_data(0, X[:2], y[:2])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "Dirichlet" in str(ei.value)
    assert e.N[0] == 3                                                  # refused before the task's state changed
    ok = good.copy()
    ok[1, 2] += 5e-7                                                    # within 1e-6 of one: accepted
    assert np.all(np.isfinite(var_exp("Dirichlet", ok, m, v, K=3)[0]))
    e.set_task_data(0, X, ok)
    e.close()


# ------------------------------------------------------------------------------------------------ whole model vs oracle
def DIR(K):
    return ("Dirichlet", {"K": K})


SET_GDB = [("Gaussian", {"sigma": 0.5}), DIR(3), ("Bernoulli", {})]
SET_DDG = [DIR(2), DIR(3), ("Gaussian", {"sigma": 0.7})]
SET_D4G = [DIR(4), ("Gaussian", {"sigma": 0.5})]


CASES = [(SET_GDB, 128, 2, 1), (SET_GDB, 128, 2, 2), (SET_DDG, 128, 2, 1), (SET_D4G, 128, 2, 1)]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n + str(k.get("K", "")) for n, k in c[0]), c[1], c[2], c[3])
                                                     for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    """In the minibatch the [K][N_t] array of log y_k is read with the TASK's stride, not the slice's."""
    Ns = [300, 257, 129][:len(specs)]
    mc.check_vs_oracle(mc.family_case(2100 + M + 7 * Q + P, specs, Ns, M, Q, P), Ns)


@pytest.mark.parametrize("specs", [SET_GDB, SET_DDG], ids=["Gaussian+Dirichlet3+Bernoulli", "Dirichlet2+Dirichlet3+Gaussian"])
def test_small_model_path_and_no_small_path(specs):
    """M = 16: all segments in one launch_quad_multi pass over one segment table (one dispatch per family present: a set outside the
    baseline masks takes the singleton instantiations) -- the second set is two Dirichlet segments with different K beside a Gaussian
    one; HMOGP_CFG_NO_SMALL_PATH runs the regular kernels on the same model."""
    Ns = [300, 257, 129]
    mc.check_small_vs_regular(mc.family_case(277, specs, Ns, 16, 2, 1), Ns, ([60, 50, 20], [160, 137, 129]))


def test_strict_qf_vs_literal_oracle():
    mc.check_strict_vs_literal(mc.family_case(231, SET_DDG, [300, 257, 129], 128, 2, 1))


# ------------------------------------------------------------------------------------------------ facade end to end
FACADE_RATIO_BOUND = 0.7765  # halfway between the measured ratio, 0.553, and 1


def _toy(seed, N=500):
    """A Gaussian output and a K = 3 composition that is a noisy softmax of correlated latent functions."""
    rng = np.random.RandomState(seed)
    l1 = lambda x: 1.5 * np.sin(2.0 * np.pi * x)
    l2 = lambda x: 1.2 * np.cos(3.0 * np.pi * x) - 0.3

    def comp(x):
        a = 12.0 * np.exp(np.hstack([l1(x), l2(x), np.zeros_like(x)]))
        a = a / a.sum(1, keepdims=True) * 12.0                          # softmax of the latent functions, concentration 12
        y = np.maximum(rng.gamma(a), 1e-9)
        return y / y.sum(1, keepdims=True)

    Xg, Xd = np.sort(rng.rand(N, 1), 0), np.sort(rng.rand(N, 1), 0)
    Yg = 0.8 * l1(Xg) + 0.3 + 0.2 * rng.randn(N, 1)
    Xt = np.sort(rng.rand(300, 1), 0)
    return Xg, Yg, Xd, comp(Xd), Xt, comp(Xt)


def test_facade_gaussian_and_composition_end_to_end():
    """The ELBO rises over two VEM iterations, and on 300 held-out inputs the mean absolute error of the predictive mean composition
    is below that of the constant training-mean composition: ratio measured once, 0.553 (0.1095 against 0.1979), asserted below the
    point halfway to 1, 0.7765 (an unfitted model sits near 1).  Both figures: DESIGN 9d."""
    import hetmogp_amd as H
    Xg, Yg, Xd, Yd, Xt, Yt = _toy(5)
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.2), H.Dirichlet(3)])
    md = likelihood.generate_metadata()
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.array([0.9, 0.9, 0.1, 0.1])[:, None], np.array([0.1, 0.1, 0.9, 0.1])[:, None]]
    Z = np.linspace(0, 1, M)[:, None]
    np.random.seed(0)
    model = H.HetMOGP(X=[Xg, Xd], Y=[Yg, Yd], Z=Z, kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list)
    assert model.Ymulti_all[1].shape == (500, 3) and model.Ymulti_all[0].shape == (500, 1)
    e0 = float(model.log_likelihood()[0, 0])
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        H.vem_algorithm(model, stochastic=False, vem_iters=2)
    caught = [w for w in caught if "K_uu is ill-conditioned" not in str(w.message)]
    assert not caught, [str(w.message) for w in caught]
    e1 = float(model.log_likelihood()[0, 0])
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    mean, var = model.predictive([Xt, Xt])
    assert mean[1].shape == (300, 3) and np.all(np.isfinite(mean[1])) and np.all(var[1] >= 0.0)
    assert np.all(mean[1] > 0.0) and np.max(np.abs(mean[1].sum(1) - 1.0)) < 1e-12
    mae_model = float(np.mean(np.abs(mean[1] - Yt)))
    mae_const = float(np.mean(np.abs(Yd.mean(0, keepdims=True) - Yt)))
    print("held-out MAE of the predictive mean composition %.4f, of the training-mean composition %.4f, ratio %.3f" %
          (mae_model, mae_const, mae_model / mae_const))
    assert mae_model < mae_const
    assert mae_model < FACADE_RATIO_BOUND * mae_const
    nlpd = model.negative_log_predictive([Xg[:50], Xd[:50]], [Yg[:50], Yd[:50]], num_samples=200, seed=3)
    assert np.isfinite(nlpd)
    # a shuffled, minibatched model carries the (N, K) observations through the permutation and the row slices
    model2 = H.HetMOGP(X=[Xg, Xd], Y=[Yg, Yd], Z=Z, kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list, batch_size=100)
    model2.shuffle_rows(seed=1)
    assert np.array_equal(model2.Ymulti_all[1], Yd[model2.row_permutation[1]]) and model2.Ymulti[1].shape == (100, 3)
    assert np.isfinite(float(model2.log_likelihood()[0, 0]))
