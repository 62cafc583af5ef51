"""GPU: the right-censored Weibull likelihood through every layer -- the row kernel against the high-precision grid
tests/golden/wbgrid.npz under the criterion of tests/likgrid.py and against the float64 restatement tests/weibull_ref.py, the
Exponential limit on the device, the predictive rule, the sampler, the Monte-Carlo log predictive (censored test rows included), the
refusal of rows that are no (time, indicator) pairs, the whole ELBO + gradient against the oracle (the checks of tests/model_cases.py)
on the default, several-pool, minibatch, small-model and strict q(f) paths, the model facade end to end, and the split step.

The oracle covers the family through a module-scoped fixture that registers tests/weibull_ref.py with oracle.likelihoods_oracle for
the duration of this module (`oracle/` is not edited; its row slicing carries a two-column Y as it is): cases are drawn by
model_cases.synth with Gamma standing in for the new task (same dim_f), whose observations are then replaced by seeded (N, 2) rows
with about 30 % censored.

Kernel figures on wbgrid.npz, worst |kernel - R| / (2^-52 S) per class and kind (ve / dm / dv), measured on an MI355X: see DESIGN 9i."""
import warnings

import numpy as np
import pytest
from scipy import stats

import likgrid
import model_cases as mc
import negbin_ref as nr
import weibull_ref as wr
from conftest import assert_parity
from test_weibull_cpu import BULK, KIND, assert_grid, bulk_rows, c_kernel, c_kernel_vs_float64, load_grid

pytestmark = pytest.mark.gpu

WB = ("Weibull", {})
NB = ("NegBinomial", {})
LIK_ID = 12


@pytest.fixture(scope="module", autouse=True)
def weibull_in_the_oracle():
    """tests/weibull_ref.py as the oracle's contract module of the family, its id, and dim_f = 2 (and tests/negbin_ref.py for the
    Negative Binomial task of the mixed model, as tests/test_negbin_gpu.py registers it) -- undone at teardown."""
    from oracle import likelihoods_oracle as lo
    patch = pytest.MonkeyPatch()
    patch.setitem(lo._CONTRACT, "Weibull", wr)
    patch.setitem(lo.LIK_IDS, "Weibull", LIK_ID)
    patch.setitem(lo._CONTRACT, "NegBinomial", nr)
    patch.setitem(lo.LIK_IDS, "NegBinomial", 11)
    dim_f = lo.dim_f
    patch.setattr(lo, "dim_f", lambda name, K=None: 2 if name in ("Weibull", "NegBinomial") else dim_f(name, K))
    yield
    patch.undo()


@pytest.fixture(scope="module")
def grid():
    return load_grid()


def _gpu_var_exp(Y, m, v):
    from hetmogp_amd.engine import var_exp
    return likgrid.pack(*var_exp("Weibull", Y, m, v), len(Y))


# ------------------------------------------------------------------------------------------------ the row kernel
def test_var_exp_on_the_high_precision_grid(grid):
    """Every element of every row within C_KERNEL = max(16, 4 C_ORACLE) of its class and kind; every element finite; no exceptions."""
    got = _gpu_var_exp(grid["y"], grid["m"], grid["v"])
    assert np.all(np.isfinite(got))
    assert_grid(grid, got, c_kernel(), "kernel on wbgrid")


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_var_exp_wave_and_block_tails(grid, N):
    """N rows of the grid in one call (one wave per row, four rows per block): the tails of the wave / block grid, with both
    indicators inside a block of four rows (the bulk rows of the grid alternate, and the stride is odd)."""
    rows = (np.arange(N) * 7 + N) % len(grid["y"])
    d = grid["y"][rows, 1]
    assert N < 4 or any(0 < d[b:b + 4].sum() < 4 for b in range(0, N - 3, 4))
    got = _gpu_var_exp(grid["y"][rows], grid["m"][rows], grid["v"][rows])
    assert_grid(grid, got, c_kernel(), "kernel on %d rows of wbgrid" % N, rows)


def test_var_exp_matches_restatement_on_seeded_bulk_rows():
    """3000 bulk rows: kernel and float64 restatement each sit within their own bulk constant of the true value in units of 2^-52 S
    (S from the restatement), so they differ by at most the sum of the two."""
    from hetmogp_amd import Weibull
    Y, m, v = bulk_rows(np.random.RandomState(5), 3000)
    got, want = _gpu_var_exp(Y, m, v), likgrid.pack(*wr.var_exp(Y, m, v), len(Y))
    likgrid.assert_rows(got, want, wr.var_exp_scale(Y, m, v), np.zeros(got.shape, np.uint8), KIND, np.zeros(len(Y), np.uint8),
                        c_kernel_vs_float64(), "kernel against weibull_ref, 3000 bulk rows")
    d = Weibull()
    assert np.array_equal(d.var_exp(Y[:100], m[:100], v[:100])[:, 0], got[:100, 0])            # the descriptor runs the same kernel
    dm, dv = d.var_exp_derivatives(Y[:100], m[:100], v[:100])
    assert np.array_equal(np.hstack([dm, dv]), got[:100, 1:])


def test_exponential_limit_on_the_device():
    """var_exp("Weibull", [y, 1], (m0, 0), (v0, 0)) against var_exp("Exponential", y, -m0, v0): k = 1 exactly, so ve (and dv_0) agree
    and dm_0 has the opposite sign, each within the sum of the two families' bulk kernel constants in units of 2^-52 S."""
    from hetmogp_amd.engine import var_exp
    rng = np.random.RandomState(5)
    N = 300
    m0, v0 = rng.uniform(-1.5, 1.5, N), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), N))
    y = np.exp(m0) * rng.exponential(1.0, N)
    Y, m, v = np.stack([y, np.ones(N)], 1), np.stack([m0, np.zeros(N)], 1), np.stack([v0, np.zeros(N)], 1)
    ve, dm, dv = var_exp("Weibull", Y, m, v)
    eve, edm, edv = var_exp("Exponential", y, -m0, v0)
    S = wr.var_exp_scale(Y, m, v)
    cw, ce = c_kernel()[BULK], likgrid.c_kernel("Exponential")[BULK]
    for name, a, b, s, c in (("ve", ve, np.ravel(eve), S[:, 0], cw[0] + ce[0]), ("dm_0", dm[:, 0], -np.ravel(edm), S[:, 1], cw[1] + ce[1]),
                             ("dv_0", dv[:, 0], np.ravel(edv), S[:, 3], cw[2] + ce[2])):
        r = np.abs(a - b) / (likgrid.EPS * s)
        print("Exponential limit, %-4s: worst |Weibull - Exponential| / (2^-52 S) = %.3g (bound %g)" % (name, r.max(), c))
        assert np.all(r <= c), name
    assert np.all(dm[:, 0] * np.ravel(edm) < 0.0)                                               # opposite signs, none zero


# ------------------------------------------------------------------------------------------------ predictive, sample, log predictive
def test_predictive_rule():
    from hetmogp_amd.engine import predictive
    from hetmogp_amd import Weibull
    rng = np.random.RandomState(5)
    N = 300
    # (m1 in [-0.5, 1], v1 <= 0.1: 1 / k <= 18 at every node, so lgamma stays below 100 and its 1-2 ulp are 4e-14 of the result; and the
    #  shape at the mean stays below e, so the variance, a difference of two second moments, is more than a tenth of either)
    m = np.stack([rng.uniform(-3.0, 4.0, N), rng.uniform(-0.5, 1.0, N)], 1)
    v = np.stack([10.0 ** rng.uniform(-6.0, 0.5, N), 10.0 ** rng.uniform(-6.0, -1.0, N)], 1)
    v[:5, 0] = 0.0
    v[5:10, 1] = 0.0
    mean, var = predictive("Weibull", m, v)
    wm, wv = wr.predictive(m, v)
    assert mean.shape == (N, 1) and var.shape == (N, 1) and np.all(mean > 0.0) and np.all(var > 0.0)
    assert np.allclose(mean, wm, rtol=1e-12, atol=0) and np.allclose(var, wv, rtol=1e-12, atol=0)
    m2, v2 = Weibull().predictive(m, v)
    assert np.array_equal(m2, mean) and np.array_equal(v2, var)
    mean, var = predictive("Weibull", np.array([[800.0, 0.0], [0.0, -6.0]]), np.array([[1.0, 0.0], [0.1, 0.1]]))   # overflow is +inf
    assert np.all(np.isposinf(mean)) and np.all(np.isposinf(var))


def test_sample_moments():
    """2e5 draws at three (f0, f1): sample mean and variance within 5 standard errors of lambda Gamma(1 + 1/k) and
    lambda^2 (Gamma(1 + 2/k) - Gamma(1 + 1/k)^2); se(mean) = sqrt(var / N), se(variance) = var sqrt((excess kurtosis + 2) / N).  The
    third point has k < 1 (a decreasing hazard, the heavy tail).  Draws are event times: one column, positive, never censored."""
    from hetmogp_amd.engine import sample
    from hetmogp_amd import Weibull
    N = 200000
    for seed, (f0, f1) in enumerate(((0.5, 0.7), (-1.0, 1.5), (1.0, -0.3))):
        y = sample("Weibull", np.tile([[f0, f1]], (N, 1)), seed=700 + seed)
        assert y.shape == (N, 1) and np.all(np.isfinite(y)) and np.all(y > 0.0)
        y = y[:, 0]
        mu, vr = wr.moments(f0, f1)
        kurt = float(stats.weibull_min(np.exp(f1)).stats("k"))
        zm, zv = abs(y.mean() - mu) / np.sqrt(vr / N), abs(y.var() - vr) / (vr * np.sqrt((kurt + 2.0) / N))
        print("sample f = (%.1f, %.1f): |mean - mu| / se = %.2f, |variance - .| / se = %.2f" % (f0, f1, zm, zv))
        assert zm <= 5.0 and zv <= 5.0, (f0, f1, zm, zv)
    ys = Weibull().samples(np.zeros((50, 2)), seed=5)
    assert ys.shape == (50, 1) and np.all(ys > 0.0)


def test_log_predictive_at_vanishing_variance():
    """v = 0: every Monte-Carlo sample is f = m, so the per-row log predictive is log p(y, delta | m) exactly -- the density of an
    observed row, the survival probability of a censored one."""
    from hetmogp_amd.engine import log_predictive_rows
    from hetmogp_amd import Weibull
    rng = np.random.RandomState(11)
    N = 500
    Y, m, _ = bulk_rows(rng, N)
    assert 0 < Y[:, 1].sum() < N
    v = np.zeros_like(m)
    got = log_predictive_rows("Weibull", Y, m, v, num_samples=128, seed=4)
    want = wr.logpdf_and_derivatives(Y[:, 0], Y[:, 1], m[:, 0], m[:, 1])[0]
    assert got.shape == (N,) and np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))) < 1e-10
    assert np.all(got[Y[:, 1] == 0.0] <= 0.0)                                   # a survival probability
    lp = Weibull().log_predictive(Y, m, v, 64, seed=1)
    assert abs(lp - want.sum() / 64.0) < 1e-10 * abs(want.sum() / 64.0)


# ------------------------------------------------------------------------------------------------ refusals
BAD = [(0, 0.0), (0, -1.0), (0, float("nan")), (0, float("inf")), (1, 0.5), (1, 2.0), (1, -1.0), (1, float("nan"))]


@pytest.mark.parametrize("col,bad", BAD, ids=["y=%r" % b if c == 0 else "delta=%r" % b for c, b in BAD])
def test_rows_that_are_no_time_and_indicator_are_refused(col, bad):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    good = np.array([[0.5, 1.0], [3.0, 0.0], [7.0, 1.0]])
    Y = good.copy()
    Y[1, col] = bad
    m, v, X = np.zeros((3, 2)), np.ones((3, 2)), np.linspace(0, 1, 3)[:, None]
    e = Engine([WB], 1, 8, 1)
    e.set_data([X], [good])
    for call in (lambda: var_exp("Weibull", Y, m, v), lambda: log_predictive_rows("Weibull", Y, m, v, num_samples=8),
                 lambda: e.set_data([X[:2]], [Y[:2]])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "Weibull" in str(ei.value)
    assert e.N[0] == 3                                                           # refused before the task's state changed
    assert np.all(np.isfinite(var_exp("Weibull", good, m, v)[0]))                # a valid call right after succeeds
    e.set_data([X], [good])
    e.close()


def test_a_one_column_y_is_refused():
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    good = np.array([[0.5, 1.0], [3.0, 0.0], [7.0, 1.0], [2.0, 1.0]])
    m, v, X = np.zeros((4, 2)), np.ones((4, 2)), np.linspace(0, 1, 4)[:, None]
    e = Engine([WB], 1, 8, 1)
    e.set_data([X], [good])
    for one in (good[:, :1], good[:, 0]):
        for call in (lambda: var_exp("Weibull", one, m, v), lambda: log_predictive_rows("Weibull", one, m, v, num_samples=8),
                     lambda: e.set_data([X], [one])):
            with pytest.raises(_lib.InvalidArgument) as ei:
                call()
            assert "Weibull" in str(ei.value)
    assert e.N[0] == 4
    assert np.all(np.isfinite(var_exp("Weibull", good, m, v)[0]))
    e.close()


def test_the_family_has_no_parameters_of_its_own():
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp_dparam
    with pytest.raises(_lib.InvalidArgument) as ei:
        var_exp_dparam("Weibull", np.array([[1.0, 1.0], [2.0, 0.0]]), np.zeros((2, 2)), np.ones((2, 2)))
    assert "no parameters of its own" in str(ei.value)
    e = Engine([WB], 1, 8, 1)
    assert e.lik_param_count(0) == 0
    e.close()


# ------------------------------------------------------------------------------------------------ whole model vs oracle
SET_W = [WB]
SET_GWB = [("Gaussian", {"sigma": 0.5}), WB, ("Bernoulli", {})]
SET_WCH = [WB, ("Categorical", {"K": 3}), ("HetGaussian", {})]
SET_MIX = [WB, NB, ("Student", {"deg_free": 4.0}), ("Ordinal", {"K": 4}), ("Dirichlet", {"K": 3})]


def _case(seed, specs, Ns, M, Q, P, censored=0.3, scale=1.5e-3, w1=1.0):
    """model_cases.family_case with Gamma standing in for every Weibull (and Negative Binomial) task; then, from RandomState(seed + 2)
    in task order, their observations are replaced -- Weibull by (N, 2) rows of the given scale and shape 1.3 with the stated share
    censored, Negative Binomial by counts with mean 3 and size 2 -- and the problem is made for the real specs.

    The scale.  synth's q(f) is that of an untrained model: the variance of f1 reaches 0.6 at M = 16 and 3 at (M, Q, P) = (128, 3, 2),
    far outside the family's envelope (v1 <= 0.1), so the shape reaches its clip of 1e3 at the outer nodes, and with times
    of the prior's own scale (y / lambda of order one) z = k (ly - f0) takes its clip of 680 at some node of most rows: the ELBO is
    then 1e280 .. 1e295, a sum of a few clipped addends.  Times short against the prior's scale (ly - f0 < 0 at nearly every node)
    keep z negative there and nine of the twelve cases of test_elbo_grad_vs_oracle at an ELBO of -3e2 .. -7e62; the three cases
    of shape (128, 3, 2), whose v0 reaches 6, clip regardless and cover the clip through the whole model.

    w1 scales the mixing weights W[:, d] of every Weibull task's f1 (its q(f1) variance by w1^2), for the one check that compares two
    device paths to 1e-12 (test_small_model_path_carries_weibull)."""
    from oracle import svmogp_oracle as so
    prm, _, X, Y = mc.family_case(seed, [("Gamma", {}) if s in (WB, NB) else s for s in specs], Ns, M, Q, P)
    rng = np.random.RandomState(seed + 2)
    d = 0
    for t, s in enumerate(specs):
        if s == WB:
            prm["W"][:, d + 1] *= w1
        d += 2 if s in (WB, NB) else mc_dim_f(s)
    for t, s in enumerate(specs):
        if s == WB:
            Y[t] = wr.draw(rng, np.full(Ns[t], np.log(scale)), np.full(Ns[t], np.log(1.3)), censored)
        elif s == NB:
            Y[t] = rng.poisson(3.0 * rng.gamma(2.0, 0.5, (Ns[t], 1))).astype(float)
    return prm, so.make_problem(specs, Q, M, P), X, Y


def mc_dim_f(spec):
    from oracle import likelihoods_oracle as lo
    return lo.dim_f(spec[0], spec[1].get("K"))


SHAPES = [(16, 1, 1), (100, 3, 1), (128, 3, 2), (256, 1, 2)]
CASES = [(s, M, Q, P) for s in (SET_W, SET_GWB, SET_WCH) for M, Q, P in SHAPES]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n for n, _ in c[0]), c[1], c[2], c[3]) for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    """One row pool, several, and a minibatch with row_begin > 0 (both columns of the task's image are read with the TASK's stride)."""
    Ns = [300, 257, 129][:len(specs)]
    case = _case(4100 + M + 7 * Q + P, specs, Ns, M, Q, P)
    t = specs.index(WB)
    assert case[3][t].shape == (Ns[t], 2) and 0.15 < 1.0 - case[3][t][:, 1].mean() < 0.45
    mc.check_vs_oracle(case, Ns)


def test_small_model_path_carries_weibull():
    """M = 48: the family's singleton instantiation of quad_multi_kernel and the captured graph, against the regular kernels.

    The check holds the two paths to 1e-12 of each other.  They differ in the rounding of q(f)'s mean and variance (1e-15), which this
    family amplifies by k |f0| through e = exp(k (ly - f0)): with synth's weights the variance of f1 reaches 0.43 here, k reaches 573
    at the outer nodes and z 428 -- the ELBO is -1.5e160 and the amplification 1e4 (all oracle-side figures).  The weights of f1 are
    halved, which puts v1 at the edge of the family's envelope (0.11; k <= 24, z <= 41, ELBO -1.6e3), where 1e-12 measures
    the two paths; the envelope is asserted on the oracle's q(f) below."""
    from oracle import likelihoods_oracle as lo
    Ns = [300, 257, 129]
    case = _case(477, SET_GWB, Ns, 48, 2, 1, w1=0.5)
    seen = {}

    class Spy(object):
        @staticmethod
        def var_exp(Y, m, v, **kw):
            seen["v1"], seen["clipped"] = float(np.max(v[:, 1])), int(wr.clipped_nodes(Y, m, v).sum())
            return wr.var_exp(Y, m, v, **kw)
    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(lo._CONTRACT, "Weibull", Spy)
        from oracle import svmogp_oracle as so
        so.elbo_grad_fused(*case)
    assert seen["v1"] <= 0.11 and seen["clipped"] == 0, seen
    mc.check_small_vs_regular(case, Ns, ([60, 50, 20], [160, 137, 129]))


def test_strict_qf_with_weibull_vs_literal_oracle():
    mc.check_strict_vs_literal(_case(431, SET_WCH, [400, 300, 257], 128, 2, 1))


def test_mixed_with_the_other_table_families():
    """Weibull, Negative Binomial, Student, Ordinal and Dirichlet(3) in one model: a set outside the baseline masks, so
    launch_quad_multi takes its generic path with the five singleton instantiations behind each other."""
    from oracle import svmogp_oracle as so
    Ns = [300, 257, 129, 200, 150]
    prm, prob, X, Y = _case(4500, SET_MIX, Ns, 16, 2, 1)
    want = so.elbo_grad_fused(prm, prob, X, Y)
    e = mc.make_engine(prob, X, Y)
    mc._parity(mc.run(e, prm), want, "mixed M = 16 ")
    e.close()


@pytest.mark.parametrize("censored", [0.0, 1.0], ids=["all-observed", "all-censored"])
def test_all_observed_and_all_censored_tasks(censored):
    from oracle import svmogp_oracle as so
    Ns = [257]
    prm, prob, X, Y = _case(4600, SET_W, Ns, 16, 1, 1, censored=0.0, scale=1.5)   # (v1 <= 0.2 at this shape: times of the prior's scale)
    if censored == 1.0:
        Y[0][:, 1] = 0.0                                                        # every row: "still running at time y"
    assert np.all(Y[0][:, 1] == 1.0 - censored)
    want = so.elbo_grad_fused(prm, prob, X, Y)
    e = mc.make_engine(prob, X, Y)
    mc._parity(mc.run(e, prm), want, "censored share %g " % censored)
    e.close()


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed):
    rng = np.random.RandomState(seed)
    Xs, Xb = np.sort(rng.rand(400, 1), 0), np.sort(rng.rand(300, 1), 0)
    Ys = wr.draw(rng, 0.5 + 0.8 * np.sin(2.0 * np.pi * Xs), 0.4 + 0.3 * np.cos(2.0 * np.pi * Xs), censored=0.3)
    Yb = (rng.rand(300, 1) < 1.0 / (1.0 + np.exp(-3.0 * np.cos(4.0 * Xb)))).astype(float)
    return [Xs, Xb], [Ys, Yb]


def _model_prm(model):
    return dict(Z=model.Z.values, m_u=model.q_u_means.values, L_flat=model.q_u_chols.values,
                variance=np.array([float(k.variance[0]) for k in model.kern_list]),
                lengthscale=np.array([float(k.lengthscale[0]) for k in model.kern_list]),
                W=np.stack([np.ravel(B.W.values) for B in model.B_list]), kappa=np.stack([np.ravel(B.kappa.values) for B in model.B_list]))


def test_facade_weibull_and_bernoulli_end_to_end():
    import hetmogp_amd as H
    from oracle import svmogp_oracle as so
    X, Y = _toy(21)
    assert 0.15 < 1.0 - Y[0][:, 1].mean() < 0.45
    likelihood = H.HetLikelihood([H.Weibull(), H.Bernoulli()])
    md = likelihood.generate_metadata()
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    # (f1, the log shape, mixes the latents with small weights: from the start q(u) = N(0, I) its variance is then 0.05, inside the
    #  family's envelope -- with weights of 0.1 and 0.9 it is 0.8, the shape reaches its clip at the outer nodes and the first L-BFGS
    #  step, taken along a gradient of 1e280, leaves the parameters' domain)
    W_list = [np.array([0.9, 0.15, 0.5])[:, None], np.array([0.1, 0.15, 0.9])[:, None]]
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
    assert np.all(mean[0] > 0.0) and np.all(var[0] > 0.0)
    Yt = [y[:50] for y in Y]
    assert 0 < Yt[0][:, 1].sum() < 50                                            # censored test rows included
    nlpd = model.negative_log_predictive([x[:50] for x in X], Yt, num_samples=200, seed=3)
    assert np.isfinite(nlpd)


# ------------------------------------------------------------------------------------------------ the split step
def test_split_step_equals_the_plain_call_bit_for_bit():
    """hmogp_step_begin / hmogp_step_finish on one rank: the bundle carries nothing family-specific."""
    specs = [("Gaussian", {"sigma": 0.5}), WB]
    Ns = [300, 257]
    prm, prob, X, Y = _case(51, specs, Ns, 64, 2, 1)
    e = mc.make_engine(prob, X, Y, small_path=False)             # (a split step always takes the regular kernels)
    full = mc.run(e, prm)
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"], W=prm["W"],
                kappa=prm["kappa"])
    e.step_begin(**args)
    out = e.step_finish()
    for k in mc.KEYS:
        assert np.array_equal(np.asarray(out[k]), np.asarray(full[k])), k
    e.close()
