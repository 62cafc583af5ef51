"""GPU: the Binomial and Beta-Binomial likelihoods through every layer -- the row kernels against the high-precision grid
tests/golden/bngrid.npz under the criterion |got - R| <= C 2^-52 S and against the float64 restatement tests/binom_ref.py, the launch
shapes, the ties to the Bernoulli kernel (n = 1, and the collapse of n Bernoulli rows into one), the predictive rule, the sampler, the
log predictive routines, the refusals, the whole ELBO + gradient against the oracle (the checks of tests/model_cases.py) on the default,
several-pool, minibatch, small-model and strict q(f) paths, the collapse identity at model level, the model facade and the split step.

The oracle covers the families through a module-scoped fixture that registers tests/binom_ref.py's contract objects with
oracle.likelihoods_oracle for the duration of this module (`oracle/` is not edited; its row slicing carries a two-column Y as it is):
cases are drawn by model_cases.synth with Bernoulli standing in for a Binomial task and Gamma for a Beta-Binomial one (same dim_f),
whose observations are then replaced by seeded (N, 2) rows.

Kernel figures on bngrid.npz, worst |kernel - R| / (2^-52 S) per family, class and output, measured on an MI355X: see DESIGN 9l."""
import warnings

import numpy as np
import pytest
from scipy import stats

import binom_ref as br
import likgrid
import model_cases as mc
import negbin_ref as nr
import weibull_ref as wr
from conftest import assert_parity

pytestmark = pytest.mark.gpu

BN = ("Binomial", {})
BB = ("BetaBinomial", {})
WB = ("Weibull", {})
NB = ("NegBinomial", {})
FAMILIES = ("Binomial", "BetaBinomial")
IDS = {"Binomial": 13, "BetaBinomial": 14}


@pytest.fixture(scope="module", autouse=True)
def binomials_in_the_oracle():
    """tests/binom_ref.py's contract objects as the oracle's contract of the two families, their ids and dim_f (and weibull_ref /
    negbin_ref for the mixed model, as their own test modules register them) -- undone at teardown."""
    with br.in_the_oracle((("Weibull", wr, 12, 2), ("NegBinomial", nr, 11, 2))):
        yield


def _gpu(family, Y, m, v):
    from hetmogp_amd.engine import var_exp
    return br.stack(*var_exp(family, Y, m, v))


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("family", FAMILIES)
def test_var_exp_on_the_high_precision_grid(family):
    """Every element of every row within C_KERNEL = max(16, 4 C_ORACLE) of its family, class and output; every element finite; no
    exceptions.  (The raw figures are printed: DESIGN 9l records them.)"""
    g = br.load_grid(family)
    br.assert_grid(family, _gpu(family, g["y"], g["m"], g["v"]), g, br.c_kernel, "kernel on bngrid")


@pytest.mark.parametrize("family", FAMILIES)
def test_var_exp_matches_restatement_on_seeded_bulk_rows(family):
    """3000 fresh bulk rows: kernel and float64 restatement each sit within their own bulk constant of the true value in units of
    2^-52 S (S from the restatement), so they differ by at most the sum of the two.  The descriptor runs the same kernel."""
    import hetmogp_amd as H
    Y, m, v = br.bulk_rows(family, 3000, seed=5)
    got, want, S = _gpu(family, Y, m, v), br.stack(*br.var_exp(family, Y, m, v)), br.var_exp_scale(family, Y, m, v)
    r = br.ratios(got, want, S)
    print("[bulk 3000] %-12s %s" % (family, " ".join("%s %.3g" % (o, x) for o, x in zip(br.OUTPUTS[family], r.max(0)))))
    for o, name in enumerate(br.OUTPUTS[family]):
        assert r[:, o].max() <= br.c_sum(family, br.BULK, o), (family, name, r[:, o].max())
    d = getattr(H, family)()
    assert np.array_equal(d.var_exp(Y[:100], m[:100], v[:100])[:, 0], got[:100, 0])
    dm, dv = d.var_exp_derivatives(Y[:100], m[:100], v[:100])
    assert np.array_equal(np.hstack([dm, dv]), got[:100, 1:])


# ------------------------------------------------------------------------------------------------ launch shapes
def _shape_rows(family, N):
    """N rows with n <= 32 and n > 32, k = 0 and k = n inside the first block (one lane per row: 256 rows; one wave per row: 4 rows)."""
    J = br.DIM_F[family]
    rng = np.random.RandomState(100 + N)
    n = np.where(np.arange(N) % 2 == 0, rng.randint(1, 33, N), rng.randint(33, 400, N)).astype(float)
    k = np.floor(rng.rand(N) * (n + 1.0)).clip(0, n)
    k[0::4], k[1::4] = 0.0, n[1::4]
    return np.stack([k, n], 1), rng.uniform(-1.5, 1.5, (N, J)), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, J)))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("family", FAMILIES)
def test_launch_shapes_equal_single_row_calls(family, N):
    """N rows in one call: the tails of the wave / block grid.  Equal row by row to calls of one row each (bit for bit: a row's result
    does not depend on its neighbours or on its place in the block)."""
    Y, m, v = _shape_rows(family, N)
    if N >= 4:
        assert np.any(Y[:4, 1] <= 32) and np.any(Y[:4, 1] > 32) and Y[0, 0] == 0.0 and Y[1, 0] == Y[1, 1]
    got = _gpu(family, Y, m, v)
    assert np.all(np.isfinite(got))
    single = np.vstack([_gpu(family, Y[i:i + 1], m[i:i + 1], v[i:i + 1]) for i in range(N)])        # every row as a call of its own
    assert np.array_equal(single, got), (family, N, np.argwhere(single != got)[:4])


# ------------------------------------------------------------------------------------------------ ties to the Bernoulli kernel
def test_binomial_at_one_trial_is_the_bernoulli_kernel():
    """(y, 1) rows against the Bernoulli kernel on the same (y, m, v): within 4 2^-52 S; bitwise equality is expected (lc = 0, and
    every product with k and n - k is exact) and reported."""
    from hetmogp_amd.engine import var_exp
    rng = np.random.RandomState(9)
    N = 2000
    y = (rng.rand(N) < 0.5).astype(float)
    m, v = rng.uniform(-6.0, 6.0, N), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), N))
    m[:4], v[:4] = (25.0, -25.0, 750.0, -750.0), 0.0
    Y = np.stack([y, np.ones(N)], 1)
    a, b = br.stack(*var_exp("Binomial", Y, m, v)), br.stack(*var_exp("Bernoulli", y, m, v))
    r = br.ratios(a, b, br.binom_scale(Y, m, v))
    print("Binomial(n = 1) vs Bernoulli: worst %.3g of 2^-52 S; bitwise equal: %s" % (r.max(), np.array_equal(a, b)))
    assert r.max() <= 4.0


def test_collapse_identity_on_the_device():
    """ve - lc, dm, dv of (k, n) equal k x Bernoulli's at y = 1 plus (n - k) x Bernoulli's at y = 0 at the same (m, v), within the sum
    of the kernels' constants times their scales (Bernoulli's scale is the Binomial scale of the rows (1, 1) and (0, 1))."""
    from hetmogp_amd.engine import var_exp
    Y, m, v = br.bulk_rows("Binomial", 1000, seed=21)
    k, n = Y[:, 0], Y[:, 1]
    got = br.stack(*var_exp("Binomial", Y, m, v))
    got[:, 0] -= br.log_choose(k, n)
    one, zero = br.stack(*var_exp("Bernoulli", np.ones(len(k)), m, v)), br.stack(*var_exp("Bernoulli", np.zeros(len(k)), m, v))
    want = k[:, None] * one + (n - k)[:, None] * zero
    Y1, Y0 = np.stack([np.ones_like(k), np.ones_like(k)], 1), np.stack([np.zeros_like(k), np.ones_like(k)], 1)
    Sb, Se = br.binom_scale(Y, m, v), k[:, None] * br.binom_scale(Y1, m, v) + (n - k)[:, None] * br.binom_scale(Y0, m, v)
    cb = likgrid.c_kernel("Bernoulli")[likgrid.BULK]
    for o, name in enumerate(br.OUTPUTS["Binomial"]):
        # (one more rounding of size 2^-52 S on the Binomial side: the subtraction of lc from ve, and the products k x, (n - k) x on the other)
        bound = br.EPS * ((br.c_kernel("Binomial", br.BULK, o) + 1.0) * Sb[:, o] + (cb[o] + 2.0) * Se[:, o])
        d = np.abs(got[:, o] - want[:, o])
        print("collapse identity on the device, %-2s: worst |difference| / bound = %.3g" % (name, np.max(d / bound)))
        assert np.all(d <= bound), name


# ------------------------------------------------------------------------------------------------ predictive and samples
@pytest.mark.parametrize("family", FAMILIES)
def test_predictive_rule(family):
    from hetmogp_amd.engine import predictive
    import hetmogp_amd as H
    rng = np.random.RandomState(6)
    N, J = 300, br.DIM_F[family]
    m, v = rng.uniform(-2.0, 2.0, (N, J)), 10.0 ** rng.uniform(-6.0, 0.3, (N, J))
    v[:5] = 0.0
    for trials in (1, 12, 1000):
        for T in (0, 10, 20):
            mean, var = predictive(family, m, v, gh_T=T, pred_trials=trials)
            wm, wv = br.predictive(family, m, v, trials=trials, T=T or 20)
            assert mean.shape == (N, 1) and var.shape == (N, 1)
            assert np.allclose(mean, wm, rtol=1e-12, atol=0) and np.allclose(var, wv, rtol=1e-12, atol=0), (family, trials, T)
            assert np.all((mean >= 0.0) & (mean <= trials)) and np.all(var > 0.0)
    m2, v2 = getattr(H, family)(pred_trials=12).predictive(m, v)
    wm, wv = br.predictive(family, m, v, trials=12)
    assert np.allclose(m2, wm, rtol=1e-12, atol=0) and np.allclose(v2, wv, rtol=1e-12, atol=0)
    if family == "Binomial":                    # one trial: Bernoulli's predictive
        bm, bv = predictive("Bernoulli", m[:, 0], v[:, 0])
        mean, var = predictive("Binomial", m, v, pred_trials=1)
        assert np.allclose(mean, bm, rtol=1e-14, atol=0) and np.allclose(var, bv, rtol=1e-14, atol=1e-17)
        assert np.array_equal(predictive("Binomial", m, v, pred_trials=0)[0], mean)          # 0 means 1


SAMPLE_POINTS = [("Binomial", 1, (np.log(0.3 / 0.7),)), ("Binomial", 12, (np.log(0.3 / 0.7),)), ("Binomial", 1000, (np.log(0.4 / 0.6),)),
                 ("Binomial", 1000, (np.log(0.97 / 0.03),)), ("BetaBinomial", 12, (np.log(1.5), np.log(3.5))),
                 ("BetaBinomial", 500, (np.log(20.0), np.log(5.0)))]


@pytest.mark.parametrize("family,trials,f", SAMPLE_POINTS, ids=["%s-%d-%d" % (s[0], s[1], i) for i, s in enumerate(SAMPLE_POINTS)])
def test_sample_moments(family, trials, f):
    """2e5 seeded draws: mean and variance within 5 standard errors of the closed forms, se(variance) from the exact fourth central
    moment, sqrt((mu4 - var^2) / N); every draw an integer in [0, n*].  The points cover the inversion (n* p < 10), BTRS, and the
    reflection p > 1/2."""
    from hetmogp_amd.engine import sample
    N = 200000
    y = sample(family, np.tile([list(f)], (N, 1)), seed=900 + trials, pred_trials=trials)
    assert y.shape == (N, 1) and np.all(y == np.floor(y)) and np.all((y >= 0) & (y <= trials))
    y = y[:, 0]
    mu, vr, mu4 = br.moments(family, trials, f)
    zm, zv = abs(y.mean() - mu) / np.sqrt(vr / N), abs(y.var() - vr) / np.sqrt((mu4 - vr * vr) / N)
    print("sample %s n* = %d: |mean - mu| / se = %.2f, |variance - .| / se = %.2f" % (family, trials, zm, zv))
    assert zm <= 5.0 and zv <= 5.0, (family, trials, zm, zv)


def test_descriptor_samples():
    import hetmogp_amd as H
    ys = H.Binomial(pred_trials=7).samples(np.zeros((50, 1)), seed=5)
    assert ys.shape == (50, 1) and np.all((ys >= 0) & (ys <= 7) & (ys == np.floor(ys)))
    ys = H.BetaBinomial(pred_trials=7).samples(np.zeros((50, 2)), seed=5)
    assert ys.shape == (50, 1) and np.all((ys >= 0) & (ys <= 7) & (ys == np.floor(ys)))


# ------------------------------------------------------------------------------------------------ log predictive
@pytest.mark.parametrize("family", FAMILIES)
def test_log_predictive_routines(family):
    """hmogp_log_predictive_gh at v = 0 is log p; over bulk rows it meets the criterion of DESIGN 9j, |lpd - restatement| <= C 2^-52 S
    with S = 1 + sum wbar |addends| and C = c_sum of the bulk class's ve, for gh_T in {0, 10, 20}; the Monte-Carlo routine agrees with
    the dense value within 6 of its own standard errors (plus the rule's own error)."""
    from hetmogp_amd.engine import log_predictive_density_rows, log_predictive_rows
    Y, m, v = br.bulk_rows(family, 400, seed=31)
    J = br.DIM_F[family]
    got = log_predictive_density_rows(family, Y, m, np.zeros_like(v))
    want = br.logpdf(family, Y, m.reshape(-1, J))
    assert np.max(np.abs(got - want) / (1.0 + np.abs(want))) <= 1e-12
    for T in (0, 10, 20):
        lpd, ess = log_predictive_density_rows(family, Y, m, v, gh_T=T, return_ess=True)
        wl, we, S = br.lpd(family, Y, m, v, T=T or 20)
        r = np.abs(lpd - wl) / (br.EPS * S)
        print("lpd %-12s T = %2d: worst %.3g of 2^-52 S" % (family, T or 20, r.max()))
        assert r.max() <= br.c_sum(family, br.BULK, 0)
        assert np.allclose(ess, we, rtol=1e-9)
    S_mc = 4096
    mcv = log_predictive_rows(family, Y, m, v, num_samples=S_mc, seed=3)
    rng = np.random.RandomState(1)
    F = m[:, None, :] + np.sqrt(v)[:, None, :] * rng.randn(len(Y), 2000, J)
    lp = br.logpdf(family, Y, F)
    mx = lp.max(1, keepdims=True)
    w = np.exp(lp - mx)
    dense, se = mx[:, 0] + np.log(w.mean(1)), w.std(1) / w.mean(1)
    z = np.abs(mcv - dense) / (se * np.sqrt(1.0 / S_mc + 1.0 / 2000.0) + 1e-12)
    print("Monte-Carlo log predictive %-12s: worst |device - NumPy| / se = %.2f" % (family, z.max()))
    assert z.max() <= 6.0


def test_predict_log_density_is_the_building_block_on_predict_f():
    from hetmogp_amd.engine import log_predictive_density_rows
    Ns = [120, 90]
    case = _case(77, [BN, BB], Ns, 16, 2, 1)
    prm, prob, X, Y = case
    e = mc.make_engine(prob, X, Y)
    mc.run(e, prm)
    d = 0
    for t, (name, kw) in enumerate(prob["specs"]):
        J = br.DIM_F[name]
        mf, vf = e.predict_f(X[t][:40])
        lpd, ess = e.predict_log_density(t, X[t][:40], Y[t][:40])
        wl, we = log_predictive_density_rows(name, Y[t][:40], mf[:, d:d + J], np.abs(vf[:, d:d + J]), return_ess=True)
        assert np.array_equal(lpd, wl) and np.array_equal(ess, we), name
        d += J
    e.close()


# ------------------------------------------------------------------------------------------------ refusals
BAD = [(0, -1.0), (0, 0.5), (0, 8.0), (0, float("nan")), (0, float("inf")), (1, 0.0), (1, 2.5), (1, 2e9), (1, float("nan"))]


@pytest.mark.parametrize("col,bad", BAD, ids=["k=%r" % b if c == 0 else "n=%r" % b for c, b in BAD])
@pytest.mark.parametrize("family", FAMILIES)
def test_rows_that_are_no_counts_out_of_trials_are_refused(family, col, bad):
    """k in {-1, 0.5, n + 1, NaN, inf}, n in {0, 2.5, 2e9, NaN}: refused with the family's name by every entry point that takes y; the
    task's N is unchanged, and a valid call right after succeeds."""
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows, log_predictive_density_rows
    good = np.array([[0.0, 3.0], [7.0, 7.0], [2.0, 40.0]])
    Y = good.copy()
    Y[1, col] = bad
    J = br.DIM_F[family]
    m, v, X = np.zeros((3, J)), np.ones((3, J)), np.linspace(0, 1, 3)[:, None]
    e = Engine([(family, {})], 1, 8, 1)
    e.set_data([X], [good])
    for call in (lambda: var_exp(family, Y, m, v), lambda: log_predictive_rows(family, Y, m, v, num_samples=8),
                 lambda: log_predictive_density_rows(family, Y, m, v), lambda: e.set_data([X[:2]], [Y[:2]])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert family + ":" in str(ei.value)
    assert e.N[0] == 3
    assert np.all(np.isfinite(var_exp(family, good, m, v)[0]))
    e.set_data([X], [good])
    e.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_a_one_column_y_is_refused(family):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp, log_predictive_rows
    good = np.array([[0.0, 3.0], [7.0, 7.0], [2.0, 40.0], [1.0, 1.0]])
    J = br.DIM_F[family]
    m, v, X = np.zeros((4, J)), np.ones((4, J)), np.linspace(0, 1, 4)[:, None]
    e = Engine([(family, {})], 1, 8, 1)
    e.set_data([X], [good])
    for one in (good[:, :1], good[:, 0]):
        for call in (lambda: var_exp(family, one, m, v), lambda: log_predictive_rows(family, one, m, v, num_samples=8),
                     lambda: e.set_data([X], [one])):
            with pytest.raises(_lib.InvalidArgument) as ei:
                call()
            assert family + ":" in str(ei.value)
    assert e.N[0] == 4
    assert np.all(np.isfinite(var_exp(family, good, m, v)[0]))
    e.close()


@pytest.mark.parametrize("family", FAMILIES)
def test_no_cdf_no_parameters_and_the_trial_count_is_checked(family):
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine, var_exp_dparam, predictive_cdf_rows, predictive_quantile_rows, predictive, sample
    J = br.DIM_F[family]
    good, m, v = np.array([[1.0, 2.0], [0.0, 5.0]]), np.zeros((2, J)), np.ones((2, J))
    with pytest.raises(_lib.InvalidArgument) as ei:
        var_exp_dparam(family, good, m, v)
    assert "no parameters of its own" in str(ei.value)
    for call in (lambda: predictive_cdf_rows(family, good[:, 0], m, v), lambda: predictive_quantile_rows(family, m, v, [0.5])):
        with pytest.raises(_lib.InvalidArgument) as ei:
            call()
        assert "incomplete beta" in str(ei.value) and family in str(ei.value)
    prm, prob, X, Y = _case(3, [(family, {})], [30], 8, 1, 1)
    e = mc.make_engine(prob, X, Y)
    assert e.lik_param_count(0) == 0
    mc.run(e, prm)
    with pytest.raises(_lib.InvalidArgument) as ei:
        e.predict_cdf(0, X[0], Y[0][:, 0])
    assert "incomplete beta" in str(ei.value)
    e.close()
    for bad in (0.5, -1.0, float("nan"), 2e9):
        for call in (lambda: predictive(family, m, v, pred_trials=bad), lambda: sample(family, m, pred_trials=bad),
                     lambda: Engine([(family, {"pred_trials": bad})], 1, 8, 1)):
            with pytest.raises(_lib.InvalidArgument) as ei:
                call()
            assert family + ":" in str(ei.value) and "trial count" in str(ei.value)


# ------------------------------------------------------------------------------------------------ whole model vs oracle
SET_B = [BN]
SET_BB = [BB]
SET_MIXED = [("Gaussian", {"sigma": 0.5}), BN, BB, ("Poisson", {})]
SET_TABLE = [BN, BB, WB, NB, ("Dirichlet", {"K": 3})]
_STAND_IN = {"Binomial": ("Bernoulli", {}), "BetaBinomial": ("Gamma", {}), "Weibull": ("Gamma", {}), "NegBinomial": ("Gamma", {})}


def _case(seed, specs, Ns, M, Q, P, hi=60):
    """model_cases.family_case with a stand-in of the same dim_f for every task of a family the synthetic generator of the oracle does
    not know; then, from RandomState(seed + 2) in task order, their observations are replaced -- Binomial / Beta-Binomial by (N, 2)
    rows, Weibull by short times with 30 % censored, Negative Binomial by counts -- and the problem is made for the real specs."""
    from oracle import svmogp_oracle as so
    prm, _, X, Y = mc.family_case(seed, [_STAND_IN.get(s[0], s) for s in specs], Ns, M, Q, P)
    rng = np.random.RandomState(seed + 2)
    for t, (name, kw) in enumerate(specs):
        if name in FAMILIES:
            Y[t] = br.count_rows(rng, name, Ns[t], hi)
        elif name == "Weibull":
            Y[t] = wr.draw(rng, np.full(Ns[t], np.log(1.5e-3)), np.full(Ns[t], np.log(1.3)), 0.3)
        elif name == "NegBinomial":
            Y[t] = rng.poisson(3.0 * rng.gamma(2.0, 0.5, (Ns[t], 1))).astype(float)
    return prm, so.make_problem(specs, Q, M, P), X, Y


SHAPES = [(16, 1, 1), (100, 3, 1), (128, 3, 2)]
CASES = [(s, M, Q, P) for s in (SET_B, SET_BB, SET_MIXED) for M, Q, P in SHAPES]


@pytest.mark.parametrize("specs,M,Q,P", CASES, ids=["%s-M%d-Q%d-P%d" % ("+".join(n for n, _ in c[0]), c[1], c[2], c[3]) for c in CASES])
def test_elbo_grad_vs_oracle(specs, M, Q, P):
    """One row pool, several, and a minibatch with row_begin > 0 (both columns of the task's image, and lc, are read with the TASK's
    stride and offset)."""
    Ns = [300, 257, 129, 200][:len(specs)]
    mc.check_vs_oracle(_case(5100 + M + 7 * Q + P, specs, Ns, M, Q, P), Ns)


def test_small_model_path_carries_the_families():
    """M = 48: the families' singleton instantiations of quad_multi_kernel and the captured graph, against the regular kernels."""
    Ns = [300, 257, 129]
    mc.check_small_vs_regular(_case(577, [("Gaussian", {"sigma": 0.5}), BN, BB], Ns, 48, 2, 1), Ns, ([60, 50, 20], [160, 137, 129]))


def test_strict_qf_vs_literal_oracle():
    mc.check_strict_vs_literal(_case(531, [BN, BB, ("HetGaussian", {})], [400, 300, 257], 128, 2, 1))


def test_mixed_with_the_other_table_families():
    """Binomial, Beta-Binomial, Weibull, Negative Binomial and Dirichlet(3) in one model: a set outside the baseline masks, so
    launch_quad_multi takes its generic path with the five singleton instantiations behind each other."""
    from oracle import svmogp_oracle as so
    Ns = [300, 257, 129, 200, 150]
    prm, prob, X, Y = _case(5500, SET_TABLE, Ns, 16, 2, 1)
    want = so.elbo_grad_fused(prm, prob, X, Y)
    e = mc.make_engine(prob, X, Y)
    mc._parity(mc.run(e, prm), want, "table families M = 16 ")
    e.close()


def test_split_step_equals_the_plain_call_bit_for_bit():
    specs = [("Gaussian", {"sigma": 0.5}), BN, BB]
    Ns = [300, 257, 129]
    prm, prob, X, Y = _case(61, specs, Ns, 64, 2, 1)
    e = mc.make_engine(prob, X, Y, small_path=False)
    full = mc.run(e, prm)
    e.step_begin(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"], W=prm["W"],
                 kappa=prm["kappa"])
    out = e.step_finish()
    for k in mc.KEYS:
        assert np.array_equal(np.asarray(out[k]), np.asarray(full[k])), k
    e.close()


def test_collapse_at_model_level():
    """A Binomial task of 40 rows with n <= 6 against a Bernoulli task holding the same rows repeated n times: ELBO - sum lc and every
    gradient agree.  The bound per output is 100 x the difference the ORACLE shows between the two formulations on the CPU (float64
    summation order: n equal addends against one product).  Where the oracle reproduces an output exactly (the ELBO: the sum over the
    rows' ve is taken in an order that does not depend on the formulation) that bound is 0 and the assertion is exact equality on the
    device too: intended, it is what "collapsed into one" promises for an output whose addends are the same numbers.  Measured on the CPU, 2026-10-19, max |a - b| / max |b|
    per output: elbo 0, g_m_u 1.5e-16, g_L_u 1.6e-15, g_variance 1.9e-15, g_lengthscale 4.0e-16, g_W 1.5e-16, g_kappa 1.2e-16, g_Z 6.3e-16
    (tests/test_binom_cpu.py::test_collapse_at_model_level_in_the_oracle re-measures and prints them; the device showed 0 ... 1.5e-15)."""
    from oracle import svmogp_oracle as so
    prm, (pa, Xa, Ya), (pb, Xb, Yb), sum_lc = br.collapse_pair()
    oracle = br.collapse_differences(so.elbo_grad_fused(prm, pa, Xa, Ya), so.elbo_grad_fused(prm, pb, Xb, Yb), sum_lc)
    ea, eb = mc.make_engine(pa, Xa, Ya), mc.make_engine(pb, Xb, Yb)
    got = br.collapse_differences(mc.run(ea, prm), mc.run(eb, prm), sum_lc)
    ea.close(), eb.close()
    for k in got:
        bound = 100.0 * oracle[k]
        print("collapse at model level, %-14s device %.3g  oracle %.3g  bound %.3g" % (k, got[k], oracle[k], bound))
        assert got[k] <= bound, (k, got[k], bound)


# ------------------------------------------------------------------------------------------------ facade end to end
def _toy(seed):
    rng = np.random.RandomState(seed)
    Xa, Xb = np.sort(rng.rand(300, 1), 0), np.sort(rng.rand(250, 1), 0)
    na, nb = rng.randint(1, 41, 300), rng.randint(5, 61, 250)
    pa = 1.0 / (1.0 + np.exp(-2.0 * np.sin(2.0 * np.pi * Xa[:, 0])))
    pb = rng.beta(np.exp(1.0 + 0.8 * np.cos(2.0 * np.pi * Xb[:, 0])), np.exp(1.2 - 0.5 * np.cos(2.0 * np.pi * Xb[:, 0])))
    return [Xa, Xb], [np.stack([rng.binomial(na, pa), na], 1).astype(float), np.stack([rng.binomial(nb, pb), nb], 1).astype(float)]


def _model_prm(model):
    return dict(Z=model.Z.values, m_u=model.q_u_means.values, L_flat=model.q_u_chols.values,
                variance=np.array([float(k.variance[0]) for k in model.kern_list]),
                lengthscale=np.array([float(k.lengthscale[0]) for k in model.kern_list]),
                W=np.stack([np.ravel(B.W.values) for B in model.B_list]), kappa=np.stack([np.ravel(B.kappa.values) for B in model.B_list]))


def test_facade_end_to_end():
    import hetmogp_amd as H
    from oracle import svmogp_oracle as so
    X, Y = _toy(23)
    trials = 25
    likelihood = H.HetLikelihood([H.Binomial(pred_trials=trials), H.BetaBinomial(pred_trials=trials)])
    md = likelihood.generate_metadata()
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.array([0.9, 0.3, 0.5])[:, None], np.array([0.1, 0.6, 0.4])[:, None]]
    np.random.seed(0)
    model = H.HetMOGP(X=X, Y=Y, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood, Y_metadata=md, W_list=W_list)
    model.parameters_changed()
    prm = _model_prm(model)
    specs = [(n, {}) for n, _ in likelihood.specs()]
    want = so.elbo_grad_fused(prm, so.make_problem(specs, Q, M, 1), X, Y)
    assert_parity(model.log_likelihood(), want["elbo"], "elbo")
    for got, key in ((model.q_u_means.gradient, "g_m_u"), (model.q_u_chols.gradient, "g_L_u"), (model.Z.gradient, "g_Z"),
                     ([k.variance.gradient[0] for k in model.kern_list], "g_variance"),
                     ([k.lengthscale.gradient[0] for k in model.kern_list], "g_lengthscale"),
                     (np.stack([B.W.gradient.ravel() for B in model.B_list]), "g_W"),
                     (np.stack([B.kappa.gradient.ravel() for B in model.B_list]), "g_kappa")):
        assert_parity(np.asarray(got, float).reshape(np.shape(want[key])), want[key], key)
    e0 = float(model.log_likelihood()[0, 0])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)      # (the optimiser view's Logexp inverse of kappa = 0 is log(0): not these families')
        model.optimize(max_iters=30)
    e1 = float(model.log_likelihood()[0, 0])
    assert np.isfinite(e1) and e1 > e0, (e0, e1)
    Xp = [np.linspace(0, 1, 37)[:, None]] * 2
    mean, var = model.predictive(Xp)
    for t in range(2):
        assert mean[t].shape == (37, 1) and np.all(np.isfinite(mean[t])) and np.all(np.isfinite(var[t]))
        assert np.all((mean[t] >= 0.0) & (mean[t] <= trials)) and np.all(var[t] > 0.0)
    Xt, Yt = [x[:50] for x in X], [y[:50] for y in Y]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        lpd = model.log_predictive_density(Xt, Yt)
        nlpd = model.negative_log_predictive(Xt, Yt, method="quadrature")
    assert all(np.shape(a)[0] == 50 and np.all(np.isfinite(a)) for a in lpd) and np.isfinite(nlpd)
    for fam in FAMILIES:
        with pytest.raises(NotImplementedError, match=fam):
            model.predict_quantiles(Xp, tasks=None) if fam == "Binomial" else model.predict_quantiles(Xp, tasks=[1])
