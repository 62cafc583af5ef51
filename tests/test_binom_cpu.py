"""CPU: the Binomial and Beta-Binomial likelihoods of DESIGN 9l at the layers that need no device -- the C enum, the ctypes ids, the
descriptors, the host-side refusals of the C ABI, the synthetic generator -- and the yardstick itself: the float64 restatement
tests/binom_ref.py against the 50-digit one (tests/binom_ref_mp.py) on the committed grid tests/golden/bngrid.npz, under the criterion
of DESIGN 9a, |got - R| <= C 2^-52 S per element.  The constants C_ORACLE live in tests/binom_ref.py with their raw figures and date."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
from scipy import stats

import binom_ref as br
import likgrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
FAMILIES = ("Binomial", "BetaBinomial")


def _f64(g, family):
    with np.errstate(all="ignore"):
        return br.stack(*br.var_exp(family, g["y"], g["m"], g["v"]))


# ---------------------------------------------------------------------------------------------------- ids, descriptors, shapes
def test_header_python_and_engine_ids_agree():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_BINOMIAL\s*=\s*13\b", src) and re.search(r"\bHMOGP_LIK_BETABINOMIAL\s*=\s*14\b", src)
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump
    from hetmogp_amd import _lib, engine, synthetic
    assert _lib.lib.hmogp_abi_version() == 8
    for name, lid, J in (("Binomial", 13, 1), ("BetaBinomial", 14, 2)):
        assert getattr(_lib, "LIK_" + name.upper()) == lid and _lib.LIK_IDS_BY_NAME[name] == lid and engine.LIK_IDS[name] == lid
        assert engine.lik_dim_f(name) == J and engine.lik_dim_y(name) == 2 and synthetic._dim_f(name, {}) == J
        assert engine.lik_param(name) == 1.0 and engine.lik_param(name, pred_trials=12) == 12.0


def test_y_must_be_n_by_2():
    from hetmogp_amd import _lib, engine
    for name in FAMILIES:
        assert engine._y_rows(name, [[1, 2], [0, 5]]).shape == (2, 2)
        for bad in (np.zeros(4), np.zeros((4, 1)), np.zeros((2, 3)), np.zeros((2, 2, 1))):
            with pytest.raises(_lib.InvalidArgument, match=name):
                engine._y_rows(name, bad)


def test_descriptor_metadata_and_specs():
    from hetmogp_amd import HetLikelihood, Gaussian, Binomial, BetaBinomial
    b, bb = Binomial(), BetaBinomial(gp_link=None, pred_trials=30)
    assert b.get_metadata() == (2, 1, 1) and bb.get_metadata() == (2, 2, 1)
    assert b.name == "Binomial" and bb.name == "BetaBinomial" and b.kwargs() == {"pred_trials": 1} and bb.kwargs() == {"pred_trials": 30}
    assert b.learnable_params() == [] and bb.learnable_params() == [] and not b.ismulti()
    md = HetLikelihood([Gaussian(), b, bb]).generate_metadata()
    assert md["function_index"].tolist() == [0, 1, 2, 2] and md["d_index"].tolist() == [0, 0, 0, 1] and md["pred_index"].tolist() == [0, 1, 2]


def test_no_predictive_cdf():
    from hetmogp_amd import engine, Binomial
    for name in FAMILIES:
        assert "incomplete beta" in engine.PREDQ_MISSING[name]
        with pytest.raises(NotImplementedError, match=name + ".*incomplete beta"):
            engine.predq_require(name)
    with pytest.raises(NotImplementedError, match="Binomial"):
        Binomial().predictive_cdf(np.zeros(1), np.zeros(1), np.ones(1))


def test_host_side_refusals_need_no_device():
    """The trial count n* of predictive / sample and the cdf's refusal are decided on the host, before the device is asked for: the same
    HMOGP_E_INVALID with or without one."""
    from hetmogp_amd import _lib
    lib = _lib.lib
    a = np.full(4, 0.5)
    p = a.ctypes.data_as(_lib.c_double_p)
    for lid, name in ((_lib.LIK_BINOMIAL, b"Binomial"), (_lib.LIK_BETABINOMIAL, b"BetaBinomial")):
        for bad in (0.5, -1.0, float("nan"), 2e9):
            assert lib.hmogp_predictive(0, lid, bad, 0, 1, p, p, p, p) == _lib.E_INVALID
            assert name + b":" in lib.hmogp_last_error(None) and b"trial count" in lib.hmogp_last_error(None)
            assert lib.hmogp_sample(0, lid, bad, 1, ctypes.c_uint64(0), p, p) == _lib.E_INVALID
            assert lib.hmogp_var_exp(0, lid, bad, 1, p, p, p, p, p, p) == _lib.E_INVALID
        assert lib.hmogp_predictive_cdf(0, lid, 1.0, 0, 1, p, p, p, p, p) == _lib.E_INVALID
        assert b"incomplete beta" in lib.hmogp_last_error(None) and name in lib.hmogp_last_error(None)
        assert lib.hmogp_predictive_quantile(0, lid, 1.0, 0, 1, 1, p, p, p, p) == _lib.E_INVALID


def test_synthetic_rows():
    from hetmogp_amd.synthetic import make_case, binomial_counts
    prm, X, Y = make_case([("Binomial", {"trials": (3, 40)}), ("BetaBinomial", {})], [4000, 3000], M=16, Q=2, seed=4)
    assert prm["W"].shape == (2, 3)
    for y, lo, hi in ((Y[0], 3, 40), (Y[1], 1, 30)):
        k, n = y[:, 0], y[:, 1]
        assert y.shape[1] == 2 and np.all(y == np.floor(y)) and np.all((k >= 0) & (k <= n))
        assert n.min() == lo and n.max() == hi and abs(n.mean() - 0.5 * (lo + hi)) < 5.0 * (hi - lo) / np.sqrt(12.0 * len(n))
    rng = np.random.RandomState(0)
    F = np.tile([[0.4, -0.2]], (20000, 1))
    for name, f in (("Binomial", F[:, :1]), ("BetaBinomial", F)):
        y = binomial_counts(rng, name, f, 50, 50)
        mu, vr, _ = br.moments(name, 50, F[0, :br.DIM_F[name]])
        assert abs(y[:, 0].mean() - mu) < 5.0 * np.sqrt(vr / len(y)), name
    assert binomial_counts(rng, "BetaBinomial", F, 50, 50)[:, 0].var() > 2.0 * binomial_counts(rng, "Binomial", F[:, :1], 50, 50)[:, 0].var()
    with pytest.raises(ValueError):
        binomial_counts(rng, "Binomial", F[:, :1], 0, 5)


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_small_and_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "bngrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    assert os.path.getsize(br.GRID) < 64 * 1024


def test_fixture_regenerates_bit_identically():
    """Every input of every row, R and S of every Binomial row and of every fourth Beta-Binomial row (such a row costs 0.17 s at 50
    digits, 400 nodes with three special functions of a + b each; tools/make_binom_grid.py writes all of them)."""
    spec = importlib.util.spec_from_file_location("make_binom_grid", os.path.join(ROOT, "tools", "make_binom_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    every = {"Binomial": 1, "BetaBinomial": 4}
    new, old = mod.build(every=every), np.load(br.GRID)
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        step = every["Binomial" if k.startswith("b_") else "BetaBinomial"] if k[-1] in "RS" else 1
        a, b = new[k][::step], old[k][::step]
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), k


def _regimes(y, r):
    """Which of nb_gamma_diffs' three regimes a call (y, r) takes: 0 sums, 1 Stirling, 2 plain."""
    return np.where(y <= 32, 0, np.where(r >= 16.0, 1, 2))


def test_grid_design():
    for family in FAMILIES:
        g = br.load_grid(family)
        y, m, v, e = g["y"], g["m"], g["v"], g["cls"] != br.BULK
        k, n = y[:, 0], y[:, 1]
        assert np.all(np.isfinite(g["R"])) and np.all(np.isfinite(g["S"])) and np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
        assert np.all((n >= 1) & (n <= 1e9) & (k >= 0) & (k <= n)) and np.all(y == np.floor(y))          # what the library accepts
        b = ~e
        assert b.sum() >= 64 and np.all(np.abs(m[b]) <= 1.5) and np.all((v[b] >= 1e-3) & (v[b] <= 0.5)) and n[b].max() <= 2000
        assert np.any(n[b] > 32) and np.any(n[b] <= 32)
        pairs = set(zip(k[e].tolist(), n[e].tolist()))
        assert {(0.0, 1.0), (1.0, 1.0), (0.0, 32.0), (32.0, 32.0), (0.0, 33.0), (33.0, 33.0), (0.0, 1e9), (1.0, 1e9), (5e8, 1e9), (1e9, 1e9)} <= pairs
        assert {750.0, -750.0} <= set(np.ravel(m[e]).tolist()) and {0.0, 1e-300} <= set(np.ravel(v[e]).tolist())
        assert g["S"].max() < 1e11                                                                # lgamma(1e9 + 1) = 2e10 is the largest addend
        if family == "Binomial":
            assert {25.0, -25.0} <= set(m[e & (v[:, 0] == 0.0), 0].tolist())                      # p at both clips
            assert np.array_equal(g["cls"] == br.CLIP, e & (np.abs(m[:, 0]) >= 25.0)) and (g["cls"] == br.CLIP).sum() == 64
        else:
            assert not np.any(g["cls"] == br.CLIP)
            assert {21.0, -21.0} <= set(m[e][:, 0].tolist()) and {21.0, -21.0} <= set(m[e][:, 1].tolist())   # a, b at 1e-9 and 1e9
            for col in ((1, 0), (0, 1), (1, 1)):                                                  # v = 0 / 1e-300 in either dimension and in both
                for tiny in (0.0, 1e-300):
                    assert np.any(e & np.all((v == tiny) == np.array(col, bool), 1)), (col, tiny)
            s = br.alpha(m[:, 0]) + br.alpha(m[:, 1])
            exact = e & np.all(v == 0.0, 1)
            seen = set(_regimes(n[exact], s[exact]).tolist())
            assert seen == {0, 1, 2}, seen                                                        # G(n, s): all three regimes at v = 0
            assert np.any(exact & (n == 33) & (s > 15.0) & (s < 16.0)) and np.any(exact & (n == 33) & (s > 16.0) & (s < 17.0))
            assert np.any(exact & (n == 32) & (s < 16.0)) and np.any(exact & (n == 32) & (s > 16.0))


def test_restatements_agree():
    """Where C_ORACLE comes from: the float64 restatement against the 50-digit R, per family, class and output (raw figures printed).
    Every element is finite; there is no exceptions list and no non-finite share."""
    for family in FAMILIES:
        g = br.load_grid(family)
        br.assert_grid(family, _f64(g, family), g, br.c_oracle, "binom_ref on bngrid")
        assert max(br.c_oracle(family, br.BULK, o) for o in range(len(br.OUTPUTS[family]))) <= 16.0
        raw = br.worst(family, _f64(g, family), g)
        for c in raw:                                                                             # the recorded raw figures are this grid's
            assert np.allclose(raw[c], br.C_ORACLE_RAW[(family, c)], rtol=0.25, atol=0.6), (family, c, raw[c])


def test_float64_scale_matches_high_precision_scale():
    for family in FAMILIES:
        g = br.load_grid(family)
        assert np.allclose(br.var_exp_scale(family, g["y"], g["m"], g["v"]), g["S"], rtol=1e-9, atol=0.0), family


def test_a_result_moved_by_twice_the_bound_is_caught():
    for family in FAMILIES:
        g = br.load_grid(family)
        for o in range(len(br.OUTPUTS[family])):
            for c in sorted(set(g["cls"].tolist())):
                i = int(np.where(g["cls"] == c)[0][3])
                got = g["R"].copy()
                br.assert_grid(family, got, g, br.c_kernel, "R itself")
                got[i, o] += 2.0 * br.c_kernel(family, c, o) * br.EPS * g["S"][i, o]
                assert got[i, o] != g["R"][i, o]
                with pytest.raises(AssertionError, match=br.OUTPUTS[family][o]):
                    br.assert_grid(family, got, g, br.c_kernel, "moved")


def test_plain_lgamma_difference_is_seen_by_the_grid():
    """Seeded corruption in the spirit of the power-before-logarithm check: G formed as the plain float64 difference of two lgammas.  On
    the rows with a (or b) at 1e9 the Beta-Binomial's ve then leaves the KERNEL's bound, not merely the oracle's."""
    g = br.load_grid("BetaBinomial")
    y, m, v = g["y"], g["m"], g["v"]
    rows = np.where((g["cls"] == br.EDGE) & ((m[:, 0] == 21.0) | (m[:, 1] == 21.0)) & (y[:, 1] <= 2000) & (y[:, 0] > 0) & (y[:, 0] < y[:, 1]))[0]
    assert len(rows) >= 6
    bound = np.array([br.c_kernel("BetaBinomial", br.EDGE, 0)] * len(rows))
    clean = br.ratios(br.stack(*br.bb_var_exp(y[rows], m[rows], v[rows])), g["R"][rows], g["S"][rows])[:, 0]
    assert np.all(clean <= bound)

    def corrupted(yy, rr):
        out = list(br.gamma_diffs(yy, rr))
        out[0] = br.plain_diffs(yy, rr)[0]
        return tuple(out)
    bad = br.ratios(br.stack(*br.bb_var_exp(y[rows], m[rows], v[rows], diffs=corrupted)), g["R"][rows], g["S"][rows])[:, 0]
    print("plain G: rows beyond C_KERNEL %d of %d, worst by a factor %.3g" % ((bad > bound).sum(), len(rows), (bad / bound).max()))
    assert (bad / bound).max() >= 1e3 and (bad > bound).sum() >= len(rows) // 2


# ---------------------------------------------------------------------------------------------------- properties of the model
def test_ve_at_vanishing_variance_is_the_textbook_pmf():
    rng = np.random.RandomState(3)
    N = 300
    n = rng.randint(1, 300, N).astype(float)
    m = rng.uniform(-3.0, 3.0, (N, 2))
    k = br.draw(rng, "Binomial", n, m[:, :1])
    Y = np.stack([k, n], 1)
    p = br.prob(m[:, 0])[0]
    assert np.all((p > 1e-9) & (p < 1.0 - 1e-9))                                                  # inside the clips
    ve = br.binom_var_exp(Y, m[:, 0], np.zeros(N))[0]
    assert np.allclose(ve, stats.binom.logpmf(k, n, p), rtol=1e-11, atol=1e-11)
    ve = br.bb_var_exp(Y, m, np.zeros((N, 2)))[0]
    assert np.allclose(ve, stats.betabinom.logpmf(k, n, np.exp(m[:, 0]), np.exp(m[:, 1])), rtol=1e-10, atol=1e-10)


def test_derivative_formulas_against_central_differences():
    """All six: Binomial's d1, d2 and the Beta-Binomial's four, against central differences of SciPy's logpmf.  logpmf carries ~1e-12
    absolute: first differences at h = 1e-4 are good to 1e-8 (rounding) + 1e-7 (truncation), second ones at h = 1e-3 to 1e-6 + 1e-5; the
    bounds are ten times that, relative to 1 + |value| (a wrong factor in any formula is an error of order one)."""
    rng = np.random.RandomState(4)
    N = 400
    n = rng.randint(1, 200, N).astype(float)
    f0, f1 = rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N)
    k = br.draw(rng, "BetaBinomial", n, np.stack([f0, f1], 1))
    h, q = 1e-4, 1e-3
    sig = lambda f: 1.0 / (1.0 + np.exp(-f))
    ref = lambda a: stats.binom.logpmf(k, n, sig(a))
    _, d1, d2 = br.binom_terms(k, n, f0)
    checks = [(d1, (ref(f0 + h) - ref(f0 - h)) / (2 * h), 1e-6), (d2, (ref(f0 + q) - 2 * ref(f0) + ref(f0 - q)) / q ** 2, 1e-4)]
    ref = lambda a, b: stats.betabinom.logpmf(k, n, np.exp(a), np.exp(b))
    _, g0, h0, g1, h1 = br.bb_logpdf_and_derivatives(k, n, f0, f1)
    checks += [(g0, (ref(f0 + h, f1) - ref(f0 - h, f1)) / (2 * h), 1e-6), (g1, (ref(f0, f1 + h) - ref(f0, f1 - h)) / (2 * h), 1e-6),
               (h0, (ref(f0 + q, f1) - 2 * ref(f0, f1) + ref(f0 - q, f1)) / q ** 2, 1e-4),
               (h1, (ref(f0, f1 + q) - 2 * ref(f0, f1) + ref(f0, f1 - q)) / q ** 2, 1e-4)]
    for i, (got, num, tol) in enumerate(checks):
        worst = np.max(np.abs(got - num) / (1.0 + np.abs(got)))
        print("derivative formula %d: worst |formula - central difference| / (1 + |.|) = %.3g (bound %g)" % (i, worst, tol))
        assert worst < tol, i


def test_collapse_identity():
    """ve - lc, dm, dv of (k, n) equal k x Bernoulli's at y = 1 plus (n - k) x Bernoulli's at y = 0 at the same (m, v) -- the oracle's own
    Bernoulli -- within the sum of the constants times their scales: the restatement's bulk constant on the Binomial side, Bernoulli's
    oracle constant (tests/likgrid.py) on the other, one more rounding each for the subtraction of lc and the products."""
    from oracle import likelihoods_oracle as lo
    Y, m, v = br.bulk_rows("Binomial", 1000, seed=21)
    k, n = Y[:, 0], Y[:, 1]
    got = br.stack(*br.binom_var_exp(Y, m[:, 0], v[:, 0]))
    got[:, 0] -= br.log_choose(k, n)
    one, zero = br.stack(*lo.bernoulli(np.ones(len(k)), m[:, 0], v[:, 0])), br.stack(*lo.bernoulli(np.zeros(len(k)), m[:, 0], v[:, 0]))
    want = k[:, None] * one + (n - k)[:, None] * zero
    Y1, Y0 = np.stack([np.ones_like(k), np.ones_like(k)], 1), np.stack([np.zeros_like(k), np.ones_like(k)], 1)
    Sb, Se = br.binom_scale(Y, m, v), k[:, None] * br.binom_scale(Y1, m, v) + (n - k)[:, None] * br.binom_scale(Y0, m, v)
    cb = likgrid.c_oracle("Bernoulli")[likgrid.BULK]
    for o, name in enumerate(br.OUTPUTS["Binomial"]):
        bound = br.EPS * ((br.c_oracle("Binomial", br.BULK, o) + 1.0) * Sb[:, o] + (cb[o] + 2.0) * Se[:, o])
        d = np.abs(got[:, o] - want[:, o])
        print("collapse identity, %-2s: worst |difference| / bound = %.3g" % (name, np.max(d / bound)))
        assert np.all(d <= bound), name
    Yn1 = np.stack([(np.arange(50) % 2).astype(float), np.ones(50)], 1)                           # n = 1: Bernoulli itself, up to the order of the sum
    a, b = br.stack(*br.binom_var_exp(Yn1, m[:50, 0], v[:50, 0])), br.stack(*lo.bernoulli(Yn1[:, 0], m[:50, 0], v[:50, 0]))
    assert br.ratios(a, b, br.binom_scale(Yn1, m[:50], v[:50])).max() <= 4.0


def test_binomial_limit_of_the_beta_binomial():
    """a = c p, b = c (1 - p), c = 1e9, v = 0: log p differs from Binomial's by O(n^2 / c) in the model (the Beta's variance) plus the
    restatement's own bound, the edge constant of ve times 2^-52 S."""
    rng = np.random.RandomState(6)
    N = 200
    n = rng.randint(1, 60, N).astype(float)
    p = rng.uniform(0.05, 0.95, N)
    k = rng.binomial(n.astype(int), p).astype(float)
    Y = np.stack([k, n], 1)
    m = np.stack([np.log(1e9 * p), np.log(1e9 * (1.0 - p))], 1)
    assert np.all(m < np.log(1e9))                                                                # inside Beta's clips
    ve = br.bb_var_exp(Y, m, np.zeros((N, 2)))[0]
    want = stats.binom.logpmf(k, n, p)
    model = n * n / 1e9 / np.minimum(p, 1.0 - p)
    bound = model + (br.c_oracle("BetaBinomial", br.EDGE, 0) + br.c_oracle("Binomial", br.BULK, 0)) * br.EPS * br.bb_scale(Y, m, np.zeros((N, 2)))[:, 0]
    d = np.abs(ve - want)
    print("Binomial limit: worst |BetaBinomial - Binomial| / bound = %.3g (worst difference %.3g)" % (np.max(d / bound), d.max()))
    assert np.all(d <= bound)
    plain = br.bb_var_exp(Y, m, np.zeros((N, 2)), diffs=br.plain_diffs)[0]                        # ... which the plain differences miss
    assert np.max(np.abs(plain - want) / bound) > 10.0


def test_predictive_moments():
    """The T = 20 rule against a 200-node one (the integrand is smooth: 1e-9 for v <= 0.5), and the closed forms at v = 0."""
    rng = np.random.RandomState(8)
    N = 100
    for family in FAMILIES:
        J = br.DIM_F[family]
        m, v = rng.uniform(-1.5, 1.5, (N, J)), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, J)))
        for trials in (1, 12, 1000):
            a, b = br.predictive(family, m, v, trials), br.predictive(family, m, v, trials, T=200)
            assert np.allclose(a[0], b[0], rtol=1e-8) and np.allclose(a[1], b[1], rtol=1e-6), (family, trials)
            mean, var = br.predictive(family, m, np.zeros_like(v), trials)
            if family == "Binomial":
                p = br.prob(m[:, 0])[0]
                wm, wv = trials * p, trials * p * (1.0 - p)
            else:
                a_, b_ = np.exp(m[:, 0]), np.exp(m[:, 1])
                s, mu = a_ + b_, a_ / (a_ + b_)
                wm, wv = trials * mu, trials * mu * (1.0 - mu) * (s + trials) / (s + 1.0)
            assert np.allclose(mean[:, 0], wm, rtol=1e-13) and np.allclose(var[:, 0], wv, rtol=1e-12), (family, trials)
            assert np.allclose(wm[0], br.moments(family, trials, m[0])[0], rtol=1e-10) and np.allclose(wv[0], br.moments(family, trials, m[0])[1], rtol=1e-9)


@pytest.mark.parametrize("family,N,seed", [("Binomial", 256, 9013), ("BetaBinomial", 64, 9014)])
def test_lpd_ess_warn_is_measured(family, N, seed):
    """LPD_ESS_WARN of the two families, measured as the comment above that table describes: every seeded row whose rule misses the
    integral (150 and 120 nodes per dimension agree to 1e-4) by more than 1e-2 has ess below the constant, and the constant flags at
    most 10 % of the rows within 1e-4.  Raw figures 2026-10-19: Binomial 2.041 (23 of 232 rows beyond 1e-2), BetaBinomial 5.992 (2 of 64)."""
    from hetmogp_amd.likelihoods import lpd_ess_warn
    y, m, v = br.envelope_rows(family, N, seed)
    a, e, _ = br.lpd(family, y, m, v)
    d1, d2 = br.lpd_dense(family, y, m, v, 150), br.lpd_dense(family, y, m, v, 120)
    ok, err = np.abs(d1 - d2) <= 1e-4, np.abs(a - d1)
    bad, good = ok & (err > 1e-2), ok & (err <= 1e-4)
    warn = lpd_ess_warn(family)
    print("[envelope] %-12s rows used %d of %d; largest ess of a row beyond 1e-2: %.3f (LPD_ESS_WARN %.1f); rows within 1e-4 it flags: %d of %d"
          % (family, ok.sum(), N, e[bad].max(), warn, (e[good] < warn).sum(), good.sum()))
    assert ok.mean() >= 0.5 and bad.any()
    assert np.all(e[bad] < warn) and warn <= np.ceil(e[bad].max() * 10.0 + 1.0) / 10.0             # measured, rounded up to one decimal
    assert (e[good] < warn).mean() <= 0.10


def test_collapse_at_model_level_in_the_oracle():
    """The figure the device test's bound is made of: the difference the oracle itself shows between a Binomial task and the Bernoulli
    task holding the same rows repeated n times (printed per output)."""
    from oracle import svmogp_oracle as so
    with br.in_the_oracle():
        prm, (pa, Xa, Ya), (pb, Xb, Yb), sum_lc = br.collapse_pair()
        assert Yb[0].shape[0] == int(Ya[0][:, 1].sum()) and Ya[0][:, 1].max() <= 6 and len(Ya[0]) == 40
        d = br.collapse_differences(so.elbo_grad_fused(prm, pa, Xa, Ya), so.elbo_grad_fused(prm, pb, Xb, Yb), sum_lc)
    print("collapse at model level, oracle: " + ", ".join("%s %.2g" % kv for kv in sorted(d.items())))
    assert max(d.values()) <= 1e-13
