"""CPU: the float64 restatement of the predictive cdf, survival function and quantiles of DESIGN 9k (tests/pquant_ref.py) against the
50-digit grid tests/golden/pqgrid.npz, the grid's regeneration, the criterion's teeth, closed forms and limits, monotonicity, the
restatement's own quantiles, and the four new symbols of the C ABI."""
import json
import os
import sys

import numpy as np
import pytest
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import make_pquant_grid as mg      # noqa: E402
import pquant_ref as pq            # noqa: E402

EPS = pq.EPS
PROBS = (0.025, 0.5, 0.975, 1e-12, 1.0 - 1e-7)
CONT = tuple(f for f in pq.FAMILIES if f not in pq.DISCRETE)


def _blocks():
    return pq.load_grid()


# ------------------------------------------------------------------------------------------------ the grid
def test_restatement_against_the_grid():
    seen = set()
    for b in _blocks():
        c, s = pq.cdf_sf(b.name, b.y, b.m, b.v, **b.kw)
        pq.assert_block(c, s, b, pq.c_oracle(b.name), "float64 %s" % b.tag)
        seen.add(b.name)
    assert seen == set(pq.FAMILIES)


def test_grid_has_the_edge_classes_the_design_names():
    g = {b.tag: b for b in _blocks()}
    n = sum(b.n for b in g.values())
    assert 200 <= n <= 600 and os.path.getsize(pq.GRID) < 64 * 1024
    for b in g.values():
        e = b.cls == pq.EDGE
        assert e.any() and (b.v[e] == 0.0).all(1).any(), b.tag
        if b.n > e.sum():
            bulk = ~e
            assert (np.abs(b.m[bulk]) <= 3.0).all() and (b.v[bulk] >= 1e-3).all() and (b.v[bulk] <= 4.0).all(), b.tag
    for tag in ("gaussian", "hetgaussian", "exponential", "ordinal4", "weibull"):
        R = g[tag].R
        for col in (0, 1):
            assert ((R[:, col] > 2.0 ** -1022) & (R[:, col] < 1e-100)).any(), (tag, col)     # a tail below 1e-100 that is still normal
    for tag in ("bernoulli", "exponential", "weibull"):
        assert (g[tag].y == 0.0).any() and (g[tag].y < 0.0).any(), tag                      # at and below the support's edge
    assert {1.0, 4.0} <= set(g["ordinal4"].y.tolist())                                       # the end categories
    w = g["weibull"]
    assert ((w.R[:, 1] == 0.0) & (w.y == 1e300)).any()                                       # z at its clip: sf = exp(-exp(680)) = 0


def test_grid_regenerates_bit_for_bit():
    g = np.load(pq.GRID)
    assert json.loads(str(g["spec"])) == [[b[0], b[1], b[2]] for b in mg.BLOCKS]
    rng = np.random.RandomState(20261019)
    for b in mg.BLOCKS:
        y, m, v, cls = mg.rows_of(b)
        for k, a in (("y", y), ("m", m), ("v", v), ("cls", cls)):
            assert np.array_equal(g["%s__%s" % (b[0], k)], a, equal_nan=True), (b[0], k)
        for i in rng.choice(len(cls), min(6, len(cls)), replace=False):
            R, S = mg.value_of(b, y[i], m[i], v[i])
            assert np.array_equal(g[b[0] + "__R"][i], R, equal_nan=True) and np.array_equal(g[b[0] + "__S"][i], S), (b[0], i)


def test_float64_scale_agrees_with_the_50_digit_scale():
    for b in _blocks():
        S = pq.scale(b.name, b.y, b.m, b.v, **b.kw)
        assert np.allclose(S, b.S, rtol=1e-9, atol=0.0), (b.tag, np.abs(S / b.S - 1.0).max())
        assert (b.S >= 1.0).all()


def test_a_result_moved_by_twice_the_constant_is_caught():
    for b in _blocks():
        C_ = pq.c_oracle(b.name)
        for col in (0, 1):
            Cc = np.array([C_[c][col] for c in b.cls], float)
            ok = np.isfinite(b.R[:, col]) & (b.R[:, col] > 2.0 ** -1000) & (b.R[:, col] != 1.0)
            assert ok.any()
            moved = b.R.copy()
            moved[:, col] = np.where(ok, b.R[:, col] * (1.0 + 2.0 * Cc * EPS * b.S[:, col]), b.R[:, col])
            with pytest.raises(AssertionError):
                pq.assert_block(moved[:, 0], moved[:, 1], b, C_, "moved %s" % b.tag)
            pq.assert_block(b.R[:, 0], b.R[:, 1], b, C_, "exact %s" % b.tag)


# ------------------------------------------------------------------------------------------------ closed forms and limits
def test_gaussian_against_scipy():
    y, m, v = pq.bulk_rows("Gaussian", 200, 11, sigma=0.5)
    c, s = pq.cdf_sf("Gaussian", y, m, v, sigma=0.5)
    sd = np.sqrt(0.25 + v[:, 0])
    np.testing.assert_allclose(c, stats.norm.cdf(y, m[:, 0], sd), rtol=1e-13)
    np.testing.assert_allclose(s, stats.norm.sf(y, m[:, 0], sd), rtol=1e-13)
    q = pq.quantile("Gaussian", m, v, [0.025, 0.5, 0.975], sigma=0.5)
    np.testing.assert_allclose(q, m + stats.norm.ppf([0.025, 0.5, 0.975])[None, :] * sd[:, None], rtol=1e-13, atol=1e-14)
    c0, _ = pq.cdf_sf("Gaussian", y, m, v, sigma=None)                  # no sigma, or one <= 0, means 0.5
    c1, _ = pq.cdf_sf("Gaussian", y, m, v, sigma=-1.0)
    assert np.array_equal(c0, c) and np.array_equal(c1, c)


@pytest.mark.parametrize("name", pq.FAMILIES)
def test_v_zero_is_the_conditional_pair(name):
    kw = dict(pq.BULK_KW.get(name, {}))
    y, m, _ = pq.bulk_rows(name, 64, 21, **kw)
    c, s = pq.cdf_sf(name, y, m, np.zeros_like(m), **kw)
    f0 = m[:, 0]
    if name == "Gaussian":
        wc, ws = stats.norm.cdf(y, f0, 0.5), stats.norm.sf(y, f0, 0.5)
    elif name == "HetGaussian":
        wc, ws = stats.norm.cdf(y, f0, np.exp(0.5 * m[:, 1])), stats.norm.sf(y, f0, np.exp(0.5 * m[:, 1]))
    elif name == "Bernoulli":
        p = 1.0 / (1.0 + np.exp(-f0))
        wc, ws = np.where(y < 1.0, 1.0 - p, 1.0), np.where(y < 1.0, p, 0.0)
    elif name == "Exponential":
        wc, ws = stats.expon.cdf(y, scale=np.exp(-f0)), stats.expon.sf(y, scale=np.exp(-f0))
    elif name == "Ordinal":
        ext = np.concatenate([pq.edges_of(**kw), [np.inf]])[y.astype(int) - 1]
        wc, ws = stats.norm.cdf(ext - f0), stats.norm.sf(ext - f0)
    else:
        wc, ws = stats.weibull_min.cdf(y, np.exp(m[:, 1]), scale=np.exp(f0)), stats.weibull_min.sf(y, np.exp(m[:, 1]), scale=np.exp(f0))
    np.testing.assert_allclose(c, wc, rtol=2e-12, atol=1e-300)
    np.testing.assert_allclose(s, ws, rtol=2e-12, atol=1e-300)


def test_hetgaussian_at_v1_zero_is_a_gaussian():
    y, m, v = pq.bulk_rows("HetGaussian", 64, 22)
    v[:, 1] = 0.0
    c, s = pq.cdf_sf("HetGaussian", y, m, v)
    sd = np.sqrt(v[:, 0] + np.exp(m[:, 1]))
    np.testing.assert_allclose(c, stats.norm.cdf(y, m[:, 0], sd), rtol=1e-12)
    np.testing.assert_allclose(s, stats.norm.sf(y, m[:, 0], sd), rtol=1e-12)


def test_weibull_at_shape_one_is_the_exponential():
    y, m1, v1 = pq.bulk_rows("Exponential", 64, 23)
    m, v = np.hstack([-m1, np.zeros_like(m1)]), np.hstack([v1, np.zeros_like(v1)])      # scale lambda = b = exp(-f), k = exp(0) = 1
    cw, sw = pq.cdf_sf("Weibull", y, m, v)
    ce, se = pq.cdf_sf("Exponential", y, m1, v1)
    np.testing.assert_allclose(cw, ce, rtol=1e-11)
    np.testing.assert_allclose(sw, se, rtol=1e-11)
    qw, qe = pq.quantile("Weibull", m, v, [0.1, 0.5, 0.9]), pq.quantile("Exponential", m1, v1, [0.1, 0.5, 0.9])
    np.testing.assert_allclose(qw, qe, rtol=1e-11)


@pytest.mark.parametrize("name", pq.FAMILIES)
def test_cdf_plus_sf_is_one_in_the_bulk(name):
    kw = dict(pq.BULK_KW.get(name, {}))
    y, m, v = pq.bulk_rows(name, 200, 24, **kw)
    c, s = pq.cdf_sf(name, y, m, v, **kw)
    assert (np.abs(c + s - 1.0) <= 64.0 * EPS).all(), (name, np.abs(c + s - 1.0).max())
    c10, s10 = pq.cdf_sf(name, y, m, v, gh_T=10, **kw)
    assert (np.abs(c10 + s10 - 1.0) <= 64.0 * EPS).all()


def test_support_edges_and_non_finite():
    for name in ("Exponential", "Weibull", "Bernoulli"):
        J = pq.dim_f(name)
        m, v = np.full((4, J), 0.3), np.full((4, J), 0.5)
        c, s = pq.cdf_sf(name, np.array([-1.0, -0.0, 0.0, np.nan]), m, v)
        assert c[0] == 0.0 and s[0] == 1.0 and np.isnan(c[3]) and np.isnan(s[3])
        if name != "Bernoulli":
            assert c[1] == c[2] == 0.0 and s[1] == s[2] == 1.0
    c, s = pq.cdf_sf("Bernoulli", np.array([1.0, 7.0]), np.zeros((2, 1)), np.ones((2, 1)))
    assert (c == 1.0).all() and (s == 0.0).all()
    q = pq.quantile("Gaussian", np.zeros((2, 1)), np.ones((2, 1)), [0.0, 1.0, -0.1, np.nan, 0.5], sigma=0.5)
    assert np.isnan(q[:, :4]).all() and (np.abs(q[:, 4]) < 1e-15).all()


# ------------------------------------------------------------------------------------------------ monotonicity
@pytest.mark.parametrize("name", pq.FAMILIES)
def test_monotone_in_y_and_in_p(name):
    kw = dict(pq.BULK_KW.get(name, {}))
    _, m, v = pq.bulk_rows(name, 12, 31, **kw)
    if name == "Ordinal":
        ys = np.arange(1.0, 5.0)
    elif name in ("Gaussian", "HetGaussian"):
        ys = np.linspace(-30.0, 30.0, 61)
    else:
        ys = np.concatenate([[-1.0, 0.0], np.exp(np.linspace(-30.0, 12.0, 60))])
    for n in range(m.shape[0]):
        c, s = pq.cdf_sf(name, ys, np.repeat(m[n:n + 1], len(ys), 0), np.repeat(v[n:n + 1], len(ys), 0), **kw)
        S = pq.scale(name, ys, np.repeat(m[n:n + 1], len(ys), 0), np.repeat(v[n:n + 1], len(ys), 0), **kw)
        slack_c, slack_s = 8.0 * EPS * S[:, 0] * c, 8.0 * EPS * S[:, 1] * s
        assert (np.diff(c) >= -slack_c[1:]).all() and (np.diff(s) <= slack_s[:-1]).all(), (name, n)
    probs = np.array([1e-12, 1e-3, 0.025, 0.3, 0.5, 0.5 + 1e-9, 0.7, 0.975, 1.0 - 1e-9])
    q = pq.quantile(name, m, v, probs, **kw)
    ok = pq.in_range(name, q)
    assert ok[:, 2:8].all()
    d = np.diff(np.where(ok, q, np.nan), axis=1)
    assert (d[np.isfinite(d)] >= 0.0).all(), name
    if name not in pq.DISCRETE:
        assert (d[:, 2:7] > 0.0).all()


# ------------------------------------------------------------------------------------------------ quantiles of the restatement
@pytest.mark.parametrize("name", CONT)
def test_restatement_quantiles_meet_the_criterion(name):
    """Both routes of the restatement -- the kernels' solver restated step by step, and SciPy's bracketing solver on the restatement's
    cdf / sf -- meet the mixed criterion with the restatement's own constant (its F is exact for itself; the constant pays for the
    solver's stopping rule), and never use more than the budget."""
    kw = dict(pq.BULK_KW.get(name, {}))
    _, m, v = pq.bulk_rows(name, 48, 41, **kw)
    b = [x for x in _blocks() if x.name == name][0]
    m, v = np.vstack([m, b.m]), np.vstack([v, b.v])
    C_ = 2.0 * max(max(t) for t in pq.c_oracle(name).values())
    got, nev = pq.quantile(name, m, v, PROBS, count=True, **kw)
    assert nev.max() <= pq.MAXEVAL and not np.isnan(got[np.isfinite(m).all(1) & np.isfinite(v).all(1)]).any()
    ex = pq.quantile_excess(name, got, m, v, PROBS, max(C_, 8.0), **kw)
    judged = pq.in_range(name, got)
    assert judged.mean() > 0.8 and (ex[judged] <= 0.0).all(), (name, np.nanmax(ex))
    print("[pquant] %-12s restated solver: mean evaluations per quantile %s, most %d" % (name, np.round(nev.mean(0), 2), nev.max()))
    sub = slice(0, 24)
    ref = pq.quantile_brentq(name, m[sub], v[sub], PROBS[:3], **kw)
    exr = pq.quantile_excess(name, ref, m[sub], v[sub], PROBS[:3], max(C_, 8.0), **kw)
    assert (exr <= 0.0).all(), (name, exr.max())
    both = pq.in_range(name, got[sub, :3])
    np.testing.assert_allclose(got[sub, :3][both], ref[both], rtol=1e-12, atol=1e-13)
    assert pq.same_out_of_range(name, got[~judged], got[~judged]).all()


@pytest.mark.parametrize("name", pq.DISCRETE)
def test_discrete_quantiles_and_no_ties_in_the_grid(name):
    rows = []
    for b in _blocks():
        if b.name != name:
            continue
        C_ = max(max(t) for t in pq.c_sum(name).values())
        ties = pq.discrete_ties(name, b.m, b.v, PROBS, C_, **b.kw)
        rows += [(b.tag, int(i), PROBS[j]) for i, j in zip(*np.nonzero(ties))]
        q = pq.quantile(name, b.m, b.v, PROBS, **b.kw)
        cum = pq.support_cdf(name, b.m, b.v, **b.kw)
        lo = 0.0 if name == "Bernoulli" else 1.0
        for j, p in enumerate(PROBS):                                   # the smallest point of the support whose cdf is >= p
            idx = (q[:, j] - lo).astype(int)
            full = np.hstack([cum, np.ones((len(cum), 1))])
            assert (np.take_along_axis(full, idx[:, None], 1)[:, 0] >= p).all()
            below = np.where(idx > 0, np.take_along_axis(full, np.maximum(idx - 1, 0)[:, None], 1)[:, 0], -1.0)
            assert (below < p).all()
    print("[pquant] %-10s rows of the grid with a cumulative probability within tol of p: %s" % (name, rows))
    assert rows == []


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbols_and_refusals_without_a_device():
    from hetmogp_amd import _lib, engine
    lib = _lib.lib
    for s in ("hmogp_predictive_cdf", "hmogp_predictive_quantile", "hmogp_predict_cdf", "hmogp_predict_quantile"):
        assert hasattr(lib, s) and s in _lib.EXPORTS, s
    assert lib.hmogp_abi_version() == 8 and _lib.ABI_VERSION == 8 and _lib.QUANT_MAXP == 8
    a = np.full(4, 0.5)
    p = a.ctypes.data_as(_lib.c_double_p)
    assert lib.hmogp_predict_cdf(None, 0, p, p, 1, 0, p, p) == _lib.E_INVALID                  # NULL handle
    assert lib.hmogp_predict_quantile(None, 0, p, 1, 1, p, 0, p) == _lib.E_INVALID
    # host-side refusals come before the device is touched: the same code with or without one
    for lik in (_lib.LIK_POISSON, _lib.LIK_GAMMA, _lib.LIK_BETA, _lib.LIK_STUDENT, _lib.LIK_NEGBINOMIAL, _lib.LIK_CATEGORICAL,
                _lib.LIK_DIRICHLET):
        assert lib.hmogp_predictive_cdf(0, lik, 3.0, 0, 1, p, p, p, p, p) == _lib.E_INVALID
        assert lib.hmogp_predictive_quantile(0, lik, 3.0, 0, 1, 1, p, p, p, p) == _lib.E_INVALID
    assert b"incomplete gamma" in lib.hmogp_last_error(None) or b"multivariate" in lib.hmogp_last_error(None)
    assert lib.hmogp_predictive_cdf(0, _lib.LIK_GAUSSIAN, 0.5, 7, 1, p, p, p, p, p) == _lib.E_INVALID          # gh_T
    for nP in (0, 9, -1):
        assert lib.hmogp_predictive_quantile(0, _lib.LIK_GAUSSIAN, 0.5, 0, 1, nP, p, p, p, p) == _lib.E_INVALID
    assert lib.hmogp_predictive_cdf(0, _lib.LIK_GAUSSIAN, 0.5, 0, 1, None, p, p, p, p) == _lib.E_INVALID       # NULL y with N > 0
    assert lib.hmogp_predictive_quantile(0, _lib.LIK_GAUSSIAN, 0.5, 0, 1, 1, p, p, p, None) == _lib.E_INVALID
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if not have:
        assert lib.hmogp_predictive_cdf(0, _lib.LIK_WEIBULL, 0.0, 0, 1, p, p, p, p, p) == _lib.E_NO_DEVICE
        assert lib.hmogp_predictive_quantile(0, _lib.LIK_EXPONENTIAL, 0.0, 0, 1, 2, p, p, p, p) == _lib.E_NO_DEVICE
        with pytest.raises(_lib.HetMOGPError) as ei:
            engine.predictive_cdf_rows("Gaussian", a, a, a, sigma=0.5)
        assert ei.value.code == _lib.E_NO_DEVICE
    with pytest.raises(NotImplementedError, match="Gamma.*incomplete gamma"):
        engine.predq_require("Gamma")
    for name in pq.REFUSED:
        with pytest.raises(NotImplementedError, match=name):
            engine.predq_require(name)
    for name in pq.FAMILIES:
        engine.predq_require(name)
