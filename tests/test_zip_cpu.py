"""CPU: the zero-inflated Poisson likelihood of DESIGN 9n at the layers that need no device -- the C enum, the ctypes ids, the descriptor,
the synthetic generator, the host-side refusals -- and the yardstick itself: the float64 restatement tests/zip_ref.py against the
high-precision one (tests/zip_ref_mp.py) on the committed grid tests/golden/zipgrid.npz, under the criterion of DESIGN 9a,
|got - R| <= C 2^-52 S per element, with g and g (rho - pi) each counted as ONE addend of S.

C_ORACLE: zip_ref.C_ORACLE_RAW (measured 2026-10-20, per class and per output, every element), rounded up to a power of two; the kernels
get max(16, 4 C_ORACLE).  The designed rows at which pi comes within 6e-9 of a clip are a class of their own ("clip"), as Binomial's are
in DESIGN 9l: log(1 - pi) at a pi rounded next to 1 sets Bernoulli's 2^27 there, and the expression shapes are Bernoulli's on purpose.

Corruption check (test_plain_difference_for_g_is_seen_by_the_grid), 2026-10-20: with g = (1 - rho) - pi the twelve edge rows with
lambda in {1e-12, 1e-6} miss the kernel bound of dm_1 (16) by factors 4.2e3 .. 9.0e10, and no ve moves by a bit."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import likgrid
import zip_ref as zr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
BULK, EDGE, CLIP = zr.BULK, zr.EDGE, zr.CLIP
PREDICTIVE_TOL = 2e-7


# ---------------------------------------------------------------------------------------------------- ids, descriptor, generator
def test_header_python_and_engine_ids_agree():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_ZIPOISSON\s*=\s*15\b", src)
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump
    from hetmogp_amd import _lib, engine, synthetic
    assert _lib.LIK_ZIPOISSON == 15 and _lib.LIK_IDS_BY_NAME["ZIPoisson"] == 15 and engine.LIK_IDS["ZIPoisson"] == 15
    assert engine.lik_dim_f("ZIPoisson") == 2 and engine.lik_dim_y("ZIPoisson") == 1 and engine.lik_param("ZIPoisson") == 0.0
    assert synthetic._dim_f("ZIPoisson", {}) == 2
    assert sorted(_lib.LIK_IDS_BY_NAME.values()) == list(range(16))                # no id taken twice


def test_descriptor_metadata_and_specs():
    from hetmogp_amd import HetLikelihood, Gaussian, ZIPoisson, Categorical
    d = ZIPoisson()
    assert d.get_metadata() == (1, 2, 1) and d.ismulti() is False and d.kwargs() == {} and d.name == "ZIPoisson"
    assert ZIPoisson(gp_link=None).learnable_params() == []
    h = HetLikelihood([Gaussian(), ZIPoisson(), Categorical(K=3)])
    md = h.generate_metadata()
    assert md["y_index"].tolist() == [0, 1, 2] and md["function_index"].tolist() == [0, 1, 1, 2, 2]
    assert md["d_index"].tolist() == [0, 0, 1, 0, 1] and md["pred_index"].tolist() == [0, 1, 2, 2]
    assert h.specs()[1] == ("ZIPoisson", {})


def test_synthetic_counts_have_more_zeros_than_their_rate_explains():
    """The same seed draws the same latent functions for a Poisson and a ZIPoisson task (both rates are exp of the clipped first
    function): the zero share of the zero-inflated task exceeds Poisson's."""
    from hetmogp_amd.synthetic import make_case
    prm, X, Y = make_case([("Gaussian", {"sigma": 0.5}), ("ZIPoisson", {})], [50, 4000], M=16, Q=2, seed=4)
    _, _, Yp = make_case([("Gaussian", {"sigma": 0.5}), ("Poisson", {})], [50, 4000], M=16, Q=2, seed=4)
    y = Y[1]
    assert y.shape == (4000, 1) and np.all(y >= 0.0) and np.all(y == np.floor(y)) and prm["W"].shape == (2, 3)
    z, zp = float(np.mean(y == 0.0)), float(np.mean(Yp[1] == 0.0))
    print("zero share: ZIPoisson %.3f, Poisson at its own rate %.3f" % (z, zp))
    assert z > zp + 0.1 and y.max() > 1.0


def test_refusals_need_no_device():
    """Observations that are no counts are refused on the host, before the device is asked for: the same HMOGP_E_INVALID with or
    without one.  So is the predictive cdf."""
    from hetmogp_amd import _lib, engine, ZIPoisson
    lib = _lib.lib
    a = np.full(4, 0.5)
    p = a.ctypes.data_as(_lib.c_double_p)
    for bad in (-1.0, 2.5, float("nan"), float("inf")):
        y = np.array([0.0, bad, 3.0, 1.0])
        py = y.ctypes.data_as(_lib.c_double_p)
        assert lib.hmogp_var_exp(0, _lib.LIK_ZIPOISSON, 0.0, 2, py, p, p, p, p, p) == _lib.E_INVALID
        assert b"ZIPoisson" in lib.hmogp_last_error(None)
        assert lib.hmogp_log_predictive(0, _lib.LIK_ZIPOISSON, 0.0, 2, 8, ctypes.c_uint64(0), py, p, p, p) == _lib.E_INVALID
        assert lib.hmogp_log_predictive_gh(0, _lib.LIK_ZIPOISSON, 0.0, 0, 2, py, p, p, p, None) == _lib.E_INVALID
        assert b"ZIPoisson" in lib.hmogp_last_error(None)
    assert "incomplete gamma" in engine.PREDQ_MISSING["ZIPoisson"]
    with pytest.raises(NotImplementedError, match="ZIPoisson.*incomplete gamma"):
        engine.predq_require("ZIPoisson")
    with pytest.raises(NotImplementedError, match="ZIPoisson"):
        ZIPoisson().predictive_cdf(np.zeros(1), np.zeros((1, 2)), np.ones((1, 2)))
    assert lib.hmogp_predictive_cdf(0, _lib.LIK_ZIPOISSON, 0.0, 0, 1, p, p, p, p, p) == _lib.E_INVALID
    assert b"incomplete gamma" in lib.hmogp_last_error(None) and b"ZIPoisson" in lib.hmogp_last_error(None)


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_small_and_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "zipgrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    assert os.path.getsize(zr.GRID) <= 32232                                               # the largest of the family grids before it


def test_fixture_regenerates_bit_identically():
    spec = importlib.util.spec_from_file_location("make_zip_grid", os.path.join(ROOT, "tools", "make_zip_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.build(), zr.load_grid()
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


def test_grid_design():
    g = zr.load_grid()
    y, m, v, cls = g["y"], g["m"], g["v"], g["cls"]
    assert np.all(np.isfinite(g["R"])) and np.all(np.isfinite(g["S"])) and np.all(np.isfinite(g["lpd"]))   # no exception list
    assert np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
    assert np.all((y >= 0) & (y == np.floor(y)))                                          # what the library accepts
    b, e = cls == BULK, cls != BULK
    assert 90 <= b.sum() <= 110 and 80 <= e.sum() <= 110
    assert np.all(np.abs(m[b]) <= 3.0) and np.all((v[b] >= 1e-3) & (v[b] <= 4.0))
    assert (y[b] == 0).sum() >= 30 and (y[b] >= 1).sum() >= 30
    x_max = np.polynomial.hermite.hermgauss(20)[0].max()
    assert np.array_equal(cls == CLIP, e & (np.abs(m[:, 1]) + x_max * np.sqrt(2.0 * v[:, 1]) >= 19.0))
    assert {0.0, 1.0, 32.0, 1000.0, 1e6} <= set(y[e].tolist())
    for yy in (0.0, 1.0, 32.0, 1000.0, 1e6):                                               # every y against every f0
        assert {750.0, -750.0, 709.78, 400.0, 355.0, 37.0, -37.0} <= set(m[e & (y == yy)][:, 0].tolist())
    for yy in (0.0, 1.0, 32.0):
        assert {20.7, -20.7, 21.0, -21.0, 750.0, -750.0} <= set(m[e & (y == yy)][:, 1].tolist())
    z = e & (y == 0.0) & np.all(v == 0.0, 1)
    with np.errstate(all="ignore"):
        p = zr.zero_prob(m[:, 1])[1]
        u = np.log(zr.one_minus_pi(m[:, 1])) - zr.rate(m[:, 0]) - np.log(p)
    assert np.any(z & (u == 0.0)) and np.any(z & (u > 0) & (u < 2e-9)) and np.any(z & (u < 0) & (u > -2e-9))
    assert np.any(z & (np.abs(u + 40.0) < 1e-6)) and np.any(z & (u > 20.7))                # far to either side (u cannot exceed 20.72)
    lam = zr.rate(m[:, 0])
    for want in (1e-12, 1e-6):
        assert (e & (y == 0) & np.isclose(lam, want, rtol=1e-9, atol=0.0)).sum() >= 6
    assert v[e].min() == 0.0 and v[e].max() == 1e4 and np.any(e & np.all(v == 0.0, 1)) and np.any(e & np.all(v == 1e4, 1))


def test_float64_restatement_against_high_precision_grid():
    """Where C_ORACLE comes from: the raw figures, per class and per output, are printed and must round up to the constants in use.  Also:
    no non-finite element anywhere, no exception list, and no bulk constant above 16."""
    g = zr.load_grid()
    got = zr.pack(*zr.var_exp(g["y"], g["m"], g["v"]))
    assert np.all(np.isfinite(got)), np.argwhere(~np.isfinite(got))[:8]                    # the non-finite share is zero
    w = zr.assert_grid(g, got, zr.c_oracle, "zip_ref on zipgrid")
    assert max(zr.c_oracle(BULK, o) for o in range(6)) <= 16.0
    for c, fig in w.items():                                                               # the recorded raw figures are what is measured
        for o, x in enumerate(fig):
            assert x <= 1.02 * zr.C_ORACLE_RAW[c][o] and zr.c_oracle(c, o) <= 2.0 * zr._pow2_up(max(x, 1.0)), (c, o, x)


def test_float64_lpd_against_the_grid():
    g = zr.load_grid()
    lpd, ess = zr.lpd(g["y"], g["m"], g["v"])
    assert np.all(np.isfinite(lpd)) and np.all((ess >= 1.0 - 1e-12) & (ess <= 400.0))
    zr.assert_rows(lpd, g["lpd"], zr.lpd_scale(g["y"], g["m"], g["v"]), g["cls"], zr.c_oracle, "zip_ref lpd on zipgrid", outputs=("lpd",))


def test_float64_scale_matches_high_precision_scale():
    g = zr.load_grid()
    S = zr.var_exp_scale(g["y"], g["m"], g["v"])
    assert np.allclose(S, g["S"], rtol=1e-9, atol=1e-300)


def test_plain_difference_for_g_is_seen_by_the_grid():
    """Seeded corruption: g replaced by the plain difference (1 - rho) - pi.  The edge rows with lambda <= 1e-6 then land beyond the KERNEL
    bound in dm_1 (not merely beyond C_ORACLE), and no ve column moves."""
    g = zr.load_grid()
    y, m, v, cls = g["y"], g["m"], g["v"], g["cls"]
    lam = zr.rate(m[:, 0])
    rows = np.where((cls == EDGE) & (y == 0.0) & (np.isclose(lam, 1e-12, rtol=1e-9, atol=0.0) | np.isclose(lam, 1e-6, rtol=1e-9, atol=0.0)))[0]
    assert len(rows) == 12
    clean = zr.pack(*zr.var_exp(y, m, v))
    bad = zr.pack(*zr.var_exp(y, m, v, plain_g=True))
    assert np.array_equal(clean[:, 0], bad[:, 0]) and np.array_equal(clean[:, [1, 3]], bad[:, [1, 3]])     # ve, dm_0, dv_0 do not move
    r_clean, r_bad = zr.ratios(clean, g["R"], g["S"])[rows], zr.ratios(bad, g["R"], g["S"])[rows]
    bound = zr.c_kernel(EDGE, 2)
    assert np.all(r_clean[:, 2] <= bound)
    print("plain g: dm_1 beyond C_KERNEL = %g by factors %.3g .. %.3g on the %d rows" % (bound, (r_bad[:, 2] / bound).min(),
                                                                                       (r_bad[:, 2] / bound).max(), len(rows)))
    assert np.all(r_bad[:, 2] > bound)


# ---------------------------------------------------------------------------------------------------- properties of the model
def test_log_density_and_derivatives_against_the_textbook_pmf():
    """The five expressions of the contract against log(pi [y = 0] + (1 - pi) poisson.pmf) and its central differences at moderate
    arguments.  The textbook form carries ~1e-13 absolute: first differences at h = 1e-4 are good to 1e-9 (rounding) + 1e-7 (truncation),
    second differences at h = 1e-3 to 1e-7 + 1e-5; the bounds are ten times that, as in DESIGN 9h."""
    from scipy import stats
    rng = np.random.RandomState(3)
    y = np.where(rng.rand(200) < 0.5, 0.0, rng.randint(1, 30, 200)).astype(float)
    f0, f1 = rng.uniform(-2.0, 3.0, 200), rng.uniform(-3.0, 3.0, 200)
    lp, d0, h0, d1, h1 = zr.logpdf_and_derivatives(y, f0, f1)

    def ref(a, b):
        pi = 1.0 / (1.0 + np.exp(-b))
        return np.log(pi * (y == 0.0) + (1.0 - pi) * stats.poisson.pmf(y, np.exp(a)))
    assert np.allclose(lp, ref(f0, f1), rtol=1e-11, atol=1e-11)
    h, k = 1e-4, 1e-3
    for got, num, tol in ((d0, (ref(f0 + h, f1) - ref(f0 - h, f1)) / (2 * h), 1e-6), (d1, (ref(f0, f1 + h) - ref(f0, f1 - h)) / (2 * h), 1e-6),
                          (h0, (ref(f0 + k, f1) - 2 * ref(f0, f1) + ref(f0 - k, f1)) / k ** 2, 1e-4),
                          (h1, (ref(f0, f1 + k) - 2 * ref(f0, f1) + ref(f0, f1 - k)) / k ** 2, 1e-4)):
        assert np.max(np.abs(got - num) / (1.0 + np.abs(got))) < tol


def test_derivatives_are_those_of_ve():
    """dm, dv of the 20-node rule against central differences, in m and in v, of a FINER rule's ve (T = 32 per dimension), as in DESIGN 9h:
    h = 1e-4 leaves a truncation of 1e-8 relative to values of order one and a rounding of 1e-11; the bound is ten times the truncation."""
    rng = np.random.RandomState(12)
    N = 60
    m = rng.uniform(-2.0, 2.5, (N, 2))
    v = np.exp(rng.uniform(np.log(1e-3), np.log(0.3), (N, 2)))
    y = zr.draw(rng, m[:, 0], m[:, 1])
    assert (y == 0).sum() >= 10 and (y > 0).sum() >= 10
    _, dm, dv = zr.var_exp(y, m, v)
    h = 1e-4
    fine = lambda mm, vv: zr.var_exp(y, mm, vv, T=32)[0]
    worst = 0.0
    for k in range(2):
        e = np.zeros(2)
        e[k] = h
        fm = (fine(m + e, v) - fine(m - e, v)) / (2 * h)
        hv = h * v[:, k]
        ev = np.zeros((N, 2))
        ev[:, k] = hv
        fv = (fine(m, v + ev) - fine(m, v - ev)) / (2 * hv)
        scale = 1.0 + np.abs(fm) + np.abs(fv)
        worst = max(worst, np.max(np.abs(dm[:, k] - fm) / scale), np.max(np.abs(dv[:, k] - fv) / scale))
    print("worst |derivative - central difference of the finer rule| / (1 + |.|) = %.3g" % worst)
    assert worst <= 1e-7


def test_separable_and_tensor_rules_agree_on_positive_rows():
    """The contract of a row with y >= 1 is the sum of two 20-node rules; the 20 x 20 tensor rule of the same log-density is the same
    number up to rounding, because the weights sum to 1: within (C_ORACLE + 8) 2^-52 S (400 addends against 40)."""
    y, m, v = zr.bulk_rows(np.random.RandomState(7), 400)
    pos = y > 0
    assert pos.sum() >= 100
    a, b = zr.pack(*zr.var_exp(y[pos], m[pos], v[pos])), zr.pack(*zr.var_exp(y[pos], m[pos], v[pos], tensor=True))
    r = zr.ratios(a, b, zr.var_exp_scale(y[pos], m[pos], v[pos]))
    print("separable against tensor rule, worst ratio per output: " + " ".join("%.3g" % x for x in r.max(0)))
    assert np.all(r.max(0) <= np.array([zr.c_oracle(BULK, o) + 8.0 for o in range(5)]))


def test_poisson_limit():
    """pi on its lower clip (m1 = -30, v1 = 1e-6: pi = 1e-9 at every node) and m0 <= 0.  y = 0: log p0 - (-lambda) = log(1 - pi + pi e^lambda)
    = log(1 + pi (e^lambda - 1)), which lies in [0, pi (e^lambda - 1)]: 0 <= ve - ve_Poisson <= 1e-9 sum w_i expm1(lambda_i).  y >= 1: the
    difference is log(1 - 1e-9) exactly.  Rounding allowance: 8 2^-52 of the row's scale."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(5)
    N = 300
    m0, v0 = rng.uniform(-3.0, 0.0, N), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), N))
    y = rng.poisson(np.exp(m0)).astype(float)
    assert (y == 0).sum() >= 50 and (y > 0).sum() >= 50
    m, v = np.stack([m0, np.full(N, -30.0)], 1), np.stack([v0, np.full(N, 1e-6)], 1)
    ve = zr.var_exp(y, m, v)[0]
    pve = lo.poisson(y, m0, v0)[0].reshape(-1)
    x, w = zr.gh()
    lam = np.exp(x[None, :] * np.sqrt(2.0 * v0)[:, None] + m0[:, None])
    slack = 8.0 * zr.EPS * zr.var_exp_scale(y, m, v)[:, 0]
    d = ve - pve
    z = y == 0
    assert np.all(d[z] >= -slack[z]) and np.all(d[z] <= 1e-9 * (np.expm1(lam[z]) * w).sum(1) + slack[z])
    assert np.all(np.abs(d[~z] - np.log1p(-1e-9)) <= slack[~z])
    assert np.max(np.abs(d)) > 1e-10                                                        # ... and the two are not the same function


def test_predictive_against_quadrature_of_the_conditional_moments():
    """mean = E[(1 - pi) lambda], variance = E[(1 - pi)(lambda + lambda^2)] - mean^2 under q(f0) q(f1), by 120-node Gauss-Hermite rules.  The
    moments of lambda are closed forms; pbar is the contract's 20-node rule of the sigmoid, whose convergence at v1 <= 2 sets the tolerance,
    PREDICTIVE_TOL = 2e-7: measured 2026-10-20 on these 200 rows, mean 6.0e-8, variance 5.3e-8 relative (tests/test_zip_gpu.py uses the same)."""
    rng = np.random.RandomState(8)
    N = 200
    m = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-3.0, 3.0, N)], 1)
    v = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (N, 2)))
    x, w = zr.gh(120)
    lam = np.exp(x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])
    q = 1.0 - zr.zero_prob(x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[1]
    e1, e2, eq = lam @ w, (lam * lam) @ w, q @ w
    mean, var = zr.predictive(m, v)
    assert mean.shape == (N, 1) and var.shape == (N, 1)
    wm = eq * e1
    wv = eq * (e1 + e2) - wm * wm
    em, ev = np.max(np.abs(mean[:, 0] - wm) / wm), np.max(np.abs(var[:, 0] - wv) / wv)
    print("predictive against 120-node rules: mean %.3g, variance %.3g (relative)" % (em, ev))
    assert em <= PREDICTIVE_TOL and ev <= PREDICTIVE_TOL
    mean, var = zr.predictive(m, np.zeros_like(v))                                         # v = 0: the moments at f = m
    mu, vr, _ = zr.moments(m[:, 0], m[:, 1])
    assert np.allclose(mean[:, 0], mu, rtol=1e-13) and np.allclose(var[:, 0], vr, rtol=1e-10)
    for T in (10, 20):
        assert np.allclose(zr.predictive(m, v, T=T)[0][:, 0], wm, rtol=1e-3)                # (gh_T = 10: a coarser rule of the same thing)
    mean, var = zr.predictive(np.array([[800.0, 0.0]]), np.array([[1.0, 1.0]]))            # overflow is +inf
    assert np.isposinf(mean[0, 0]) and np.isposinf(var[0, 0])


def test_lpd_ess_warn_is_measured():
    """LPD_ESS_WARN["ZIPoisson"] by the rule of DESIGN 9j: the largest ess, rounded up to one decimal, among the seeded bulk rows whose
    20 x 20 rule misses the integral (150 and 120 nodes per dimension agree to 1e-4) by more than 1e-2; at most 10 % of the rows may be
    left out because the dense rules disagree, and the constant flags at most 10 % of the rows within 1e-4.  Raw figure 2026-10-20:
    10.607 (7 of the 505 rows used; 7 of 512 left out; 0 of 475 good rows flagged)."""
    from hetmogp_amd.likelihoods import lpd_ess_warn
    N = 512
    y, m, v = zr.envelope_rows(N, 9015)
    a, e = zr.lpd(y, m, v)
    d1, d2 = zr.lpd_dense(y, m, v, 150), zr.lpd_dense(y, m, v, 120)
    ok, err = np.abs(d1 - d2) <= 1e-4, np.abs(a - d1)
    bad, good = ok & (err > 1e-2), ok & (err <= 1e-4)
    warn = lpd_ess_warn("ZIPoisson")
    print("[envelope] ZIPoisson rows used %d of %d; largest ess of a row beyond 1e-2: %.3f over %d rows (LPD_ESS_WARN %.1f); rows within "
          "1e-4 it flags: %d of %d" % (ok.sum(), N, e[bad].max(), bad.sum(), warn, (e[good] < warn).sum(), good.sum()))
    assert (~ok).mean() <= 0.10 and bad.any()
    assert np.all(e[bad] < warn) and warn <= np.ceil(e[bad].max() * 10.0 + 1.0) / 10.0             # measured, rounded up to one decimal
    assert (e[good] < warn).mean() <= 0.10


def test_outputs_are_finite_at_the_corners():
    for y in (0.0, 1.0, 33.0, 1e6):
        for m0 in (750.0, -750.0, 0.0):
            for m1 in (750.0, -750.0, 21.0, -21.0, 0.0):
                for v0 in (0.0, 1e4):
                    out = zr.pack(*zr.var_exp(np.array([y]), np.array([[m0, m1]]), np.array([[v0, v0]])))
                    assert np.all(np.isfinite(out)), (y, m0, m1, v0)
                    assert np.isfinite(zr.lpd(np.array([y]), np.array([[m0, m1]]), np.array([[v0, v0]]))[0][0]), (y, m0, m1, v0)
