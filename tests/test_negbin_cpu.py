"""CPU: the heteroscedastic Negative Binomial likelihood of DESIGN 9h at the layers that need no device -- the C enum, the ctypes ids,
the descriptor, the synthetic generator -- and the yardstick itself: the float64 restatement tests/negbin_ref.py against the
high-precision one (tests/negbin_ref_mp.py) on the committed grid tests/golden/nbgrid.npz, under the criterion of tests/likgrid.py,
|got - R| <= C 2^-52 S  per element, with each of the differences G, D1, D2 of lgamma, psi, psi' counted as ONE addend of S.

C_ORACLE: the largest |negbin_ref - R| / (2^-52 S) over the committed grid, no element left out, per row class and output kind
(ve, dm, dv), rounded up to a power of two (a figure within 2 % of a power of two takes the next one: NumPy's exp / log differ by
an ulp between CPU generations).  Measured 2026-10-19 (NumPy / SciPy on the CPU), raw figures:
    bulk   1.67 / 0.988 / 1.61          edge   10.5 / 10.0 / 43.8
The edge figures are the rounding of f0 = m + sqrt(2 v) x_i, |f0| = 750, in y z and r p where the sigmoid has saturated (rows 165-169:
f0 = 750, dv_0) -- not folded into S, as in DESIGN 9a.  No element of the grid is non-finite and none is excepted.

Corruption check (test_plain_differences_are_seen_by_the_grid), the figures by which the plain float64 differences miss C_KERNEL on the
rows with r / y >= 1e6, 2026-10-19: G 1.26e6 x, D1 4.31e6 x, D2 1.37e5 x (worst row each; 7 of the 12 rows beyond it for each function)."""
import importlib.util
import os
import re

import numpy as np

import likgrid
import negbin_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
GRID = os.path.join(ROOT, "tests", "golden", "nbgrid.npz")
BULK, EDGE = likgrid.BULK, likgrid.EDGE
KIND = np.array([0, 1, 1, 2, 2])

C_ORACLE = {BULK: (2.0, 2.0, 2.0), EDGE: (16.0, 16.0, 64.0)}


def c_kernel():
    """The kernel's constants: max(16, 4 C_ORACLE), the rule of DESIGN 9a (wave-shuffle summation order, 1-2 ulp special functions)."""
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE.items()}


def c_kernel_vs_float64():
    """Kernel against the float64 restatement instead of R: each sits within its own constant of the true value, so the two add."""
    k = c_kernel()
    return {c: tuple(a + b for a, b in zip(k[c], C_ORACLE[c])) for c in k}


def load_grid():
    return np.load(GRID)


def assert_grid(g, got, C, what, rows=None):
    idx = np.arange(len(g["y"])) if rows is None else rows
    return likgrid.assert_rows(got, g["R"][idx], g["S"][idx], np.zeros(got.shape, np.uint8), KIND, g["cls"][idx], C, what)


def bulk_rows(rng, N):
    """Seeded bulk rows: m in [-3, 3], v log-uniform in [1e-3, 4], y drawn from the model at the row's own mean parameters."""
    m = rng.uniform(-3.0, 3.0, (N, 2))
    v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, 2)))
    return nr.draw(rng, m[:, 0], m[:, 1]), m, v


# ---------------------------------------------------------------------------------------------------- ids, descriptor
def test_header_python_and_engine_ids_agree():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_NEGBINOMIAL\s*=\s*11\b", src)
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump
    from hetmogp_amd import _lib, engine, synthetic
    assert _lib.LIK_NEGBINOMIAL == 11 and _lib.LIK_IDS_BY_NAME["NegBinomial"] == 11 and engine.LIK_IDS["NegBinomial"] == 11
    assert engine.lik_dim_f("NegBinomial") == 2 and engine.lik_dim_y("NegBinomial") == 1 and engine.lik_param("NegBinomial") == 0.0
    assert synthetic._dim_f("NegBinomial", {}) == 2


def test_descriptor_metadata_and_specs():
    from hetmogp_amd import HetLikelihood, Gaussian, NegBinomial, Categorical
    d = NegBinomial()
    assert d.get_metadata() == (1, 2, 1) and d.ismulti() is False and d.kwargs() == {} and d.name == "NegBinomial"
    assert NegBinomial(gp_link=None).learnable_params() == []
    h = HetLikelihood([Gaussian(), NegBinomial(), Categorical(K=3)])
    md = h.generate_metadata()
    assert md["y_index"].tolist() == [0, 1, 2] and md["function_index"].tolist() == [0, 1, 1, 2, 2]
    assert md["d_index"].tolist() == [0, 0, 1, 0, 1] and md["pred_index"].tolist() == [0, 1, 2, 2]
    assert h.specs()[1] == ("NegBinomial", {})


def test_synthetic_counts_are_over_dispersed_integers():
    from hetmogp_amd.synthetic import make_case
    prm, X, Y = make_case([("Gaussian", {"sigma": 0.5}), ("NegBinomial", {})], [50, 4000], M=16, Q=2, seed=4)
    y = Y[1]
    assert y.shape == (4000, 1) and np.all(y >= 0.0) and np.all(y == np.floor(y)) and prm["W"].shape == (2, 3)
    assert y.var() > y.mean() > 0.0


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_small_and_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "nbgrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    assert os.path.getsize(GRID) < likgrid.SIZE_BOUND // 8


def test_fixture_regenerates_bit_identically():
    spec = importlib.util.spec_from_file_location("make_negbin_grid", os.path.join(ROOT, "tools", "make_negbin_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.build(), load_grid()
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


def test_grid_design():
    g = load_grid()
    y, m, v, e = g["y"], g["m"], g["v"], g["cls"] == EDGE
    assert np.all(np.isfinite(g["R"])) and np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
    assert np.all((y >= 0) & (y == np.floor(y)))                                          # what the library accepts
    b = ~e
    assert b.sum() >= 64 and np.all(np.abs(m[b]) <= 3.0) and np.all((v[b] >= 1e-3) & (v[b] <= 4.0))
    assert np.any(y[b] > 32) and np.any(y[b] == 0)                                         # the bulk reaches past the sums
    assert {0.0, 1.0, 32.0, 33.0, 1000.0, 1e6} <= set(y[e].tolist())
    assert {21.0, -21.0, 750.0, -750.0} <= set(m[e][:, 1].tolist()) and {750.0, -750.0} <= set(m[e][:, 0].tolist())
    r = np.exp(np.minimum(m[e][:, 1], 21.0))
    assert np.any((r > 15.0) & (r < 16.0)) and np.any((r > 16.0) & (r < 17.0))             # both sides of the series' threshold
    ratio = r[y[e] > 0] / y[e][y[e] > 0]
    for want in (1e-6, 1.0, 1e6, 1e9):
        assert np.any(np.isclose(ratio, want, rtol=1e-9)), want
    z = m[e][:, 0] - m[e][:, 1]
    assert np.any(z == 0.0) and np.any(np.isclose(z, 1e-9, atol=1e-12) & (z != 0)) and np.any(z == 40.0) and np.any(z == -40.0)
    assert v[e].min() == 0.0 and v[e].max() == 1e4 and np.any(np.all(v[e] == 0.0, 1)) and np.any(np.all(v[e] == 1e4, 1))


def test_float64_restatement_against_high_precision_grid():
    """Where C_ORACLE comes from; also: no non-finite element anywhere (the contract's form cannot overflow once f0 is clipped at
    LIM_VAL and r lies in [1e-9, 1e9]), no exception list, no bulk row above the bulk constants, no bulk constant above 16."""
    g = load_grid()
    got = likgrid.pack(*nr.var_exp(g["y"], g["m"], g["v"]), len(g["y"]))
    assert np.all(np.isfinite(got)), np.argwhere(~np.isfinite(got))[:8]                    # the non-finite share is zero
    assert_grid(g, got, C_ORACLE, "negbin_ref on nbgrid")
    assert max(C_ORACLE[BULK]) <= 16.0


def test_float64_scale_matches_high_precision_scale():
    g = load_grid()
    S = nr.var_exp_scale(g["y"], g["m"], g["v"])
    assert np.allclose(S, g["S"], rtol=1e-12, atol=1e-300)


def test_plain_differences_are_seen_by_the_grid():
    """Seeded corruption: each of G, D1, D2 in turn replaced by the plain float64 difference of gammaln / digamma / zeta(2, .).  On the rows
    with r / y >= 1e6 the result then lands far beyond C_KERNEL (not merely beyond C_ORACLE): the grid sees the problem DESIGN 9h is about."""
    g = load_grid()
    y, m, v = g["y"], g["m"], g["v"]
    rows = np.where((g["cls"] == EDGE) & (y > 0) & (np.exp(np.minimum(m[:, 1], 21.0)) >= 1e6 * np.maximum(y, 1.0)) & (v[:, 1] <= 1e-3)
                    & (np.abs(m[:, 0]) < 100.0))[0]
    assert len(rows) >= 6
    bound = np.array([[c_kernel()[c][k] for k in KIND] for c in g["cls"][rows]])
    clean = likgrid.ratios(likgrid.pack(*nr.var_exp(y[rows], m[rows], v[rows]), len(rows)), g["R"][rows], g["S"][rows],
                           np.zeros((len(rows), 5), np.uint8))
    assert np.all(clean <= bound)
    for which, name, cols in ((0, "G", [0]), (1, "D1", [2, 4]), (2, "D2", [4])):
        def corrupted(yy, rr, which=which):
            out = list(nr.gamma_diffs(yy, rr))
            out[which] = nr.plain_diffs(yy, rr)[which]
            return tuple(out)
        got = likgrid.pack(*nr.var_exp(y[rows], m[rows], v[rows], diffs=corrupted), len(rows))
        r = likgrid.ratios(got, g["R"][rows], g["S"][rows], np.zeros(got.shape, np.uint8))
        excess = (r / bound)[:, cols].max(1)
        print("plain %-2s: rows beyond C_KERNEL %d of %d, worst by a factor %.3g" % (name, int((excess > 1.0).sum()), len(rows), excess.max()))
        assert excess.max() >= 1e3, (name, excess)
        other = [c for c in range(5) if c not in cols and not (which == 1 and c == 4)]
        assert np.all(r[:, other] <= bound[:, other]), name                               # ... and nothing else moved


# ---------------------------------------------------------------------------------------------------- properties of the model
def test_log_density_and_derivatives_against_the_textbook_pmf():
    """The five expressions of the contract against SciPy's nbinom.logpmf and its central differences at moderate arguments.  logpmf
    carries ~1e-12 absolute: first differences at h = 1e-4 are good to 1e-8 (rounding) + 1e-7 (truncation), second differences at
    h = 1e-3 to 1e-6 + 1e-5; the bounds are ten times that."""
    from scipy import stats
    rng = np.random.RandomState(3)
    y = rng.randint(0, 60, 200).astype(float)
    f0, f1 = rng.uniform(-2.0, 3.5, 200), rng.uniform(-2.0, 4.0, 200)
    lp, d0, h0, d1, h1 = nr.logpdf_and_derivatives(y, f0, f1)
    ref = lambda a, b: stats.nbinom.logpmf(y, np.exp(b), np.exp(b) / (np.exp(b) + np.exp(a)))
    assert np.allclose(lp, ref(f0, f1), rtol=1e-11, atol=1e-11)
    h, k = 1e-4, 1e-3
    for got, num, tol in ((d0, (ref(f0 + h, f1) - ref(f0 - h, f1)) / (2 * h), 1e-6), (d1, (ref(f0, f1 + h) - ref(f0, f1 - h)) / (2 * h), 1e-6),
                          (h0, (ref(f0 + k, f1) - 2 * ref(f0, f1) + ref(f0 - k, f1)) / k ** 2, 1e-4),
                          (h1, (ref(f0, f1 + k) - 2 * ref(f0, f1) + ref(f0, f1 - k)) / k ** 2, 1e-4)):
        assert np.max(np.abs(got - num) / (1.0 + np.abs(got))) < tol


def test_derivatives_are_those_of_ve():
    """dm, dv of the 20-node rule against central differences, in m and in v, of a FINER rule's ve (T = 32 per dimension): the two
    agree as far as the 20-node rule has converged, 5e-11 for v <= 0.5, and as far as the differences go: h = 1e-4 leaves a
    truncation of h^2 / 6 times the third derivative, 1e-8 relative to values of order one, and a rounding of 1e-11.  The bound is ten
    times the truncation, 1e-7 (measured: 2.3e-9); a wrong factor in any derivative is an error of order one."""
    rng = np.random.RandomState(12)
    N = 40
    m = rng.uniform(-2.0, 3.0, (N, 2))
    v = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, 2)))
    y = nr.draw(rng, m[:, 0], m[:, 1])
    _, dm, dv = nr.var_exp(y, m, v)
    h = 1e-4
    fine = lambda mm, vv: nr.var_exp(y, mm, vv, T=32)[0]
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


def test_predictive_closed_form_against_quadrature_of_the_conditional_moments():
    """mean = E[mu], variance = E[mu + mu^2 / r] + Var[mu] under q(f0) q(f1), by 120-node Gauss-Hermite rules, to 1e-10 relative."""
    rng = np.random.RandomState(8)
    N = 200
    m = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N)], 1)
    v = np.exp(rng.uniform(np.log(1e-3), np.log(2.0), (N, 2)))
    x, w = nr.gh(120)
    f0 = x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1]
    f1 = x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:]
    e1, e2, ir = np.exp(f0) @ w, np.exp(2.0 * f0) @ w, np.exp(-f1) @ w
    mean, var = nr.predictive(m, v)
    assert mean.shape == (N, 1) and var.shape == (N, 1)
    assert np.max(np.abs(mean[:, 0] - e1) / e1) <= 1e-10
    want = e1 + e2 * ir + (e2 - e1 * e1)
    assert np.max(np.abs(var[:, 0] - want) / want) <= 1e-10
    mean, var = nr.predictive(m, np.zeros_like(v))                                         # v = 0: the moments at f = m
    mu, vr = nr.moments(m[:, 0], m[:, 1])
    assert np.allclose(mean[:, 0], mu, rtol=1e-14) and np.allclose(var[:, 0], vr, rtol=1e-14)


def test_poisson_limit():
    """m1 = 18, v1 = 1e-6 (r = 6.6e7): ve, dm_0, dv_0 are the Poisson oracle's up to (mu^2 + y^2) / r.  log p differs from Poisson's by
    ((y - mu)^2 - y) / (2 r) + O(r^-2), its f0-derivatives by mu (mu - y) / r and (2 mu^2 - y mu) / r: each below (mu^2 + y^2) / r, evaluated per
    row with E_q[mu^2] = exp(2 m0 + 2 v0) and the smallest r of the row's nodes."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(5)
    N = 300
    m0, v0 = rng.uniform(-2.0, 3.0, N), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), N))
    y = rng.poisson(np.exp(m0)).astype(float)
    m, v = np.stack([m0, np.full(N, 18.0)], 1), np.stack([v0, np.full(N, 1e-6)], 1)
    ve, dm, dv = nr.var_exp(y, m, v)
    pve, pdm, pdv = lo.poisson(y, m0, v0)
    r_min = np.exp(18.0 - nr.gh()[0].max() * np.sqrt(2e-6))
    bound = (np.exp(2.0 * m0 + 2.0 * v0) + y * y) / r_min
    for name, a, b in (("ve", ve, pve), ("dm_0", dm[:, 0], pdm[:, 0]), ("dv_0", dv[:, 0], pdv[:, 0])):
        d = np.abs(a - b)
        print("Poisson limit, %-4s: worst |NB - Poisson| / bound = %.3g" % (name, np.max(d / (bound * 1.001 + 1e-13 * (1.0 + np.abs(b))))))
        assert np.all(d <= bound * 1.001 + 1e-13 * (1.0 + np.abs(b))), name
    assert np.max(np.abs(ve - pve)) > 1e-12                                                # ... and the two are not the same function


def test_outputs_are_finite_at_the_corners():
    for y in (0.0, 1.0, 33.0, 1e6):
        for m0 in (750.0, -750.0, 0.0):
            for m1 in (750.0, -750.0, 21.0, -21.0, 0.0):
                for v0 in (0.0, 1e4):
                    out = likgrid.pack(*nr.var_exp(np.array([y]), np.array([[m0, m1]]), np.array([[v0, v0]])), 1)
                    assert np.all(np.isfinite(out)), (y, m0, m1, v0)
