"""CPU: the right-censored Weibull likelihood of DESIGN 9i at the layers that need no device -- the C enum, the ctypes ids, the
descriptor, the synthetic generator -- and the yardstick itself: the float64 restatement tests/weibull_ref.py against the
high-precision one (tests/weibull_ref_mp.py) on the committed grid tests/golden/wbgrid.npz, under the criterion of tests/likgrid.py,
|got - R| <= C 2^-52 S  per element.

C_ORACLE: the largest |weibull_ref - R| / (2^-52 S) over the committed grid, no element left out, per row class and output kind
(ve, dm, dv), rounded up to the next power of two.  Measured 2026-10-19 (NumPy / SciPy on the CPU), raw figures:
    bulk   2156 / 2161 / 2166          edge   4420 / 95075 / 95073
Both are the rounding of z = k (ly - f0) amplified by |z| in e = exp(z), which is NOT folded into S (DESIGN 9a's rule): a bulk row may
carry nodes with z of several hundred, short of the clip at 680, where W e dominates every sum (the worst bulk row, 223, has z = 445
and k = 157 at its corner node, which carries the sums); the edge figure is dm_1 / dv_1 of the row with ly - f0 of 1e-6 (row 338: z next to 0, the addends -e z cancel over the
nodes of f0 while ly - f0 carries the rounding of ly = 1 - 1.1e-16).  No element of the grid is non-finite and none is excepted.

Corruption check (test_power_before_logarithm_is_seen_by_the_grid): z formed as log((y / lambda)^k) leaves C_KERNEL on the edge rows
with y = 1e-300 / 1e300 or |m0| = 700 (the quotient or the power overflows or vanishes: non-finite outputs) and on the rows with z
next to 0 (the power rounds next to 1: the digits of z are lost)."""
import importlib.util
import os
import re

import numpy as np
import pytest

import likgrid
import weibull_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
GRID = os.path.join(ROOT, "tests", "golden", "wbgrid.npz")
BULK, EDGE = likgrid.BULK, likgrid.EDGE
KIND = np.array([0, 1, 1, 2, 2])

C_ORACLE = {BULK: (4096.0, 4096.0, 4096.0), EDGE: (8192.0, 131072.0, 131072.0)}


def c_kernel():
    """The kernel's constants: max(16, 4 C_ORACLE), the rule of DESIGN 9a (wave-shuffle summation order, 1-2 ulp device functions)."""
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE.items()}


def c_kernel_vs_float64():
    """Kernel against the float64 restatement instead of R: each sits within its own constant of the true value, so the two add."""
    k = c_kernel()
    return {c: tuple(a + b for a, b in zip(k[c], C_ORACLE[c])) for c in k}


@pytest.fixture(scope="module")
def grid():
    """The committed grid, loaded once for the module; nobody writes to it."""
    g = dict(np.load(GRID))
    for a in g.values():
        a.setflags(write=False)
    return g


def load_grid():
    return dict(np.load(GRID))


def assert_grid(g, got, C, what, rows=None):
    idx = np.arange(len(g["y"])) if rows is None else rows
    return likgrid.assert_rows(got, g["R"][idx], g["S"][idx], np.zeros(got.shape, np.uint8), KIND, g["cls"][idx], C, what)


def bulk_rows(rng, N):
    """Seeded bulk rows: m in [-1.5, 1.5]^2, v log-uniform in [1e-3, 0.5]^2, y from the row's own Weibull, every second row
    censored, and only rows in which no node reaches the clip of z (the others are drawn again)."""
    Y, m, v = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 2))
    while len(Y) < N:
        mm = rng.uniform(-1.5, 1.5, (N, 2))
        vv = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, 2)))
        yy = wr.draw(rng, mm[:, 0], mm[:, 1], censored=0.0)
        yy[:, 1] = np.arange(N) % 2
        ok = (yy[:, 0] > 0.0) & (wr.clipped_nodes(yy, mm, vv) == 0)
        Y, m, v = np.vstack([Y, yy[ok]]), np.vstack([m, mm[ok]]), np.vstack([v, vv[ok]])
    return Y[:N], m[:N], v[:N]


# ---------------------------------------------------------------------------------------------------- ids, descriptor
def test_header_python_and_engine_ids_agree():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_WEIBULL\s*=\s*12\b", src)
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump
    from hetmogp_amd import _lib, engine, synthetic
    assert _lib.LIK_WEIBULL == 12 and _lib.LIK_IDS_BY_NAME["Weibull"] == 12 and engine.LIK_IDS["Weibull"] == 12
    assert engine.lik_dim_f("Weibull") == 2 and engine.lik_dim_y("Weibull") == 2 and engine.lik_param("Weibull") == 0.0
    assert synthetic._dim_f("Weibull", {}) == 2
    y = engine._y_rows("Weibull", [[1.0, 1.0], [2.0, 0.0], [3.0, 1.0]])
    assert y.shape == (3, 2) and y.flags.c_contiguous
    for bad in (np.ones(4), np.ones((4, 1)), np.ones((4, 3))):                     # never reshaped into pairs
        with pytest.raises(_lib.InvalidArgument) as ei:
            engine._y_rows("Weibull", bad)
        assert "Weibull" in str(ei.value)


def test_descriptor_metadata_and_specs():
    from hetmogp_amd import HetLikelihood, Gaussian, Weibull, Categorical
    d = Weibull()
    assert d.get_metadata() == (2, 2, 1) and d.ismulti() is False and d.kwargs() == {} and d.name == "Weibull"
    assert Weibull(gp_link=None).learnable_params() == []
    h = HetLikelihood([Gaussian(), Weibull(), Categorical(K=3)])
    md = h.generate_metadata()
    assert md["y_index"].tolist() == [0, 1, 1, 2] and md["function_index"].tolist() == [0, 1, 1, 2, 2]
    assert md["d_index"].tolist() == [0, 0, 1, 0, 1] and md["pred_index"].tolist() == [0, 1, 2, 2]
    assert h.specs()[1] == ("Weibull", {})


@pytest.mark.parametrize("share", [0.3, 0.6, 0.0])
def test_synthetic_rows_are_censored_at_the_stated_share(share):
    """The generator censors at an independent censoring time: the share of censored rows is Binomial(N, share), asserted within
    5 standard errors; a censored time lies below the event time the same seed gives without censoring."""
    from hetmogp_amd.synthetic import make_case, weibull_censored
    N = 4000
    prm, X, Y = make_case([("Gaussian", {"sigma": 0.5}), ("Weibull", {"censored": share})], [50, N], M=16, Q=2, seed=4)
    y = Y[1]
    assert y.shape == (N, 2) and np.all(np.isfinite(y)) and np.all(y[:, 0] > 0.0) and prm["W"].shape == (2, 3)
    assert np.all((y[:, 1] == 0.0) | (y[:, 1] == 1.0))
    got = 1.0 - y[:, 1].mean()
    assert abs(got - share) <= 5.0 * np.sqrt(max(share * (1.0 - share), 1e-12) / N), (got, share)
    f0, f1 = np.linspace(-1, 1, N), np.linspace(-0.5, 1, N)
    a = weibull_censored(np.random.RandomState(1), f0, f1, share)
    b = weibull_censored(np.random.RandomState(1), f0, f1, 0.0)
    assert np.all(b[:, 1] == 1.0) and np.all(a[:, 0] <= b[:, 0]) and np.all((a[:, 0] < b[:, 0]) == (a[:, 1] == 0.0))
    assert np.array_equal(a, wr.draw(np.random.RandomState(1), f0, f1, share))     # the tests' restatement draws the same rows


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_small_and_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "wbgrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    assert os.path.getsize(GRID) < likgrid.SIZE_BOUND


def test_fixture_regenerates_bit_identically(grid):
    spec = importlib.util.spec_from_file_location("make_weibull_grid", os.path.join(ROOT, "tools", "make_weibull_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new = mod.build()
    assert sorted(new) == sorted(grid)
    for k in grid:
        assert new[k].dtype == grid[k].dtype and new[k].tobytes() == grid[k].tobytes(), k


def test_reference_modules_are_independent():
    src = open(os.path.join(ROOT, "tests", "weibull_ref_mp.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(hetmogp_amd|weibull_ref\b)", src, re.M)


def test_grid_design(grid):
    g = grid
    Y, m, v, e = g["y"], g["m"], g["v"], g["cls"] == EDGE
    y, d = Y[:, 0], Y[:, 1]
    assert np.all(np.isfinite(g["R"])) and np.all(np.isfinite(g["S"])) and np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
    assert np.all(np.isfinite(y) & (y > 0) & ((d == 0) | (d == 1)))                          # what the library accepts
    b = ~e
    assert b.sum() >= 128 and np.all(np.abs(m[b]) <= 1.5) and np.all((v[b] >= 1e-3) & (v[b] <= 0.5))
    assert (d[b] == 0).sum() == (d[b] == 1).sum()                                            # both indicators, half each
    nclip = wr.clipped_nodes(Y, m, v)
    assert np.all(nclip[b] == 0)                                                             # no bulk row reaches the clip of z
    # every designed row with delta = 0 and with delta = 1
    key = lambda i: (y[i],) + tuple(m[i]) + tuple(v[i])
    assert sorted(key(i) for i in np.where(e & (d == 0))[0]) == sorted(key(i) for i in np.where(e & (d == 1))[0])
    assert np.any(e & (nclip > 0) & (nclip < 400)) and np.any(e & (nclip == 400))            # the clip at some, and at all, nodes
    assert {10.0, -10.0, 750.0, -750.0} <= set(m[e][:, 1].tolist())                          # k at both clips
    assert {1e-300, 1e300} <= set(y[e].tolist()) and {700.0, -700.0} <= set(m[e][:, 0].tolist())
    assert np.any(e & (v[:, 0] == 0) & (v[:, 1] > 0)) and np.any(e & (v[:, 0] > 0) & (v[:, 1] == 0)) and np.any(e & np.all(v == 0, 1))
    z0 = np.log(y) - m[:, 0]
    assert np.any(e & (z0 == 0.0) & (v[:, 0] == 0.0)) and np.any(e & (np.abs(z0) > 0) & (np.abs(z0) < 1e-8))   # z at and next to 0


def test_float64_restatement_against_high_precision_grid(grid):
    """Where C_ORACLE comes from; also: no non-finite element anywhere (the clips of k and z guarantee it), no exceptions list."""
    got = likgrid.pack(*wr.var_exp(grid["y"], grid["m"], grid["v"]), len(grid["y"]))
    assert np.all(np.isfinite(got)), np.argwhere(~np.isfinite(got))[:8]
    w = assert_grid(grid, got, C_ORACLE, "weibull_ref on wbgrid")
    for c in (BULK, EDGE):                                     # ... and each constant IS the next power of two above its figure
        for k in range(3):
            assert C_ORACLE[c][k] < 4.0 * max(w[c][k], 0.5), (c, k, w[c][k])


def test_float64_scale_matches_high_precision_scale(grid):
    """The float64 scale carries the float64 rounding of e: C_ORACLE 2^-52 relative at the worst (3e-11); a scale needs no more."""
    S = wr.var_exp_scale(grid["y"], grid["m"], grid["v"])
    assert np.allclose(S, grid["S"], rtol=1e-9, atol=1e-300)


def test_power_before_logarithm_is_seen_by_the_grid(grid):
    """Seeded corruption: z = log((y / lambda)^k), the power formed first.  The edge rows with an extreme time or scale, and those with
    z next to 0, then leave C_KERNEL (not merely C_ORACLE); the clean restatement stays inside on the same rows."""
    g = grid
    y, m, v = g["y"], g["m"], g["v"]
    z0 = np.log(y[:, 0]) - m[:, 0]
    extreme = (g["cls"] == EDGE) & ((y[:, 0] <= 1e-300) | (y[:, 0] >= 1e300) | (np.abs(m[:, 0]) == 700.0))
    near0 = (g["cls"] == EDGE) & (np.abs(z0) > 0) & (np.abs(z0) < 1e-8)
    # (extreme rows whose z is clipped at 680, or whose quotient is moderate, give the same result either way: at least the four
    #  with y = 1e-300 against lambda >= 1, where the quotient vanishes, must differ; next to 0 the two rows whose ly - f0 changes sign
    #  over the nodes of f0, so that the addends cancel and S is small, must -- beside an addend delta = 1 the loss stays inside C)
    for what, rows, least in (("extreme y or scale", np.where(extreme)[0], 4), ("z next to 0", np.where(near0)[0], 2)):
        assert len(rows) >= 4, what
        bound = np.array([[c_kernel()[c][k] for k in KIND] for c in g["cls"][rows]])
        nf = np.zeros((len(rows), 5), np.uint8)
        clean = likgrid.ratios(likgrid.pack(*wr.var_exp(y[rows], m[rows], v[rows]), len(rows)), g["R"][rows], g["S"][rows], nf)
        assert np.all(clean <= bound), what
        with np.errstate(all="ignore"):
            got = likgrid.pack(*wr.var_exp(y[rows], m[rows], v[rows], zform=wr.z_of_pow), len(rows))
        r = likgrid.ratios(got, g["R"][rows], g["S"][rows], nf)
        out = (r > bound).any(1)
        print("pow before log, %-18s: rows beyond C_KERNEL %d of %d, non-finite rows %d, worst finite excess %.3g" %
              (what, int(out.sum()), len(rows), int((~np.isfinite(got)).any(1).sum()),
               np.max(np.where(np.isfinite(r), r / bound, 0.0))))
        assert out.sum() >= least, (what, r.max(1))


# ---------------------------------------------------------------------------------------------------- properties of the model
def test_exponential_limit_against_the_oracle():
    """delta = 1, m1 = 0, v1 = 0 (k = 1 exactly): the row is Exponential's at (-m0, v0), whose link is f = -log scale: ve and dv_0
    agree, dm_0 has the opposite sign -- each within the sum of the two families' bulk oracle constants in units of 2^-52 S."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(5)
    N = 300
    m0, v0 = rng.uniform(-1.5, 1.5, N), np.exp(rng.uniform(np.log(1e-3), np.log(0.5), N))
    y = np.exp(m0) * rng.exponential(1.0, N)
    Y, m, v = np.stack([y, np.ones(N)], 1), np.stack([m0, np.zeros(N)], 1), np.stack([v0, np.zeros(N)], 1)
    ve, dm, dv = wr.var_exp(Y, m, v)
    eve, edm, edv = lo.var_exp_all("Exponential", y[:, None], -m0[:, None], v0[:, None])
    S = wr.var_exp_scale(Y, m, v)
    ce = likgrid.c_oracle("Exponential")[BULK]
    for name, a, b, s, c in (("ve", ve, np.ravel(eve), S[:, 0], C_ORACLE[BULK][0] + ce[0]),
                             ("dm_0", dm[:, 0], -np.ravel(edm), S[:, 1], C_ORACLE[BULK][1] + ce[1]),
                             ("dv_0", dv[:, 0], np.ravel(edv), S[:, 3], C_ORACLE[BULK][2] + ce[2])):
        r = np.abs(a - b) / (likgrid.EPS * s)
        print("Exponential limit, %-4s: worst |Weibull - Exponential| / (2^-52 S) = %.3g (bound %g)" % (name, r.max(), c))
        assert np.all(r <= c), name
    assert np.all(np.abs(dm[:, 0]) > 0)


@pytest.mark.parametrize("delta", [1.0, 0.0])
def test_derivative_formulas_against_central_differences(delta):
    """d/df and d2/df2 against central differences of log p and of the first derivatives, h = 1e-5: truncation h^2 / 6 times the next
    derivative but one (of order (1 + z^2) e k^2 <= 1e3 on these rows: 2e-8), rounding 2^-52 |.| / h = 2e-11 |.|; the bound is 1e-6
    relative to 1 + |value|, and a wrong sign or factor is an error of order one."""
    rng = np.random.RandomState(3)
    N = 400
    f0, f1 = rng.uniform(-1.0, 1.0, N), rng.uniform(-1.0, 1.0, N)
    y = wr.draw(rng, f0, f1, censored=0.0)[:, 0]
    lp, d0, h0, d1, h1 = wr.logpdf_and_derivatives(y, delta, f0, f1)
    h = 1e-5
    L = lambda a, b, k=0: wr.logpdf_and_derivatives(y, delta, a, b)[k]
    for name, got, num in (("d/df0", d0, (L(f0 + h, f1) - L(f0 - h, f1)) / (2 * h)), ("d/df1", d1, (L(f0, f1 + h) - L(f0, f1 - h)) / (2 * h)),
                           ("d2/df0", h0, (L(f0 + h, f1, 1) - L(f0 - h, f1, 1)) / (2 * h)),
                           ("d2/df1", h1, (L(f0, f1 + h, 3) - L(f0, f1 - h, 3)) / (2 * h))):
        err = np.max(np.abs(got - num) / (1.0 + np.abs(got)))
        print("delta = %g, %-6s: worst |formula - central difference| / (1 + |.|) = %.3g" % (delta, name, err))
        assert err <= 1e-6, name


def test_log_density_against_scipy():
    """delta = 1: weibull_min.logpdf; delta = 0: log(1 - CDF) = weibull_min.logsf, the survival function of a right-censored row."""
    from scipy import stats
    rng = np.random.RandomState(9)
    N = 300
    f0, f1 = rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N)
    y = wr.draw(rng, f0, f1, censored=0.0)[:, 0]
    dist = stats.weibull_min(np.exp(f1), scale=np.exp(f0))
    ev, ce = wr.logpdf_and_derivatives(y, 1.0, f0, f1)[0], wr.logpdf_and_derivatives(y, 0.0, f0, f1)[0]
    assert np.allclose(ev, dist.logpdf(y), rtol=1e-11, atol=1e-11)
    assert np.allclose(ce, dist.logsf(y), rtol=1e-11, atol=1e-300)
    inside = dist.cdf(y) < 1.0 - 1e-9
    assert np.allclose(ce[inside], np.log1p(-dist.cdf(y[inside])), rtol=1e-6, atol=1e-12)   # ... which IS log(1 - CDF)
    assert np.all(ce <= 0.0)


def test_predictive_against_a_200_node_rule():
    """Mean and variance of the event time: the 20-node rule over f1 against a 200-node one.  For v1 <= 0.02 and m1 >= 0 the nodes of
    the 20-node rule reach f1 >= -1.08, where Gamma(1 + p exp(-f1)) has a logarithmic derivative below c = 8 in f1 (p = 2: psi(6.9) 5.9);
    a Gauss-Hermite rule of n nodes integrates exp(a x) to (a^2 / 2)^n / n! relative, a = c sqrt(2 v1) <= 1.6: 1e-17 at n = 20.  The
    200-node rule's nodes reach f1 = -3.8, Gamma(94) = 1e144 under a weight of 1e-160.  Bound 1e-10.  (The EXACT expectation under a
    Gaussian q(f1) is dominated by k -> 0 and is astronomically large for any v1 > 0: `predictive` is the rule's value)"""
    rng = np.random.RandomState(8)
    N = 200
    m = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(0.0, 1.5, N)], 1)
    v = np.stack([np.exp(rng.uniform(np.log(1e-3), np.log(0.5), N)), np.exp(rng.uniform(np.log(1e-4), np.log(0.02), N))], 1)
    mean, var = wr.predictive(m, v)
    m2, v2 = wr.predictive(m, v, T=200)
    assert mean.shape == (N, 1) and var.shape == (N, 1) and np.all(mean > 0) and np.all(var > 0)
    assert np.max(np.abs(mean - m2) / m2) <= 1e-10
    e2, e2f = var + mean ** 2, v2 + m2 ** 2                     # (the second moment is what the rule forms; the variance a difference)
    assert np.max(np.abs(e2 - e2f) / e2f) <= 1e-10
    mean, var = wr.predictive(m, np.zeros_like(v))                                         # v = 0: the moments at f = m
    mu, vr = wr.moments(m[:, 0], m[:, 1])
    assert np.allclose(mean[:, 0], mu, rtol=1e-13) and np.allclose(var[:, 0], vr, rtol=1e-9)
    mean, var = wr.predictive(np.array([[800.0, 0.0], [0.0, -6.0]]), np.array([[1.0, 0.0], [0.1, 0.1]]))   # overflow is +inf
    assert np.all(np.isposinf(mean)) and np.all(np.isposinf(var))


def test_outputs_are_finite_at_the_corners():
    """y in {1e-300 .. 1e300}, m in {-700 .. 700}^2, v in {0, 1e-3, 4, 100} (both dimensions), both indicators: all five outputs finite."""
    ys, ms, vs = (1e-300, 1e-10, 1.0, 1e10, 1e300), (-700.0, -10.0, 0.0, 10.0, 700.0), (0.0, 1e-3, 4.0, 100.0)
    rows = [(y, d, m0, m1, v) for y in ys for d in (0.0, 1.0) for m0 in ms for m1 in ms for v in vs]
    a = np.array(rows)
    out = likgrid.pack(*wr.var_exp(a[:, :2], a[:, 2:4], a[:, 4:5].repeat(2, 1)), len(a))
    assert np.all(np.isfinite(out)), a[~np.isfinite(out).all(1)][:8]
