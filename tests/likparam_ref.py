"""Derivatives of the variational expectation with respect to the likelihoods' own parameters, twice:

  * a float64 NumPy / SciPy restatement of the three per-row rules (Gaussian closed form, Student 20 x 20, Ordinal GH20), written
    from the contract's formulas with the kernels' branch structure;
  * a high-precision (mpmath) evaluation of the SAME finite rules, the rule's closed form differentiated term by term, with the
    conventions of tests/lik_ref_mp.py and tests/ordinal_ref_mp.py: the float64 inputs and Gauss-Hermite tables are exact numbers,
    every output element comes as R (the value) and S (sum over nodes of weight times the absolute values of the addends).

Addends.  Gaussian d/dsigma: -1/sigma, (y-m)^2/sigma^3, v/sigma^3.  Student d/dnu: psi((nu+1)/2)/2, -psi(nu/2)/2, -1/(2 nu), and
per node -log1p(u)/2, (nu+1)/(2 nu) u/(1+u).  Ordinal, per node: d/dlo: -phi(a)/(sigma P); d/dhi: phi(b)/(sigma P);
d/dsigma: a phi(a)/(sigma P), -b phi(b)/(sigma P) (terms with an infinite a or b are 0).

The grid of the tests (bulk and edge rows of each family) is built here once per process and shared."""
import functools

import mpmath
import numpy as np
from scipy import special

import likgrid
import ordinal_ref_mp as omp

mp, mpf = mpmath.mp, mpmath.mpf
WORK_DPS = 120
EPS = 2.0 ** -52
BULK, EDGE = 0, 1
INF = float("inf")
_X20, _W20 = np.polynomial.hermite.hermgauss(20)
_WN20 = _W20 / np.sqrt(np.pi)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def gaussian_dsigma(y, m, v, sigma=0.5):
    y, m, v = (np.asarray(a, float).reshape(-1) for a in (y, m, v))
    r = y - m
    return (-1.0 / sigma + (r * r + v) / (sigma * sigma * sigma))[:, None]


def student_dlogc(nu):
    """C'(nu); from nu = 64 on the derivative of the asymptotic series of C in x = nu / 2."""
    if nu < 64.0:
        return 0.5 * special.digamma(0.5 * (nu + 1.0)) - 0.5 * special.digamma(0.5 * nu) - 0.5 / nu
    ix = 2.0 / nu
    z = ix * ix
    return 0.5 * z * (1.0 / 8.0 + z * (-1.0 / 64.0 + z * (1.0 / 128.0 + z * (-17.0 / 2048.0 + z * (31.0 / 2048.0 + z * (-691.0 / 16384.0))))))


def student_dnu(y, m, v, deg_free=5.0):
    y = np.asarray(y, float).reshape(-1)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    nu = float(deg_free)
    r = y[:, None] - (_X20[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])                    # [N, 20]
    s = np.exp(np.minimum(-(_X20[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:]), 709.782712893384))
    u = r[:, :, None] ** 2 * s[:, None, :] / nu
    w = _WN20[:, None] * _WN20[None, :]
    node = 0.5 * (nu + 1.0) / nu * (u / (1.0 + u)) - 0.5 * np.log1p(u)
    return (student_dlogc(nu) + np.sum(w[None] * node, (1, 2)))[:, None]


def _ordinal_node(a, b):
    """(phi(a) / P, phi(b) / P, h) with the three branches of the kernel; a < b arrays, either may be infinite."""
    mir = a + b > 0.0
    a, b = np.where(mir, -b, a), np.where(mir, -a, b)
    with np.errstate(all="ignore"):
        Q = 0.5 * (special.erfc(-a * np.sqrt(0.5)) + special.erfc(b * np.sqrt(0.5)))
        direct = (b > 0.0) & (Q < 0.5)
        pa, pb = np.exp(-0.5 * a * a) / np.sqrt(2.0 * np.pi), np.exp(-0.5 * b * b) / np.sqrt(2.0 * np.pi)
        rP = 1.0 / (1.0 - Q)
        apa = np.where(np.isinf(a), 0.0, a * pa)
        bpb = np.where(np.isinf(b), 0.0, b * pb)
        ra1, rb1, h1 = pa * rP, pb * rP, (apa - bpb) * rP
        Ea, Eb = special.erfcx(-a * np.sqrt(0.5)), special.erfcx(-b * np.sqrt(0.5))
        x = 0.5 * (b - a) * (a + b)
        em, ed = np.expm1(x), np.exp(x)
        D = (Eb - Ea) - em * Ea
        rD = np.sqrt(2.0 / np.pi) / D
        ra2, rb2 = ed * rD, rD
        h2 = (np.where(np.isinf(a), 0.0, a * ed) - b) * rD
    ra, rb, h = np.where(direct, ra1, ra2), np.where(direct, rb1, rb2), np.where(direct, h1, h2)
    return np.where(mir, rb, ra), np.where(mir, ra, rb), h


def ordinal_edges(K=None, bin_edges=None):
    if bin_edges is None:
        return np.arange(1, int(K), dtype=float) - 0.5 * int(K)
    return np.asarray(bin_edges, float).reshape(-1)


def ordinal_cuts(y, edges):
    ext = np.concatenate([[-INF], edges, [INF]])
    k = np.asarray(y, float).reshape(-1).astype(int)
    return ext[k - 1], ext[k]


def ordinal_dparam(y, m, v, K=None, bin_edges=None, sigma=1.0):
    """[N, 3]: d ve / d lo, d hi, d sigma of the row's own two cut points."""
    lo, hi = ordinal_cuts(y, ordinal_edges(K, bin_edges))
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    f = _X20[None, :] * np.sqrt(2.0 * v)[:, None] + m[:, None]
    qa, qb, h = _ordinal_node((lo[:, None] - f) / sigma, (hi[:, None] - f) / sigma)
    return np.stack([-(qa @ _WN20) / sigma, (qb @ _WN20) / sigma, (h @ _WN20) / sigma], 1)


def dparam(name, y, m, v, **kw):
    return dict(Gaussian=gaussian_dsigma, Student=student_dnu, Ordinal=ordinal_dparam)[name](y, m, v, **kw)


def dparam_scale(name, y, m, v, **kw):
    """float64 condition scale S of dparam's elements (sum of the absolute values of the addends), for rows that have no
    high-precision twin."""
    if name == "Gaussian":
        y, m, v = (np.asarray(a, float).reshape(-1) for a in (y, m, v))
        s = kw.get("sigma", 0.5)
        return (1.0 / s + ((y - m) ** 2 + v) / s ** 3)[:, None]
    if name == "Student":
        y = np.asarray(y, float).reshape(-1)
        m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
        nu = float(kw.get("deg_free", 5.0))
        r = y[:, None] - (_X20[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])
        s = np.exp(np.minimum(-(_X20[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:]), 709.782712893384))
        u = r[:, :, None] ** 2 * s[:, None, :] / nu
        w = _WN20[:, None] * _WN20[None, :]
        c = 0.5 * abs(special.digamma(0.5 * (nu + 1.0))) + 0.5 * abs(special.digamma(0.5 * nu)) + 0.5 / nu
        return (c + np.sum(w[None] * (0.5 * (nu + 1.0) / nu * (u / (1.0 + u)) + 0.5 * np.log1p(u)), (1, 2)))[:, None]
    sigma = kw.get("sigma", 1.0)
    lo, hi = ordinal_cuts(y, ordinal_edges(kw.get("K"), kw.get("bin_edges")))
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    f = _X20[None, :] * np.sqrt(2.0 * v)[:, None] + m[:, None]
    a, b = (lo[:, None] - f) / sigma, (hi[:, None] - f) / sigma
    qa, qb, _ = _ordinal_node(a, b)
    with np.errstate(invalid="ignore"):
        ta, tb = np.where(np.isinf(a), 0.0, np.abs(a) * qa), np.where(np.isinf(b), 0.0, np.abs(b) * qb)
    return np.stack([(qa @ _WN20) / sigma, (qb @ _WN20) / sigma, ((ta + tb) @ _WN20) / sigma], 1)


def ordinal_bin_gradient(y, d, K):
    """Per-row (d lo, d hi, d sigma) [N, 3] -> gradient with respect to (b_1 .. b_{K-1}, sigma): label k adds d hi to cut k, d lo to cut k - 1."""
    k = np.asarray(y, float).reshape(-1).astype(int)
    g = np.zeros(K)
    for c in range(1, K):
        g[c - 1] = d[k == c, 1].sum() + d[k == c + 1, 0].sum()
    g[K - 1] = d[:, 2].sum()
    return g


# ---------------------------------------------------------------------------------------------------- high precision
def _acc(terms):
    return float(sum(terms)), float(sum(abs(t) for t in terms))


def gaussian_row_mp(y, m, v, sigma):
    with mp.workdps(WORK_DPS):
        y, m, v, s = (mpf(float(a)) for a in (y, m, v, sigma))
        R, S = _acc([-1 / s, (y - m) ** 2 / s ** 3, v / s ** 3])
        return np.array([R]), np.array([S])


def student_dlogc_mp(nu):
    nu = mpf(float(nu))
    return [mpmath.digamma((nu + 1) / 2) / 2, -mpmath.digamma(nu / 2) / 2, -1 / (2 * nu)]


def student_row_mp(y, m, v, nu):
    with mp.workdps(60):                               # (400 nodes; no cancellation beyond the addends themselves)
        x, w = omp.gh20()
        y, nu = mpf(float(y)), mpf(float(nu))
        r = [y - (xi * mpmath.sqrt(2 * mpf(float(v[0]))) + mpf(float(m[0]))) for xi in x]
        lim = mpf(709.782712893384)
        s = [mpmath.exp(min(-(xi * mpmath.sqrt(2 * mpf(float(v[1]))) + mpf(float(m[1]))), lim)) for xi in x]
        terms = student_dlogc_mp(nu)
        kn = (nu + 1) / (2 * nu)
        for i in range(20):
            for j in range(20):
                u = r[i] * r[i] * s[j] / nu
                ww = w[i] * w[j]
                terms.append(-ww * mpmath.log1p(u) / 2)
                terms.append(ww * kn * u / (1 + u))
        R, S = _acc(terms)
        return np.array([R]), np.array([S])


def ordinal_row_mp(lo, hi, sigma, m, v):
    with mp.workdps(WORK_DPS):
        x, w = omp.gh20()
        sg, mm, sv = mpf(float(sigma)), mpf(float(m)), mpmath.sqrt(2 * mpf(float(v)))
        tl, th, ts = [], [], []
        for xi, wi in zip(x, w):
            f = mm + sv * xi
            a = -mpmath.inf if lo == -INF else (mpf(float(lo)) - f) / sg
            b = mpmath.inf if hi == INF else (mpf(float(hi)) - f) / sg
            _, P = omp.prob_terms(a, b)
            pa, pb = omp._phi(a), omp._phi(b)
            tl.append(-wi * pa / (sg * P))
            th.append(wi * pb / (sg * P))
            ts.append(wi * (mpf(0) if mpmath.isinf(a) else a * pa) / (sg * P))
            ts.append(-wi * (mpf(0) if mpmath.isinf(b) else b * pb) / (sg * P))
        out = [_acc(tl), _acc(th), _acc(ts)]
        return np.array([o[0] for o in out]), np.array([o[1] for o in out])


# ---------------------------------------------------------------------------------------------------- the grid
def _ordinal_edges_for(K, sigma, rng, width=None):
    w = sigma * (rng.uniform(0.25, 4.0, K - 1) if width is None else np.full(K - 1, width))
    e = np.cumsum(w)
    return e - 0.5 * (e[0] + e[-1])


def _rows():
    """[(name, kw, cls, y, m [J], v [J])]: a bulk class as in the var_exp grids (m in [-3, 3], v in [1e-3, 4], bins of 0.25 .. 4 sigma) and
    an edge class: bins down to 1e-3 sigma, |m| up to 40 sigma, end bins, nu in {0.7, 2.5, 5, 30, 64, 1e3, 1e6}; K in {2, 3, 5, 11, 32}."""
    rng = np.random.RandomState(20261018)
    rows = []
    for sigma in (0.2, 0.5, 1.0, 3.0):
        for _ in range(6):
            m, v = rng.uniform(-3, 3), 10.0 ** rng.uniform(-3, np.log10(4.0))
            rows.append(("Gaussian", dict(sigma=sigma), BULK, m + sigma * rng.randn(), [m], [v]))
    for sigma, r, v in ((1e-3, 40.0, 0.0), (1e-3, 1e-6, 1e-8), (1e3, 40.0, 1e4), (1e3, 0.0, 0.0), (0.5, 40.0, 1e-12), (2.0, 1.0, 3.0)):
        rows.append(("Gaussian", dict(sigma=sigma), EDGE, 1.5 + r * sigma, [1.5], [v]))
    for nu in (3.0, 5.0, 10.0):
        for _ in range(6):
            m, v = rng.uniform(-3, 3, 2), 10.0 ** rng.uniform(-3, np.log10(4.0), 2)
            rows.append(("Student", dict(deg_free=nu), BULK, m[0] + np.exp(0.5 * m[1]) * rng.standard_t(nu), list(m), list(v)))
    for nu in (0.7, 2.5, 5.0, 30.0, 64.0, 1e3, 1e6):
        for m0, m1, v0, v1, res in ((0.0, 0.0, 1.0, 1.0, 0.5), (40.0, -6.0, 1e-3, 0.0, 1e-6), (-2.0, 5.0, 4.0, 4.0, 40.0), (1.0, -12.0, 0.0, 1e-3, 3.0)):
            rows.append(("Student", dict(deg_free=nu), EDGE, m0 + res, [m0, m1], [v0, v1]))
    for K in (2, 3, 5, 11, 32):
        for sigma in (0.5, 2.0):
            e = _ordinal_edges_for(K, sigma, rng)
            labels = range(1, K + 1) if K <= 5 else (1, 2, K // 2, K - 1, K)
            for y in labels:
                m, v = rng.uniform(-3, 3), 10.0 ** rng.uniform(-3, np.log10(4.0))
                rows.append(("Ordinal", dict(bin_edges=list(e), sigma=sigma), BULK, float(y), [m], [v]))
    for K in (2, 3, 5, 11, 32):
        sigma = {2: 1.0, 3: 1e-3, 5: 1.0, 11: 1e3, 32: 0.5}[K]
        for width in (1e-3, 1e-2, 1.0):
            e = _ordinal_edges_for(K, sigma, rng, width)
            kw = dict(bin_edges=list(e), sigma=sigma)
            for y, mr, v in ((1, 40.0, 1e-6), (K, -40.0, 1.0), (1, -40.0, 0.0), (K, 40.0, 1e2), ((K + 1) // 2, 0.3, 1e-6),
                             ((K + 1) // 2, 10.0, 1.0), (min(2, K), -40.0, 1e2), (max(K - 1, 1), 3.0, 0.0)):
                rows.append(("Ordinal", kw, EDGE, float(y), [mr * sigma], [v * sigma * sigma]))
    return rows


@functools.lru_cache(maxsize=None)
def grid():
    """dict name -> dict(groups=[(kw, idx)], y, m, v, cls, R, S) with R, S [n, C] from the high-precision rules."""
    out = {}
    for name in ("Gaussian", "Student", "Ordinal"):
        rs = [r for r in _rows() if r[0] == name]
        R, S = [], []
        for _, kw, _, y, m, v in rs:
            if name == "Gaussian":
                a = gaussian_row_mp(y, m[0], v[0], kw["sigma"])
            elif name == "Student":
                a = student_row_mp(y, m, v, kw["deg_free"])
            else:
                lo, hi = ordinal_cuts([y], np.asarray(kw["bin_edges"]))
                a = ordinal_row_mp(float(lo[0]), float(hi[0]), kw["sigma"], m[0], v[0])
            R.append(a[0]), S.append(a[1])
        groups = {}
        for i, r in enumerate(rs):
            groups.setdefault(repr(sorted(r[1].items())), (r[1], []))[1].append(i)
        out[name] = dict(groups=[(kw, np.array(idx)) for kw, idx in groups.values()], y=np.array([r[3] for r in rs]),
                         m=np.array([r[4] for r in rs]), v=np.array([r[5] for r in rs]), cls=np.array([r[2] for r in rs]),
                         R=np.array(R), S=np.array(S))
    return out


def evaluate(g, fn, name):
    """fn(name, y, m, v, **kw) -> [n, C] over the rows of one family's grid."""
    out = np.empty(g["R"].shape)
    for kw, idx in g["groups"]:
        out[idx] = fn(name, g["y"][idx], g["m"][idx], g["v"][idx], **kw)
    return out


def ratios(got, g):
    """The project's criterion (tests/likgrid.py: ratios): |got - R| / (2^-52 max(S, 2^-1022)) per element, 0 where got == R."""
    return likgrid.ratios(got, g["R"], g["S"], np.zeros(g["R"].shape, np.uint8))


def worst_ratios(got, g):
    """{class: [C] largest ratio}."""
    r = ratios(got, g)
    return {c: r[g["cls"] == c].max(0) for c in (BULK, EDGE)}
