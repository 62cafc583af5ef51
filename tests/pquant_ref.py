"""float64 NumPy / SciPy restatement of the predictive cdf, survival function and quantiles of DESIGN 9k, and the loader / criteria of
its grid tests/golden/pqgrid.npz (tools/make_pquant_grid.py; 50-digit values from tests/pquant_ref_mp.py).

For a row with q(f) = N(m, diag v), over the nodes and normalised weights of DESIGN 9j (tests/logpred_ref.py: `gh`, `_tensor_nodes`)

    cdf(y) = sum_nodes w C(y | f_node),      sf(y) = sum_nodes w S(y | f_node)

with the conditional pair (C, S) evaluated directly, never as 1 - the other; links and clips as in logpred_ref._logpdf_terms:

  Gaussian      closed form: z = (y - m) / sqrt(sigma^2 + v);  C = erfc(-z / sqrt 2) / 2,  S = erfc(z / sqrt 2) / 2
  HetGaussian   T nodes over f1: z_j = (y - m0) / sqrt(v0 + safe_exp(f1_j)), the same pair
  Bernoulli     p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9): (0, 1) for y < 0, (1 - p, p) for 0 <= y < 1, (1, 0) for y >= 1
  Exponential   b = clip(safe_exp(-f), 1e-9, 1e9): (0, 1) for y <= 0, else S = exp(-y / b), C = -expm1(-y / b)
  Ordinal       closed form: y the label c in 1 .. K, z = (b_c - m) / sqrt(sigma^2 + v), b_K = +inf, Gaussian's pair
  Weibull       y a time: (0, 1) for y <= 0, else k = shape(f1), z = min(k (log y - f0), 680), e = exp(z): S = exp(-e), C = -expm1(-e)

Scale (defined once, here: `scale`): S = 1 + sum_i wbar_i A_i per output, wbar_i = w_i G_i / sum_j w_j G_j the share of node i in that
output (G = C for the cdf, S for the sf) and A_i the magnitude of the conditional exponent at the node: z^2 / 2 for the Phi families,
y / b for Exponential, e + |z| for Weibull, 0 for Bernoulli.

Criterion for cdf and sf against the 50-digit value R: |got - R| <= C 2^-52 S R; exact zeros, exact ones and non-finite values equal.
Quantiles (mixed forward / backward): with yhat moved 4 ulps down / up (4 ulps of log yhat in the log-variable families),
F(yhat-) - tol <= p <= F(yhat+) + tol, F this file's cdf, tol = (C_KERNEL + C_ORACLE) 2^-52 S p; for p > 1/2 the same on the survival
function: sf(yhat+) - tol <= 1 - p <= sf(yhat-) + tol, tol with 1 - p.  Bernoulli, Ordinal: the label equals this file's, except on rows
where some cumulative probability lies within tol of p (`discrete_ties`; the grid has none).

C_ORACLE[family][class] = (cdf, sf): the largest figure of THIS file against the grid, rounded up to the next power of two (measured
2026-10-19, CPU, NumPy / SciPy; `python tools/make_pquant_grid.py --measure` prints the raw figures).  The kernels get
C_KERNEL = max(16, 4 C_ORACLE), logpred_ref.c_kernel's rule.

`quantile` restates the kernels' solver step by step (one state machine between two evaluations of the rule, every loop bounded: at most
MAXEVAL evaluations per quantile) and can count its evaluations; `quantile_brentq` is the independent route (SciPy's bracketing solver
on this file's cdf / sf)."""
import json
import os
import sys

import numpy as np
from scipy import optimize, special

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import likgrid as lg               # noqa: E402
import logpred_ref as lr           # noqa: E402
import weibull_ref as wr           # noqa: E402
from oracle import lik_ordinal as lo     # noqa: E402

BULK, EDGE = lg.BULK, lg.EDGE
GRID = os.path.join(lg.GOLDEN, "pqgrid.npz")
FAMILIES = ("Gaussian", "HetGaussian", "Bernoulli", "Exponential", "Ordinal", "Weibull")
REFUSED = ("Poisson", "Gamma", "Beta", "Student", "NegBinomial", "Categorical", "Dirichlet")
DISCRETE = ("Bernoulli", "Ordinal")
LOGVAR = ("Exponential", "Weibull")
ZMAX = 680.0
EPS = 2.0 ** -52
MAXEVAL, MAXDBL, MAXNEWTON = 128, 64, 24

# family -> {class: (C_cdf, C_sf)}, measured 2026-10-19 (see the module docstring; the raw figures beside each line)
C_ORACLE = {
    "Gaussian": {BULK: (4, 1), EDGE: (1, 2)},            # raw 2.01 0.772 | 0.894 1.28
    "HetGaussian": {BULK: (2, 2), EDGE: (2, 4)},         # raw 1.3 1.09 | 1.65 2.52
    "Bernoulli": {BULK: (2, 2), EDGE: (1, 1)},           # raw 1.55 1.49 | 0.931 0.892
    "Exponential": {BULK: (2, 1), EDGE: (4, 1)},         # raw 1.27 0.612 | 2.71 0.588
    "Ordinal": {BULK: (1, 2), EDGE: (2, 2)},             # raw 0.887 1.66 | 1.51 1.27
    "Weibull": {BULK: (1, 8), EDGE: (2, 4)},             # raw 0.523 5.42 | 1.83 2.57     (|f| eps in exp(k (log y - f0)) on the sf side)
}


def c_oracle(family):
    return C_ORACLE[family]


def c_kernel(family):
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE[family].items()}


def c_sum(family):
    k, o = c_kernel(family), c_oracle(family)
    return {c: tuple(a + b for a, b in zip(k[c], o[c])) for c in k}


def dim_f(name, **kw):
    return lr.dim_f(name, **kw)


def sigma_of(name, **kw):
    if name == "Gaussian":
        s = kw.get("sigma")
        return 0.5 if s is None or not s > 0.0 else float(s)
    return float(kw.get("sigma", 1.0))


def edges_of(**kw):
    return np.asarray(lo.edges_of(kw.get("K"), kw.get("bin_edges")), float)


def _mv(name, m, v, **kw):
    J = dim_f(name, **kw)
    return np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)


# ------------------------------------------------------------------------------------------------------------ the rule
def _phi_pair(z):
    return 0.5 * special.erfc(-z * np.sqrt(0.5)), 0.5 * special.erfc(z * np.sqrt(0.5))


def node_terms(name, y, m, v, gh_T=0, **kw):
    """(C [N, S], S [N, S], A [N, S], W [S]): the conditional pair and the magnitude of the conditional exponent at the nodes."""
    T = int(gh_T) or 20
    m, v = _mv(name, m, v, **kw)
    y = np.asarray(y, float).reshape(-1)
    with np.errstate(all="ignore"):
        if name in ("Gaussian", "Ordinal"):
            sd = np.sqrt(sigma_of(name, **kw) ** 2 + v[:, 0])
            if name == "Ordinal":
                ext = np.concatenate([edges_of(**kw), [np.inf]])
                y = ext[y.astype(int) - 1]
            z = ((y - m[:, 0]) / sd)[:, None]
            C, S = _phi_pair(z)
            return C, S, np.where(np.isfinite(z), 0.5 * z * z, 0.0), np.ones(1)
        if name == "HetGaussian":
            x, w = lr.gh(T)
            sd = np.sqrt(v[:, 0:1] + lr._safe_exp(m[:, 1:2] + np.sqrt(2.0 * v[:, 1:2]) * x[None, :]))
            z = (y - m[:, 0])[:, None] / sd
            C, S = _phi_pair(z)
            return C, S, 0.5 * z * z, w
        F, W = lr._tensor_nodes(m, v, T)
        yy = y[:, None]
        if name == "Bernoulli":
            ef = lr._safe_exp(F[..., 0])
            p = np.clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9)
            C = np.where(yy < 0.0, 0.0, np.where(yy < 1.0, 1.0 - p, 1.0))
            S = np.where(yy < 0.0, 1.0, np.where(yy < 1.0, p, 0.0))
            nan = np.isnan(yy) & np.ones_like(p, bool)
            return np.where(nan, np.nan, C), np.where(nan, np.nan, S), np.zeros_like(p), W
        if name == "Exponential":
            b = lr._clip9(lr._safe_exp(-F[..., 0]))
            a = yy / b
            pos = yy > 0.0
            C = np.where(pos, -np.expm1(-a), np.where(yy <= 0.0, 0.0, np.nan))
            S = np.where(pos, np.exp(-a), np.where(yy <= 0.0, 1.0, np.nan))
            return C, S, np.where(pos, a, 0.0), W
        if name == "Weibull":
            ly = np.where(yy > 0.0, np.log(np.where(yy > 0.0, yy, 1.0)), np.where(yy <= 0.0, -np.inf, np.nan))
            return _weibull_pair(ly, F) + (W,)
    raise KeyError(name)


def _weibull_pair(ly, F):
    """ly [N, 1] = log of the time (-inf: a time <= 0), F [N, S, 2] -> (C, S, A)."""
    with np.errstate(all="ignore"):
        k = wr.shape(F[..., 1])
        z = np.minimum(k * (ly - F[..., 0]), ZMAX)
        e = np.exp(z)
        off = np.isneginf(ly) & np.ones_like(z, bool)
        C = np.where(off, 0.0, -np.expm1(-e))
        S = np.where(off, 1.0, np.exp(-e))
        return C, S, np.where(off, 0.0, e + np.abs(z))


def cdf_sf(name, y, m, v, gh_T=0, **kw):
    """(cdf [N], sf [N]) by the rule of DESIGN 9k."""
    C, S, A, W = node_terms(name, y, m, v, gh_T, **kw)
    return (C * W[None, :]).sum(1), (S * W[None, :]).sum(1)


def scale(name, y, m, v, gh_T=0, **kw):
    """S [N, 2] = 1 + sum_i wbar_i A_i for the cdf and for the sf (float64: a scale needs no more)."""
    C, S, A, W = node_terms(name, y, m, v, gh_T, **kw)
    out = []
    with np.errstate(all="ignore"):
        for G in (C, S):
            e = G * W[None, :]
            tot = e.sum(1, keepdims=True)
            wbar = np.where(tot > 0.0, e / np.where(tot > 0.0, tot, 1.0), 0.0)
            out.append(1.0 + np.nansum(np.where(wbar > 0.0, wbar * A, 0.0), 1))
    return np.stack(out, 1)


# ------------------------------------------------------------------------------------------------------------ quantiles
def _ord(x):
    b = np.float64(x).view(np.int64)
    return int(b) if b >= 0 else -int(b & np.int64(0x7FFFFFFFFFFFFFFF))


def _unord(k):
    return float(np.int64(k).view(np.float64)) if k >= 0 else -float(np.int64(-k).view(np.float64))


def ulps(x, n):
    """x moved by n units in the last place (through zero by the ordered bit pattern)."""
    x = np.asarray(x, float)
    return np.array([_unord(_ord(t) + n) if np.isfinite(t) else t for t in x.ravel()]).reshape(x.shape)


def _z_guess(q):
    t = np.sqrt(-2.0 * np.log(q))
    return t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308)))


def _loglog(q, use_sf):
    return np.log(-np.log(q)) if use_sf else np.log(-np.log1p(-q))


class _Row:
    """The solver's view of one row: x -> (cdf, sf, density in x), x = y or log y."""

    def __init__(self, name, m, v, T, **kw):
        self.name = name
        x, w = lr.gh(T)
        with np.errstate(all="ignore"):
            if name == "Gaussian":
                self.s = np.sqrt(sigma_of(name, **kw) ** 2 + v[0])
                self.m0, self.sd, self.w = m[0], np.array([self.s]), np.ones(1)
                self.d0 = self.s
            elif name == "HetGaussian":
                self.m0, self.w = m[0], w
                self.sd = np.sqrt(v[0] + lr._safe_exp(x * np.sqrt(2.0 * v[1]) + m[1]))
                self.s = self.d0 = np.sqrt(v[0] + lr._safe_exp(m[1] + 0.5 * v[1]))
            elif name == "Exponential":
                self.b, self.w = lr._clip9(lr._safe_exp(-(x * np.sqrt(2.0 * v[0]) + m[0]))), w
                self.m0, self.d0 = m[0], 1.0 + np.sqrt(2.0 * v[0])
            else:
                F, self.w = lr._tensor_nodes(m[None, :], v[None, :], T)
                self.f0, self.k = F[0, :, 0], wr.shape(F[0, :, 1])
                self.m0, self.rk = m[0], 1.0 / wr.shape(m[1])
                self.d0 = 1.0 + self.rk + np.sqrt(2.0 * v[0])

    def guess(self, tq, use_sf):
        with np.errstate(all="ignore"):
            if self.name in ("Gaussian", "HetGaussian"):
                return self.m0 + _z_guess(tq) * self.s if use_sf else self.m0 - _z_guess(tq) * self.s
            if self.name == "Exponential":
                return float(np.clip(-self.m0, -20.72326583694641, 20.72326583694641)) + _loglog(tq, use_sf)
            return self.m0 + _loglog(tq, use_sf) * self.rk

    def eval(self, x):
        with np.errstate(all="ignore"):
            if self.name in ("Gaussian", "HetGaussian"):
                z = (x - self.m0) / self.sd
                C, S = _phi_pair(z)
                D = np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi) / self.sd
            elif self.name == "Exponential":
                a = np.exp(x) / self.b
                C, S = -np.expm1(-a), np.exp(-a)
                D = a * S
            else:
                e = np.exp(np.minimum(self.k * (x - self.f0), ZMAX))
                C, S = -np.expm1(-e), np.exp(-e)
                D = self.k * e * S
            return float((self.w * C).sum()), float((self.w * S).sum()), float((self.w * D).sum())


def _solve(row, p):
    """One quantile by the kernels' state machine -> (x, evaluations)."""
    use_sf = p > 0.5
    tq = 1.0 - p if use_sf else p
    x = row.guess(tq, use_sf)
    lo = hi = x
    d, have, ndbl, nnewton = row.d0, 0, 0, 0
    with np.errstate(all="ignore"):
        for ev in range(MAXEVAL):
            C, S, D = row.eval(x)
            G = S if use_sf else C
            if not G == G:
                return np.nan, ev + 1
            if abs(G - tq) <= 8.9e-16 * tq:
                return x, ev + 1
            right = G > tq if use_sf else G < tq
            if right:
                lo, have = x, have | 1
            else:
                hi, have = x, have | 2
            dx = np.float64(G) * np.log(np.float64(G) / tq) / np.float64(D)
            xn = x + dx if use_sf else x - dx
            if abs(xn - x) <= 2.3e-16 * abs(x):
                return x, ev + 1
            if have != 3:
                if ndbl >= MAXDBL:
                    return np.nan, ev + 1
                ndbl += 1
                stp = 2.0 * abs(xn - x)
                if not stp <= d:
                    stp = d
                stp = max(stp, abs(x) * 8.9e-16, d * 2.0 ** -40)
                x = x + stp if right else x - stp
                d *= 2.0
                continue
            if _ord(hi) - _ord(lo) <= 1:
                return x, ev + 1
            if nnewton < MAXNEWTON and xn > lo and xn < hi:
                nnewton += 1
                x = float(xn)
                continue
            x = _unord(_ord(lo) + ((_ord(hi) - _ord(lo)) >> 1))
    return np.nan, MAXEVAL


def quantile(name, m, v, probs, gh_T=0, count=False, **kw):
    """(N, nP) quantiles by the rule and the solver of DESIGN 9k; count=True: (quantiles, evaluations [N, nP])."""
    T = int(gh_T) or 20
    m, v = _mv(name, m, v, **kw)
    probs = np.asarray(probs, float).reshape(-1)
    out, nev = np.full((m.shape[0], probs.shape[0]), np.nan), np.zeros((m.shape[0], probs.shape[0]), int)
    ok = (probs > 0.0) & (probs < 1.0)
    if name in DISCRETE:
        cum = support_cdf(name, m, v, T, **kw)
        for j, p in enumerate(probs):
            if ok[j]:
                out[:, j] = 1.0 - (name == "Bernoulli") + (cum < p).sum(1)
        return (out, nev) if count else out
    for n in range(m.shape[0]):
        row = _Row(name, m[n], v[n], T, **kw)
        for j, p in enumerate(probs):
            if ok[j]:
                x, nev[n, j] = _solve(row, float(p))
                with np.errstate(all="ignore"):
                    out[n, j] = np.exp(x) if name in LOGVAR else x
    return (out, nev) if count else out


def support_cdf(name, m, v, gh_T=0, **kw):
    """Bernoulli: [N, 1] = cdf(0); Ordinal: [N, K - 1] = cdf of the labels 1 .. K - 1 (the last point of the support has cdf 1)."""
    m, v = _mv(name, m, v, **kw)
    if name == "Bernoulli":
        return cdf_sf(name, np.zeros(m.shape[0]), m, v, gh_T, **kw)[0][:, None]
    K = len(edges_of(**kw)) + 1
    return np.stack([cdf_sf(name, np.full(m.shape[0], float(c)), m, v, gh_T, **kw)[0] for c in range(1, K)], 1)


def discrete_ties(name, m, v, probs, tolC, gh_T=0, **kw):
    """[N, nP] bool: some cumulative probability of the row lies within tolC 2^-52 S p of p (the label is then not pinned)."""
    m, v = _mv(name, m, v, **kw)
    cum = support_cdf(name, m, v, gh_T, **kw)
    K1 = cum.shape[1]
    S = np.stack([scale(name, np.full(m.shape[0], float(c) if name == "Ordinal" else 0.0), m, v, gh_T, **kw)[:, 0]
                  for c in range(1, K1 + 1)], 1)
    probs = np.asarray(probs, float).reshape(-1)
    return np.stack([(np.abs(cum - p) <= tolC * EPS * S * p).any(1) for p in probs], 1)


def quantile_brentq(name, m, v, probs, gh_T=0, **kw):
    """The independent route: SciPy's bracketing solver on this file's cdf (p <= 1/2) or sf, in y or log y."""
    m, v = _mv(name, m, v, **kw)
    probs = np.asarray(probs, float).reshape(-1)
    out = np.full((m.shape[0], probs.shape[0]), np.nan)
    logv = name in LOGVAR
    for n in range(m.shape[0]):
        for j, p in enumerate(probs):
            use_sf = p > 0.5

            def h(x):
                c, s = cdf_sf(name, np.array([np.exp(x) if logv else x]), m[n:n + 1], v[n:n + 1], gh_T, **kw)
                return ((1.0 - p) - s[0]) if use_sf else (c[0] - p)
            a, b = -1.0, 1.0
            for _ in range(80):
                if h(a) < 0.0:
                    break
                a *= 2.0
            for _ in range(80):
                if h(b) > 0.0:
                    break
                b *= 2.0
            x = optimize.brentq(h, a, b, xtol=1e-300, rtol=8.9e-16, maxiter=500)
            out[n, j] = np.exp(x) if logv else x
    return out


def quantile_excess(name, yhat, m, v, probs, C, gh_T=0, **kw):
    """The mixed criterion of the module docstring per element, as an excess over the tolerance in units of it (<= 0: met).  C: the
    constant (a scalar or [N]); NaN where yhat cannot be judged (`in_range`)."""
    m, v = _mv(name, m, v, **kw)
    yhat = np.asarray(yhat, float).reshape(m.shape[0], -1)
    probs = np.asarray(probs, float).reshape(-1)
    C = np.broadcast_to(np.asarray(C, float), (m.shape[0],))
    out = np.full(yhat.shape, np.nan)
    for j, p in enumerate(probs):
        y = yhat[:, j]
        if name in LOGVAR:
            with np.errstate(all="ignore"):
                ym, yp = np.exp(ulps(np.log(y), -4)), np.exp(ulps(np.log(y), 4))
        else:
            ym, yp = ulps(y, -4), ulps(y, 4)
        col = 1 if p > 0.5 else 0
        tq = 1.0 - p if col else p
        Fm, Fp = cdf_sf(name, ym, m, v, gh_T, **kw)[col], cdf_sf(name, yp, m, v, gh_T, **kw)[col]
        tol = C * EPS * scale(name, y, m, v, gh_T, **kw)[:, col] * tq
        lo, hi = (Fp, Fm) if col else (Fm, Fp)       # the sf decreases
        with np.errstate(all="ignore"):
            out[:, j] = np.where(in_range(name, y), np.maximum(lo - tol - tq, tq - hi - tol) / tol, np.nan)
    return out


def in_range(name, y):
    """Where a quantile can be judged: finite, and in the log-variable families a NORMAL positive number (a quantile below 2^-1022 or
    above the largest double has no 4-ulp neighbourhood in log y that a double y can resolve)."""
    y = np.asarray(y, float)
    return np.isfinite(y) & ((y >= 2.0 ** -1022) if name in LOGVAR else True)


def same_out_of_range(name, got, want):
    """Elements outside `in_range`: both 0 or subnormal, both +inf, or both NaN."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    sub = lambda a: (a >= 0.0) & (a < 2.0 ** -1022)   # noqa: E731
    return (sub(got) & sub(want)) | ((got == np.inf) & (want == np.inf)) | (np.isnan(got) & np.isnan(want))


# ------------------------------------------------------------------------------------------------------------ seeded rows
BULK_KW = {"Gaussian": {"sigma": 0.5}, "Ordinal": {"K": 4, "sigma": 1.0}}


def bulk_rows(name, n, seed, **kw):
    """logpred_ref.bulk_rows with y as the cdf takes it: (N,) values, Ordinal labels, Weibull times."""
    y, m, v = lr.bulk_rows(name, n, seed, **kw)
    y = np.asarray(y, float)
    return (y[:, 0] if y.ndim == 2 else y), m, v


# ------------------------------------------------------------------------------------------------------------ the grid
class Block:
    """One block of pqgrid.npz: rows of one family under one set of keyword arguments."""

    def __init__(self, g, tag, name, kw):
        self.tag, self.name, self.kw = tag, name, kw
        for k in ("y", "m", "v", "cls", "R", "S"):
            setattr(self, k, g["%s__%s" % (tag, k)])
        self.n = len(self.cls)


def load_grid(path=GRID):
    g = np.load(path)
    return [Block(g, tag, name, kw) for tag, name, kw in json.loads(str(g["spec"]))]


def figures(got, R, S, ones_exact=True):
    """|got - R| / (2^-52 S R) per element; 0 where both are the same exact 0, exact 1 or non-finite value, +inf where they differ.
    ones_exact=False: R is a float64 value itself, whose 1.0 may be a rounded 1 - 2^-54: a 1 is then a number like any other."""
    got, R = np.asarray(got, float), np.asarray(R, float)
    with np.errstate(all="ignore"):
        fig = np.abs(got - R) / (EPS * S * np.abs(R))
    special_ = (R == 0.0) | ((R == 1.0) & ones_exact) | ~np.isfinite(R) | ~np.isfinite(got)
    same = (got == R) | (np.isnan(got) & np.isnan(R))
    return np.where(special_, np.where(same, 0.0, np.inf), fig)


def assert_block(got_cdf, got_sf, b, C, what, rows=None):
    """The criterion of the module docstring on one block (or on `rows` of it), output by output; prints the worst figures and returns
    them as {class: (cdf, sf)}."""
    rows = np.arange(b.n) if rows is None else np.asarray(rows)
    out = {BULK: [0.0, 0.0], EDGE: [0.0, 0.0]}
    bad = []
    for col, got in enumerate((got_cdf, got_sf)):
        fig = figures(np.asarray(got, float).reshape(-1), b.R[rows, col], b.S[rows, col])
        for c in (BULK, EDGE):
            sel = b.cls[rows] == c
            if sel.any():
                out[c][col] = float(fig[sel].max())
                over = np.nonzero(sel & ~(fig <= C[c][col]))[0]
                bad += [(("cdf", "sf")[col], int(rows[i]), float(fig[i]), C[c][col]) for i in over]
    print("%-28s bulk cdf %.3g sf %.3g | edge cdf %.3g sf %.3g" % (what, out[BULK][0], out[BULK][1], out[EDGE][0], out[EDGE][1]))
    assert not bad, "%s: %d elements over their constant, e.g. (output, row, figure, constant) %s" % (what, len(bad), bad[:6])
    return {c: tuple(t) for c, t in out.items()}
