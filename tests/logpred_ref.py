"""float64 NumPy / SciPy restatement of the deterministic per-row log predictive density of DESIGN 9j, and the loader / criterion of
its grid tests/golden/lpgrid.npz (tools/make_logpred_grid.py; 50-digit values from tests/logpred_ref_mp.py).

For a row with q(f) = N(m, diag v) over the family's J functions

    lpd = log sum_nodes (prod_d w_{i_d}) p(y | f_node),   f_node,d = m_d + sqrt(2 v_d) x_{i_d},    ess = (sum e)^2 / sum e^2,  e = (prod w) p

with the normalised Gauss-Hermite weights once per dimension, T = 20 nodes per dimension (Categorical, Dirichlet: 10).  log p(y|f) is
what the Monte-Carlo kernel evaluates per sample -- same links and clips --, for Gamma and Beta their densities with the families' links
and clips.  Gaussian: the closed form log N(y; m, sigma^2 + v), ess = +inf.  HetGaussian: f0 integrated analytically, T nodes over f1
of log N(y; m0, v0 + safe_exp(f1)).

Criterion (tests/likgrid.py's): |got - R| <= C 2^-52 S per element, S = 1 + sum_i wbar_i A_i with wbar the normalised node mass and A_i
the sum of the absolute values of the addends of log p at node i (the leading 1: the sum and the logarithm).  ess is a ratio of two such
sums: |got - R| <= 4 C 2^-52 S R.

C_ORACLE[family][class] = (lpd, ess): the largest figure of THIS file against the grid, per family, row class and output, rounded up to
the next power of two (measured 2026-10-19, CPU, NumPy / SciPy; `python tools/make_logpred_grid.py --measure` prints the raw
figures).  The kernels get C_KERNEL = max(16, 4 C_ORACLE)."""
import json
import os
import sys

import numpy as np
from scipy import special

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import likgrid as lg               # noqa: E402
import negbin_ref as nb            # noqa: E402
import weibull_ref as wr           # noqa: E402
from oracle import lik_dirichlet as ld   # noqa: E402
from oracle import lik_ordinal as lo     # noqa: E402
from oracle import lik_student as ls     # noqa: E402

LIM_VAL = 709.782712893384
SQRT_DBL_MAX = 1.3407807929942596e154
BULK, EDGE = lg.BULK, lg.EDGE
GRID = os.path.join(lg.GOLDEN, "lpgrid.npz")
FAMILIES = ("Gaussian", "Bernoulli", "HetGaussian", "Categorical", "Poisson", "Exponential", "Gamma", "Beta", "Student", "Ordinal",
            "Dirichlet", "NegBinomial", "Weibull")
MC_REFUSED = ("Gamma", "Beta")     # hmogp_log_predictive (Monte Carlo) refuses these two

# family -> {class: (C_lpd, C_ess)}, measured 2026-10-19 (see the module docstring; the raw figures beside each line).  The large figures
# are properties of the formulas in float64 that S does not fold in (DESIGN 9a's rule); each is named on its line.
C_ORACLE = {
    "Gaussian": {BULK: (1, 1), EDGE: (1, 1)},            # raw 0.561 0 | 0.803 0
    "Bernoulli": {BULK: (1, 1), EDGE: (1, 1)},           # raw 0.92 0.343 | 0.951 0.196
    "HetGaussian": {BULK: (1, 1), EDGE: (2, 1)},         # raw 0.816 0.286 | 1.32 0.0877
    "Categorical": {BULK: (2, 1), EDGE: (2, 1)},         # raw 1.01 0.539 | 1.96 0.366
    "Poisson": {BULK: (1, 1), EDGE: (128, 1)},           # raw 0.531 0.334 | 128 0.196     (|f| eps in exp(f) at |f| ~ 700)
    "Exponential": {BULK: (1, 1), EDGE: (8, 1)},         # raw 0.818 0.23 | 7.1 0.115
    "Gamma": {BULK: (1, 1), EDGE: (2, 1)},               # raw 0.673 0.129 | 1.05 0.0884
    "Beta": {BULK: (1, 1), EDGE: (2, 1)},                # raw 0.436 0.203 | 1.48 0.101
    "Student": {BULK: (256, 1), EDGE: (512, 1)},         # raw 224 0.233 | 259 0.206       (nu = 300: oracle/lik_student.logc subtracts two
                                                         #  lgammas of ~600; every other block stays below 1)
    "Ordinal": {BULK: (1, 1), EDGE: (128, 8)},           # raw 0.856 0.391 | 104 7.5       (the narrow middle bin: E(b) - E(a))
    "Dirichlet": {BULK: (1, 1), EDGE: (1, 1)},           # raw 0.479 0.0498 | 0.255 0.101
    "NegBinomial": {BULK: (1, 1), EDGE: (4, 1)},         # raw 0.645 0.438 | 3.48 0.308
    "Weibull": {BULK: (4, 1), EDGE: (16, 1)},            # raw 2.01 0.318 | 11.5 0.391
}


def c_oracle(family):
    return C_ORACLE[family]


def c_kernel(family):
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE[family].items()}


def c_sum(family):
    """Bound between a kernel result and this file's float64 value: each within its own constant of R."""
    k, o = c_kernel(family), c_oracle(family)
    return {c: tuple(a + b for a, b in zip(k[c], o[c])) for c in k}


# ------------------------------------------------------------------------------------------------------------ shapes
def dim_f(name, **kw):
    if name == "Categorical":
        return int(kw["K"]) - 1
    if name == "Dirichlet":
        return int(kw["K"])
    return 1 if name in ("Gaussian", "Bernoulli", "Poisson", "Exponential", "Ordinal") else 2


def dim_y(name, **kw):
    return int(kw["K"]) if name == "Dirichlet" else (2 if name == "Weibull" else 1)


def default_T(name):
    return 10 if name in ("Categorical", "Dirichlet") else 20


def gh(T):
    x, w = np.polynomial.hermite.hermgauss(int(T))
    return x, w / np.sqrt(np.pi)


def _safe_exp(f):
    return np.exp(np.minimum(f, LIM_VAL))


def _clip9(x):
    return np.clip(x, 1e-9, 1e9)


def _yrows(name, y, **kw):
    dy = dim_y(name, **kw)
    y = np.asarray(y, float)
    return y.reshape(-1) if dy == 1 else y.reshape(-1, dy)


# ------------------------------------------------------------------------------------------------------------ log p(y | f)
def _logpdf_terms(name, y, F, **kw):
    """y: the rows ([N], [N, 2], [N, K]); F [N, S, J] -> (log p [N, S], A [N, S] = sum of the absolute values of its addends)."""
    with np.errstate(all="ignore"):
        if name in ("Dirichlet",):
            a = _clip9(_safe_exp(F))
            ly = np.log(y)[:, None, :]
            t0, t1, t2 = special.gammaln(a.sum(-1)), special.gammaln(a), (a - 1.0) * ly
            return ld.logpdf(y, F), np.abs(t0) + np.abs(t1).sum(-1) + np.abs(t2).sum(-1)
        if name == "Weibull":
            yy, dl = y[:, 0:1], y[:, 1:2]
            f0, f1 = F[..., 0], F[..., 1]
            k, lk, z, e = wr._terms(yy, f0, f1, wr.z_of_log)
            return wr.logpdf_and_derivatives(yy, dl, f0, f1)[0], dl * (np.abs(lk) + np.abs(np.log(yy)) + np.abs(z)) + e
        yy = y[:, None]
        f0 = F[..., 0]
        if name == "Gaussian":
            s = 0.5 if kw.get("sigma") is None else float(kw["sigma"])
            t = [np.full(f0.shape, -0.5 * np.log(2.0 * np.pi)), np.full(f0.shape, -np.log(s)), -0.5 * ((yy - f0) / s) ** 2]
        elif name == "Bernoulli":
            ef = _safe_exp(f0)
            p = np.clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9)
            t = [yy * np.log(p), (1.0 - yy) * np.log(1.0 - p)]
        elif name == "Poisson":
            t = [-_safe_exp(f0), yy * f0, -special.gammaln(yy + 1.0) + 0.0 * f0]
        elif name == "Exponential":
            b = _clip9(_safe_exp(-f0))
            t = [-np.log(b), -yy / b]
        elif name == "HetGaussian":
            f1 = F[..., 1]
            d = np.minimum(yy - f0, SQRT_DBL_MAX)
            t = [np.full(f0.shape, -0.5 * np.log(2.0 * np.pi)), -0.5 * f1, -0.5 * (d * d / _safe_exp(f1))]
        elif name == "Categorical":
            K = int(kw["K"])
            e = _safe_exp(F)
            den = 1.0 + e.sum(-1)
            p = np.concatenate([np.clip(e / den[..., None], 1e-9, 1.0 - 1e-9), np.clip(1.0 / den, 1e-9, 1.0 - 1e-9)[..., None]], -1)
            lab = np.broadcast_to(yy.astype(int) - 1, f0.shape)
            py = np.take_along_axis(p, lab[..., None], -1)[..., 0]
            lp = np.log(py / p.sum(-1))
            return lp, np.abs(np.log(py)) + np.abs(np.log(p.sum(-1)))
        elif name == "Student":
            nu = float(kw.get("deg_free", 5.0))
            f1 = F[..., 1]
            lp = ls.logpdf_and_derivatives(yy, f0, f1, nu)[0]
            return lp, np.abs(ls.logc(nu)) + np.abs(0.5 * f1) + np.abs(lp - ls.logc(nu) + 0.5 * f1)
        elif name == "Ordinal":
            lp = lo.logpdf(np.broadcast_to(yy, f0.shape), f0, kw.get("K"), kw.get("bin_edges"), kw.get("sigma", 1.0))
            return lp, np.abs(lp)
        elif name == "NegBinomial":
            f1 = F[..., 1]
            r, z, sp, p, q, G, D1, D2 = nb._terms(yy, f0, f1, nb.gamma_diffs)
            lp = nb.logpdf_and_derivatives(yy, f0, f1)[0]
            return lp, np.abs(G) + special.gammaln(yy + 1.0) + np.abs(yy * z) + (r + yy) * sp
        elif name == "Gamma":
            a, b = _clip9(_safe_exp(f0)), _clip9(_safe_exp(F[..., 1]))
            t = [-special.gammaln(a), a * np.log(b), (a - 1.0) * np.log(yy), -b * yy]
        elif name == "Beta":
            a, b = _clip9(_safe_exp(f0)), _clip9(_safe_exp(F[..., 1]))
            lga, lgb, lgab = special.gammaln(a), special.gammaln(b), special.gammaln(a + b)
            lp = (a - 1.0) * np.log(yy) + (b - 1.0) * np.log(1.0 - yy) - (lga + lgb - lgab)
            return lp, np.abs((a - 1.0) * np.log(yy)) + np.abs((b - 1.0) * np.log(1.0 - yy)) + np.abs(lga) + np.abs(lgb) + np.abs(lgab)
        else:
            raise KeyError(name)
        lp = t[0]
        for a in t[1:]:
            lp = lp + a
        return lp, sum(np.abs(a) for a in t)


def _as_nodes(name, y, F, **kw):
    J = dim_f(name, **kw)
    y = _yrows(name, y, **kw)
    F = np.asarray(F, float)
    flat = F.ndim < 3
    F = F.reshape(y.shape[0], 1, J) if flat else F
    return y, F, flat


def logpdf(name, y, F, **kw):
    """log p(y | f): y the rows, F [N, J] (-> [N]) or [N, S, J] (-> [N, S]).  Gaussian: the density with the task's sigma."""
    y, F, flat = _as_nodes(name, y, F, **kw)
    lp = _logpdf_terms(name, y, F, **kw)[0]
    return lp[:, 0] if flat else lp


# ------------------------------------------------------------------------------------------------------------ the rule
def _tensor_nodes(m, v, T):
    """m, v [N, J] -> F [N, T^J, J], W [T^J]: node index = the digits (i_0 .. i_{J-1}), i_{J-1} fastest."""
    x, w = gh(T)
    N, J = m.shape
    idx = np.stack(np.meshgrid(*([np.arange(T)] * J), indexing="ij"), -1).reshape(-1, J)
    F = m[:, None, :] + np.sqrt(2.0 * v)[:, None, :] * x[idx][None, :, :]
    return F, np.prod(w[idx], 1)


def _rule_terms(name, y, m, v, T, **kw):
    """(log p [N, S], A [N, S], W [S]) at the nodes of the rule; Gaussian / HetGaussian in their own forms."""
    y = _yrows(name, y, **kw)
    J = dim_f(name, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    with np.errstate(all="ignore"):
        if name == "Gaussian":
            s = 0.5 if kw.get("sigma") is None else float(kw["sigma"])
            s2 = s * s + v[:, 0]
            d = y - m[:, 0]
            t = [np.full(d.shape, -0.5 * np.log(2.0 * np.pi)), -0.5 * np.log(s2), -0.5 * (d * d / s2)]
            return (t[0] + t[1] + t[2])[:, None], sum(np.abs(a) for a in t)[:, None], np.ones(1)
        if name == "HetGaussian":
            x, w = gh(T)
            var = v[:, 0:1] + _safe_exp(m[:, 1:2] + np.sqrt(2.0 * v[:, 1:2]) * x[None, :])
            d = np.minimum(y - m[:, 0], SQRT_DBL_MAX)[:, None]
            t = [np.full(var.shape, -0.5 * np.log(2.0 * np.pi)), -0.5 * np.log(var), -0.5 * (d * d / var)]
            return t[0] + t[1] + t[2], sum(np.abs(a) for a in t), w
        F, W = _tensor_nodes(m, v, T)
        lp, A = _logpdf_terms(name, y, F, **kw)
        return lp, A, W


def _combine(lp, W):
    """-> (lpd, ess, wbar [N, S]) from log p at the nodes and their weights; nodes with log p = -inf contribute nothing."""
    with np.errstate(all="ignore"):
        mx = np.max(lp, 1, keepdims=True)
        none = np.isneginf(mx)
        e = W[None, :] * np.exp(lp - np.where(none, 0.0, mx))
        s1, s2 = e.sum(1), (e * e).sum(1)
        lpd = np.where(none[:, 0], -np.inf, mx[:, 0] + np.log(s1))
        ess = np.where(none[:, 0], np.nan, s1 * s1 / s2)
        return lpd, ess, e / s1[:, None]


def lpd(name, y, m, v, gh_T=0, **kw):
    """(lpd [N], ess [N]) by the rule of DESIGN 9j."""
    T = int(gh_T) or default_T(name)
    lp, A, W = _rule_terms(name, y, m, v, T, **kw)
    a, e, _ = _combine(lp, W)
    if name == "Gaussian":
        e = np.full(a.shape, np.inf)
    return a, e


def lpd_scale(name, y, m, v, gh_T=0, **kw):
    """S [N] = 1 + sum_i wbar_i A_i (float64: a scale needs no more)."""
    T = int(gh_T) or default_T(name)
    lp, A, W = _rule_terms(name, y, m, v, T, **kw)
    wbar = _combine(lp, W)[2]
    with np.errstate(all="ignore"):
        return 1.0 + np.nansum(np.where(wbar > 0.0, wbar * A, 0.0), 1)


# ------------------------------------------------------------------------------------------------------------ the integral itself
DENSE_T = {1: (150, 120), 2: (150, 120), 3: (40, 32), 4: (18, 14)}


def dense(name, y, m, v, T, moments=False, chunk=None, **kw):
    """The integral log E_q[p(y | f)] itself by a T-node-per-dimension tensor rule over ALL of the family's dimensions (every family
    through the same path, Gaussian and HetGaussian included).  moments=True: (log E[p], log E[p^2])."""
    y = _yrows(name, y, **kw)
    J = dim_f(name, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    chunk = chunk or max(1, int(2e5 // (T ** J)))
    o1, o2 = np.empty(len(y)), np.empty(len(y))
    for r0 in range(0, len(y), chunk):
        sl = slice(r0, r0 + chunk)
        F, W = _tensor_nodes(m[sl], v[sl], T)
        lp = _logpdf_terms(name, y[sl], F, **kw)[0]
        with np.errstate(all="ignore"):
            lw = np.log(W)[None, :]
            o1[sl], o2[sl] = special.logsumexp(lw + lp, axis=1), special.logsumexp(lw + 2.0 * lp, axis=1)
    return (o1, o2) if moments else o1


def dense_checked(name, y, m, v, **kw):
    """(log E[p], log E[p^2], ok): `dense` at the two node counts of DENSE_T; ok where they agree to 1e-4."""
    Ta, Tb = DENSE_T[dim_f(name, **kw)]
    a1, a2 = dense(name, y, m, v, Ta, moments=True, **kw)
    b1 = dense(name, y, m, v, Tb, **kw)
    return a1, a2, np.abs(a1 - b1) <= 1e-4


def mc_se(name, y, m, v, S, **kw):
    """Standard error of the S-sample log-mean-exp estimate of the row's lpd: sqrt((E[p^2] / E[p]^2 - 1) / S), from `dense`."""
    a1, a2, _ = dense_checked(name, y, m, v, **kw)
    with np.errstate(all="ignore"):
        return np.sqrt(np.maximum(np.exp(a2 - 2.0 * a1) - 1.0, 0.0) / S)


# ------------------------------------------------------------------------------------------------------------ seeded bulk rows
def draw_y(name, rng, F, **kw):
    """One observation per row from the model at f = F [N, J]."""
    N = F.shape[0]
    with np.errstate(all="ignore"):
        if name == "Gaussian":
            return F[:, 0] + (0.5 if kw.get("sigma") is None else kw["sigma"]) * rng.randn(N)
        if name == "Bernoulli":
            return (rng.rand(N) < 1.0 / (1.0 + np.exp(-F[:, 0]))).astype(float)
        if name == "HetGaussian":
            return F[:, 0] + np.exp(0.5 * F[:, 1]) * rng.randn(N)
        if name == "Categorical":
            e = np.concatenate([np.exp(F), np.ones((N, 1))], 1)
            c = np.cumsum(e / e.sum(1, keepdims=True), 1)
            return 1.0 + np.minimum((rng.rand(N)[:, None] > c).sum(1), e.shape[1] - 1)
        if name == "Poisson":
            return rng.poisson(np.exp(F[:, 0])).astype(float)
        if name == "Exponential":
            return np.maximum(rng.exponential(1.0, N) * _clip9(np.exp(-F[:, 0])), 1e-12)      # mean b = e^-f
        if name == "Gamma":
            return np.maximum(rng.gamma(np.exp(F[:, 0]), 1.0) / np.exp(F[:, 1]), 1e-12)
        if name == "Beta":
            return np.clip(rng.beta(np.exp(F[:, 0]), np.exp(F[:, 1])), 1e-9, 1.0 - 1e-9)
        if name == "Student":
            return F[:, 0] + np.exp(0.5 * F[:, 1]) * rng.standard_t(kw.get("deg_free", 5.0), N)
        if name == "Ordinal":
            edges = lo.edges_of(kw.get("K"), kw.get("bin_edges"))
            z = F[:, 0] + kw.get("sigma", 1.0) * rng.randn(N)
            return 1.0 + (z[:, None] > edges[None, :]).sum(1)
        if name == "Dirichlet":
            g = np.maximum(rng.gamma(_clip9(np.exp(F)), 1.0), 1e-12)
            return g / g.sum(1, keepdims=True)
        if name == "NegBinomial":
            r = np.exp(F[:, 1])
            return rng.poisson(rng.gamma(r, np.exp(F[:, 0]) / r)).astype(float)
        if name == "Weibull":
            t = np.exp(F[:, 0]) * rng.exponential(1.0, N) ** (1.0 / wr.shape(F[:, 1]))
            return np.stack([np.maximum(t, 1e-12), (np.arange(N) % 3 != 0).astype(float)], 1)
    raise KeyError(name)


BULK_KW = {"Gaussian": {"sigma": 0.5}, "Categorical": {"K": 3}, "Student": {"deg_free": 4.0}, "Ordinal": {"K": 4, "sigma": 1.0},
           "Dirichlet": {"K": 3}}


def bulk_rows(name, n, seed, vlo=1e-3, vhi=4.0, mlim=3.0, **kw):
    """Seeded bulk rows: m uniform in [-mlim, mlim], v log-uniform in [vlo, vhi], y drawn from the model at a draw f ~ q(f)."""
    rng = np.random.RandomState(seed)
    J = dim_f(name, **kw)
    m = rng.uniform(-mlim, mlim, (n, J))
    v = np.exp(rng.uniform(np.log(vlo), np.log(vhi), (n, J)))
    y = draw_y(name, rng, m + np.sqrt(v) * rng.randn(n, J), **kw)
    return y, m, v


# ------------------------------------------------------------------------------------------------------------ the grid
class Block:
    """One block of lpgrid.npz: rows of one family under one set of keyword arguments."""

    def __init__(self, g, tag, name, kw):
        self.tag, self.name, self.kw = tag, name, kw
        for k in ("y", "m", "v", "cls", "R", "S"):
            setattr(self, k, g["%s__%s" % (tag, k)])
        self.n = len(self.cls)


def load_grid(path=GRID):
    g = np.load(path)
    return [Block(g, tag, name, kw) for tag, name, kw in json.loads(str(g["spec"]))]


def assert_block(got_lpd, got_ess, b, C, what, rows=None):
    """The criterion of the module docstring on one block (or on `rows` of it), output by output (a Gaussian row's ess = +inf must not
    take its lpd out of the check); prints the worst figures, returns them as {class: (lpd, ess)}."""
    rows = np.arange(b.n) if rows is None else np.asarray(rows)
    R, S, cls = b.R[rows], b.S[rows], b.cls[rows]
    out = []
    for col, got in enumerate((got_lpd, got_ess)):
        with np.errstate(all="ignore"):
            scale = S if col == 0 else 4.0 * S * np.abs(R[:, 1])
            scale = np.where(np.isfinite(scale), scale, 1.0)[:, None]
        Rc = R[:, col:col + 1]
        w = lg.assert_rows(np.asarray(got, float).reshape(-1, 1), Rc, scale, lg.classes(Rc), np.array([0]), cls,
                           {c: (t[col], 0.0, 0.0) for c, t in C.items()}, "%s %s" % (what, ("lpd", "ess")[col]))
        out.append(w)
    return {c: (out[0][c][0], out[1][c][0]) for c in (BULK, EDGE)}
