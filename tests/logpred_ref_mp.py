"""High-precision restatement (mpmath 1.3.0, 50 digits) of the deterministic log predictive density of DESIGN 9j, with the conventions of
tests/lik_ref_mp.py: the float64 inputs (y, m, v, the likelihood's parameters) and the float64 Gauss-Hermite tables are exact numbers,
everything else is carried in high precision.  Per row:

  R = (lpd, ess):  lpd = log sum_i e_i,  ess = (sum_i e_i)^2 / sum_i e_i^2,  e_i = (prod_d w_{i_d}) p(y | f_i)
  S = 1 + sum_i (e_i / sum e) A_i,  A_i = the sum of the absolute values of the addends of log p at node i (listed per family below)

Addends of log p(y | f) (safe_exp(x) = exp(min(x, LIM)), clip9 = clip to [1e-9, 1e9]):
  Gaussian      closed form, one "node":  -log(2 pi)/2,  -log(sigma^2 + v)/2,  -(y - m)^2 / (2 (sigma^2 + v));   ess = +inf
  HetGaussian   nodes over f1 only, var = v0 + safe_exp(f1):  -log(2 pi)/2,  -log(var)/2,  -min(y - m0, sqrt(DBL_MAX))^2 / (2 var)
  Bernoulli     p = clip(ef / (1 + ef), 1e-9, 1 - 1e-9):  y log p,  (1 - y) log(1 - p)
  Poisson       -safe_exp(f),  y f,  -lgamma(y + 1)
  Exponential   b = clip9(safe_exp(-f)):  -log b,  -y / b
  Categorical   p_k = clip(e_k / den), p_K = clip(1 / den), den = 1 + sum e_k:  log p_y,  -log sum_k p_k
  Student       log c(nu),  -f1 / 2,  -(nu + 1)/2 log1p((y - f0)^2 safe_exp(-f1) / nu)
  Ordinal       log (Phi(b) - Phi(a))                (one addend)
  NegBinomial   r = clip9(safe_exp(f1)), z = min(f0, LIM) - log r:  lgamma(y + r) - lgamma(r),  -lgamma(y + 1),  y z,  -(r + y) softplus(z)
  Weibull       k = clip(safe_exp(f1), 1e-3, 1e3), z = min(k (log y - f0), 680):  delta log k,  -delta log y,  delta z,  -exp(z)
  Gamma         a = clip9(safe_exp(f0)), b = clip9(safe_exp(f1)):  -lgamma(a),  a log b,  (a - 1) log y,  -b y
  Beta          (a - 1) log y,  (b - 1) log(1 - y),  -lgamma(a),  -lgamma(b),  lgamma(a + b)
  Dirichlet     lgamma(A),  -lgamma(a_k) (each k),  (a_k - 1) log y_k (each k)

Independent of the float64 code (imports neither hetmogp_amd nor logpred_ref)."""
import itertools

import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
LIM_VAL = mpf(709.782712893384)
SQRT_DBL_MAX = mpf(1.3407807929942596e154)
NINF = mpf("-inf")
DBL_MAX = mpf(1.7976931348623157e308)


def gh(T):
    x, w = np.polynomial.hermite.hermgauss(int(T))
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def _sexp(f):
    return mpmath.exp(min(f, LIM_VAL))


def _clip(x, lo, hi):
    return min(max(x, mpf(lo)), mpf(hi))


def _log(x):
    return NINF if x == 0 else mpmath.log(x)


def _ncdf_diff_log(a, b):
    """log(Phi(b) - Phi(a)), a < b (either may be infinite), without cancellation between two values next to 1."""
    if a + b > 0:
        a, b = -b, -a
    Fa = mpf(0) if a == NINF else mpmath.erfc(-a / mpmath.sqrt(2)) / 2
    if b > 0:
        Q = Fa + mpmath.erfc(b / mpmath.sqrt(2)) / 2
        return mpmath.log1p(-Q)
    return mpmath.log(mpmath.erfc(-b / mpmath.sqrt(2)) / 2 - Fa)


def addends(name, y, f, kw):
    """The addends of log p(y | f) at one node: y a float (or a sequence of floats), f a list of mpf."""
    if name == "Bernoulli":
        ef = _sexp(f[0])
        p = _clip(ef / (1 + ef), 1e-9, 1.0 - 1e-9)
        yy = mpf(float(y))
        return [yy * mpmath.log(p), (1 - yy) * mpmath.log(1 - p)]
    if name == "Poisson":
        yy = mpf(float(y))
        return [-_sexp(f[0]), yy * f[0], -mpmath.loggamma(yy + 1)]
    if name == "Exponential":
        b = _clip(_sexp(-f[0]), 1e-9, 1e9)
        return [-mpmath.log(b), -mpf(float(y)) / b]
    if name == "Categorical":
        K = int(kw["K"])
        e = [_sexp(t) for t in f]
        den = 1 + sum(e)
        p = [_clip(t / den, 1e-9, 1.0 - 1e-9) for t in e] + [_clip(1 / den, 1e-9, 1.0 - 1e-9)]
        assert len(p) == K
        return [mpmath.log(p[int(y) - 1]), -mpmath.log(sum(p))]
    if name == "Student":
        nu = mpf(float(kw.get("deg_free", 5.0)))
        r = mpf(float(y)) - f[0]
        logc = mpmath.loggamma((nu + 1) / 2) - mpmath.loggamma(nu / 2) - mpmath.log(nu * mpmath.pi) / 2
        return [logc, -f[1] / 2, -(nu + 1) / 2 * mpmath.log1p(r * r * _sexp(-f[1]) / nu)]
    if name == "Ordinal":
        edges = kw.get("bin_edges")
        if edges is None:
            edges = [k - 0.5 * int(kw["K"]) for k in range(1, int(kw["K"]))]
        ext = [NINF] + [mpf(float(t)) for t in edges] + [mpf("inf")]
        s = mpf(float(kw.get("sigma", 1.0)))
        k = int(y)
        return [_ncdf_diff_log((ext[k - 1] - f[0]) / s, (ext[k] - f[0]) / s)]
    if name == "NegBinomial":
        yy = mpf(float(y))
        r = _clip(_sexp(f[1]), 1e-9, 1e9)
        z = min(f[0], LIM_VAL) - mpmath.log(r)
        sp = max(z, 0) + mpmath.log1p(mpmath.exp(-abs(z)))
        return [mpmath.loggamma(yy + r) - mpmath.loggamma(r), -mpmath.loggamma(yy + 1), yy * z, -(r + yy) * sp]
    if name == "Weibull":
        ly, d = mpmath.log(mpf(float(y[0]))), mpf(float(y[1]))
        k = _clip(_sexp(f[1]), 1e-3, 1e3)
        z = min(k * (ly - f[0]), mpf(680))
        return [d * mpmath.log(k), -d * ly, d * z, -mpmath.exp(z)]
    if name == "Gamma":
        yy = mpf(float(y))
        a, b = _clip(_sexp(f[0]), 1e-9, 1e9), _clip(_sexp(f[1]), 1e-9, 1e9)
        return [-mpmath.loggamma(a), a * mpmath.log(b), (a - 1) * _log(yy), -b * yy]
    if name == "Beta":
        yy = mpf(float(y))
        a, b = _clip(_sexp(f[0]), 1e-9, 1e9), _clip(_sexp(f[1]), 1e-9, 1e9)
        return [(a - 1) * _log(yy), (b - 1) * _log(1 - yy), -mpmath.loggamma(a), -mpmath.loggamma(b), mpmath.loggamma(a + b)]
    if name == "Dirichlet":
        a = [_clip(_sexp(t), 1e-9, 1e9) for t in f]
        return [mpmath.loggamma(sum(a))] + [-mpmath.loggamma(t) for t in a] + [(t - 1) * mpmath.log(mpf(float(u))) for t, u in zip(a, y)]
    raise KeyError(name)


def row(name, y, m, v, gh_T=0, **kw):
    """One row: y a float (Weibull: (time, indicator); Dirichlet: the K shares), m, v [J] float64 -> (R [2] = lpd, ess; S) as float64."""
    m, v = [float(t) for t in np.ravel(m)], [float(t) for t in np.ravel(v)]
    with mp.workdps(WORK_DPS):
        if name == "Gaussian":
            s = 0.5 if kw.get("sigma") is None else float(kw["sigma"])
            s2 = mpf(s) ** 2 + mpf(v[0])
            d = mpf(float(y)) - mpf(m[0])
            t = [-mpmath.log(2 * mpmath.pi) / 2, -mpmath.log(s2) / 2, -d * d / (2 * s2)]
            return np.array([float(sum(t)), np.inf]), float(1 + sum(abs(a) for a in t))
        T = int(gh_T) or (10 if name in ("Categorical", "Dirichlet") else 20)
        x, w = gh(T)
        nodes = []     # (weight, [addends])
        if name == "HetGaussian":
            d = min(mpf(float(y)) - mpf(m[0]), SQRT_DBL_MAX)
            for xi, wi in zip(x, w):
                var = mpf(v[0]) + _sexp(mpf(m[1]) + mpmath.sqrt(2 * mpf(v[1])) * xi)
                nodes.append((wi, [-mpmath.log(2 * mpmath.pi) / 2, -mpmath.log(var) / 2, -d * d / (2 * var)]))
        else:
            J = len(m)
            fd = [[mpf(m[k]) + mpmath.sqrt(2 * mpf(v[k])) * xi for xi in x] for k in range(J)]
            for idx in itertools.product(range(T), repeat=J):
                W = mpf(1)
                for i in idx:
                    W *= w[i]
                nodes.append((W, addends(name, y, [fd[k][i] for k, i in enumerate(idx)], kw)))
        s1 = s2 = sa = mpf(0)
        for W, t in nodes:
            l = sum(t)
            if l == NINF or l < -DBL_MAX:      # log p is a float64 number: below -DBL_MAX it is -inf, and the node contributes nothing
                continue
            e = W * mpmath.exp(l)
            s1 += e
            s2 += e * e
            sa += e * sum(abs(a) for a in t)
        if s1 == 0:
            return np.array([-np.inf, np.nan]), 1.0
        return np.array([float(mpmath.log(s1)), float(s1 * s1 / s2)]), float(1 + sa / s1)
