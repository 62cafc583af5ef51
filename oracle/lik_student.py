"""NumPy restatement of the heteroscedastic Student-t likelihood: the reference ships only a constructor
(likelihoods/student.py), so this file restates the project's own contract.  `oracle.likelihoods_oracle` dispatches "Student" here.

Model: f0 = location (identity link), f1 = log of the squared scale, nu = deg_free fixed.  With r = y - f0,
s = exp(min(-f1, LIM_VAL)), u = r^2 s / nu and C = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2:
    log p = C - f1/2 - (nu+1)/2 log1p(u)
Variational expectations: the 20 x 20 Gauss-Hermite tensor rule, weights w/sqrt(pi) once per dimension."""
import numpy as np
from scipy.special import gammaln

LIM_VAL = 709.782712893384       # log(DBL_MAX): GPy safe_exp clip


def logc(nu):
    return gammaln(0.5 * (nu + 1.0)) - gammaln(0.5 * nu) - 0.5 * np.log(nu * np.pi)


def logpdf_and_derivatives(y, f0, f1, nu):
    """log p and its first / second derivatives with respect to f0 and f1 (broadcasting)."""
    r = y - f0
    s = np.exp(np.minimum(-f1, LIM_VAL))
    u = r * r * s / nu
    a = 1.0 / (1.0 + u)
    lp = logc(nu) - 0.5 * f1 - 0.5 * (nu + 1.0) * np.log1p(u)
    d0 = (nu + 1.0) * r * s * a / nu
    d00 = (nu + 1.0) * s * (u - 1.0) * a * a / nu
    d1 = -0.5 + 0.5 * (nu + 1.0) * u * a
    d11 = -0.5 * (nu + 1.0) * u * a * a
    return lp, d0, d1, d00, d11


def var_exp(y, m, v, deg_free=5.0, T=20):
    """y [N], m, v [N, 2] -> ve [N], dm [N, 2], dv [N, 2]."""
    nu = float(deg_free)
    y = np.asarray(y, float).reshape(-1)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = np.polynomial.hermite.hermgauss(T)
    w = w / np.sqrt(np.pi)
    f0 = x[None, :, None] * np.sqrt(2.0 * v[:, 0, None, None]) + m[:, 0, None, None]     # [N, i, 1]
    f1 = x[None, None, :] * np.sqrt(2.0 * v[:, 1, None, None]) + m[:, 1, None, None]     # [N, 1, j]
    W = w[:, None] * w[None, :]
    lp, d0, d1, d00, d11 = logpdf_and_derivatives(y[:, None, None], f0, f1, nu)
    q = lambda g: np.einsum("nij,ij->n", np.broadcast_to(g, (y.shape[0], T, T)), W)
    ve = q(lp)
    dm = np.stack([q(d0), q(d1)], 1)
    dv = 0.5 * np.stack([q(d00), q(d11)], 1)
    return ve, dm, dv


def predictive(m, v, deg_free=5.0):
    nu = float(deg_free)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    mean = m[:, :1] if nu > 1.0 else np.full((m.shape[0], 1), np.nan)
    var = (v[:, :1] + nu / (nu - 2.0) * np.exp(m[:, 1:2] + 0.5 * v[:, 1:2])) if nu > 2.0 else np.full((m.shape[0], 1), np.inf)
    return mean, var
