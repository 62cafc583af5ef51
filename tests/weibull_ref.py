"""TEST INFRASTRUCTURE ONLY -- float64 NumPy restatement of the right-censored Weibull likelihood of DESIGN 9i, the family's oracle
(registered with oracle.likelihoods_oracle by the fixture of tests/test_weibull_gpu.py; `oracle/` itself is not edited).

A row of Y is (y, delta): a time y > 0 and the event indicator, 1.0 (the event was observed at y) or 0.0 (right-censored: the event
is later than y).  f0 = log of the scale lambda, f1 = log of the shape k = clip(safe_exp(f1), 1e-3, 1e3), lk = log k.  With
ly = log y, z = min(k (ly - f0), 680), e = exp(z) = (y / lambda)^k:

    log p     = delta (lk - ly + z) - e          (delta = 0: the log survival function -e)
    d/df0     = k (e - delta)                    d2/df0^2 = -k^2 e
    d/df1     = delta (1 + z) - e z              d2/df1^2 = z (delta - e - e z)       (the clips are ignored in the derivatives)

Variational expectations: the 20 x 20 Gauss-Hermite tensor rule, weights w / sqrt(pi) once per dimension:
ve = sum w_i w_j log p, dm_d = sum w w d/df_d, dv_d = 1/2 sum w w d2/df_d^2.  The arrangement is the kernel's
(csrc/lik_device.h, lik_weibull_wave): ly - f0 per node of f0, k and lk per node of f1, one exp per node of the tensor rule."""
import numpy as np
from scipy import special

LIM_VAL = np.log(np.finfo(np.float64).max)
K_LO, K_HI = 1e-3, 1e3
Z_MAX = 680.0


def gh(T=20):
    x, w = np.polynomial.hermite.hermgauss(T)
    return x, w / np.sqrt(np.pi)


def shape(f1):
    return np.clip(np.exp(np.minimum(f1, LIM_VAL)), K_LO, K_HI)


def split(Y):
    """(y, delta), each [N], of an (N, 2) array of rows."""
    Y = np.asarray(Y, float)
    assert Y.ndim == 2 and Y.shape[1] == 2, Y.shape
    return Y[:, 0], Y[:, 1]


# ---------------------------------------------------------------------------------------------------- log p and its derivatives
def z_of_log(y, k, f0):
    """z = min(k (log y - f0), 680): the contract's form."""
    return np.minimum(k * (np.log(y) - f0), Z_MAX)


def z_of_pow(y, k, f0):
    """z as the logarithm of (y / lambda)^k formed by pow first: what the contract's form replaces (the corruption check).  The
    quotient overflows or vanishes where its logarithm is moderate, and the power loses the digits of z next to 0."""
    with np.errstate(all="ignore"):
        return np.minimum(np.log(np.power(y / np.exp(f0), k)), Z_MAX)


def _terms(y, f0, f1, zform):
    k = shape(f1)
    z = zform(y, k, f0)
    with np.errstate(under="ignore"):
        e = np.exp(z)
    return k, np.log(k), z, e


def logpdf_and_derivatives(y, delta, f0, f1, zform=z_of_log):
    """(log p, d/df0, d2/df0^2, d/df1, d2/df1^2) at f = (f0, f1), broadcast."""
    k, lk, z, e = _terms(y, f0, f1, zform)
    ez = e * z
    return delta * (lk - np.log(y) + z) - e, k * (e - delta), -(k * k * e), delta * (1.0 + z) - ez, z * (delta - e - ez)


def _nodes(Y, m, v, T=20):
    y, delta = split(Y)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = gh(T)
    f0 = (x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])[:, :, None]
    f1 = (x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[:, None, :]
    return y[:, None, None], delta[:, None, None], f0, f1, w[:, None] * w[None, :]


def var_exp(Y, m, v, zform=z_of_log, T=20):
    """Y [N, 2] = (y, delta), m, v [N, 2] -> ve [N], dm [N, 2], dv [N, 2].  `zform` swaps the way z is formed (the corruption check);
    T = 20 is the contract's rule, any other T a finer / coarser one for convergence checks."""
    yy, dd, f0, f1, W = _nodes(Y, m, v, T)
    lp, d0, h0, d1, h1 = logpdf_and_derivatives(yy, dd, f0, f1, zform)
    s = lambda a: (a * W).sum((1, 2))
    return s(lp), np.stack([s(d0), s(d1)], 1), 0.5 * np.stack([s(h0), s(h1)], 1)


def var_exp_scale(Y, m, v):
    """The condition scale S [N, 5] of (ve, dm_0, dm_1, dv_0, dv_1) in float64: the rule's sum over the ABSOLUTE values of the addends
    delta lk, -delta ly, delta z, -e (and likewise for the derivative formulas; tests/weibull_ref_mp.py lists them)."""
    yy, dd, f0, f1, W = _nodes(Y, m, v)
    k, lk, z, e = _terms(yy, f0, f1, z_of_log)
    s = lambda a: (a * W).sum((1, 2))
    az, ez = np.abs(z), e * np.abs(z)
    return np.stack([s(dd * np.abs(lk) + dd * np.abs(np.log(yy)) + dd * az + e),
                     s(k * e + k * dd),
                     s(dd + dd * az + ez),
                     0.5 * s(k * k * e),
                     0.5 * s(dd * az + ez + ez * az)], 1)


def clipped_nodes(Y, m, v):
    """Number of nodes of the 20 x 20 rule at which z takes its clip, per row."""
    yy, dd, f0, f1, W = _nodes(Y, m, v)
    return (shape(f1) * (np.log(yy) - f0) >= Z_MAX).sum((1, 2))


# ---------------------------------------------------------------------------------------------------- predictive, moments
def predictive(m, v, T=20):
    """Mean and variance of the event time under independent q(f0), q(f1) (no clip of the result, overflow is +inf):
    mean = exp(m0 + v0/2) GH_j[Gamma(1 + 1/k_j)], E[y^2] = exp(2 m0 + 2 v0) GH_j[Gamma(1 + 2/k_j)], variance = E[y^2] - mean^2
    (+inf where E[y^2] is).  (N, 1) each; T = 20 is the contract's rule."""
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = gh(T)
    ik = 1.0 / shape(x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])
    with np.errstate(over="ignore", invalid="ignore"):
        g1, g2 = np.exp(special.gammaln(1.0 + ik)) @ w, np.exp(special.gammaln(1.0 + 2.0 * ik)) @ w
        mean = np.exp(m[:, 0] + 0.5 * v[:, 0]) * g1
        e2 = np.exp(2.0 * m[:, 0] + 2.0 * v[:, 0]) * g2
        var = np.where(np.isfinite(e2), e2 - mean * mean, np.inf)
    return mean[:, None], var[:, None]


def moments(f0, f1):
    """Mean and variance of the event time given f: lambda Gamma(1 + 1/k), lambda^2 (Gamma(1 + 2/k) - Gamma(1 + 1/k)^2)."""
    lam, ik = np.exp(f0), 1.0 / shape(np.asarray(f1, float))
    g1, g2 = special.gamma(1.0 + ik), special.gamma(1.0 + 2.0 * ik)
    return lam * g1, lam * lam * (g2 - g1 * g1)


def draw(rng, f0, f1, censored=0.3):
    """Seeded rows (y, delta) [N, 2]: event times from the row's own Weibull, censored at an independent censoring time so that the
    stated share of rows is censored (hetmogp_amd.synthetic.weibull_censored restated: tests do not import the package here)."""
    f0, f1 = np.asarray(f0, float).reshape(-1, 1), np.asarray(f1, float).reshape(-1, 1)
    ik = 1.0 / shape(f1)
    t = np.exp(f0) * (-np.log(1.0 - rng.rand(*f0.shape))) ** ik
    u = -np.log(1.0 - rng.rand(*f0.shape))
    if censored == 0.0:
        return np.hstack([t, np.ones_like(t)])
    c = np.exp(f0) * ((1.0 - censored) / censored * u) ** ik
    return np.hstack([np.minimum(t, c), (t <= c).astype(float)])
