"""TEST INFRASTRUCTURE ONLY -- float64 NumPy restatement of the heteroscedastic Negative Binomial likelihood of DESIGN 9h, the
family's oracle (registered with oracle.likelihoods_oracle by the fixture of tests/test_negbin_gpu.py; `oracle/` itself is not edited).

Counts y = 0, 1, 2, ..; f0 = log of the mean, f1 = log of the size r = clip(safe_exp(f1), 1e-9, 1e9).  With lr = log r,
z = min(f0, LIM_VAL) - lr, sp = softplus(z) = max(z, 0) + log1p(exp(-|z|)), p = sigmoid(z), q = 1 - p (both from the same exp(-|z|)):

    log p     = G - lgamma(y+1) + y z - (r + y) sp           G  = lgamma(y+r) - lgamma(r)
    d/df0     = y q - r p                                    D1 = psi(y+r)    - psi(r)
    d2/df0^2  = -(r + y) p q                                 D2 = psi'(y+r)   - psi'(r)
    d/df1     = r (D1 - sp) - d/df0
    d2/df1^2  = r (D1 - sp) + r^2 D2 + 2 r p - (r + y) p q   (the clip is ignored in the derivatives)

Variational expectations: the 20 x 20 Gauss-Hermite tensor rule, weights w / sqrt(pi) once per dimension:
ve = sum w_i w_j log p, dm_d = sum w w d/df_d, dv_d = 1/2 sum w w d2/df_d^2.

G, D1, D2 take the arrangement of the kernel (csrc/lik_device.h, nb_gamma_diffs), never the difference of two large numbers:
    y <= 32            G = log prod_{k<y} (r + k),  D1 = sum 1 / (r + k),  D2 = -sum 1 / (r + k)^2
    y > 32, r >= 16    Stirling's series of the two arguments subtracted term by term, the leading terms in closed form
    y > 32, r < 16     the plain differences (SciPy's gammaln / digamma / zeta(2, .))."""
import numpy as np
from scipy import special

LIM_VAL = np.log(np.finfo(np.float64).max)
LO, HI = 1e-9, 1e9
Y_SUM, R_STIRLING = 32.0, 16.0


def gh(T=20):
    x, w = np.polynomial.hermite.hermgauss(T)
    return x, w / np.sqrt(np.pi)


# ---------------------------------------------------------------------------------------------------- the three differences
def _horner(z, coef):
    s = np.zeros_like(z)
    for c in coef[::-1]:
        s = c + z * s
    return s


def stirling_c(x):
    """lgamma(x) - [(x - 1/2) log x - x + log(2 pi) / 2], x >= 16 (truncation 1.1e-16)."""
    ix = 1.0 / x
    return ix * _horner(ix * ix, [1.0 / 12.0, -1.0 / 360.0, 1.0 / 1260.0, -1.0 / 1680.0, 1.0 / 1188.0])


def stirling_d(x):
    """log x - 1 / (2x) - psi(x), x >= 16 (truncation 2.4e-20)."""
    ix = 1.0 / x
    z = ix * ix
    return z * _horner(z, [1.0 / 12.0, -1.0 / 120.0, 1.0 / 252.0, -1.0 / 240.0, 1.0 / 132.0, -691.0 / 32760.0, 1.0 / 12.0])


def stirling_e(x):
    """psi'(x) - 1 / x - 1 / (2 x^2), x >= 16 (truncation 2.4e-20)."""
    ix = 1.0 / x
    z = ix * ix
    return ix * z * _horner(z, [1.0 / 6.0, -1.0 / 30.0, 1.0 / 42.0, -1.0 / 30.0, 5.0 / 66.0, -691.0 / 2730.0, 7.0 / 6.0])


def gamma_diffs(y, r):
    """(G, D1, D2) for non-negative integer-valued y and r in [1e-9, 1e9], broadcast against each other."""
    y, r = np.broadcast_arrays(np.asarray(y, float), np.asarray(r, float))
    G, D1, D2 = np.empty(y.shape), np.empty(y.shape), np.empty(y.shape)
    small = y <= Y_SUM
    if np.any(small):
        k = np.arange(int(Y_SUM), dtype=float)
        t = r[small][:, None] + k
        on = k < y[small][:, None]
        it = np.where(on, 1.0 / t, 0.0)
        G[small] = np.log(np.prod(np.where(on, t, 1.0), 1))
        D1[small] = it.sum(1)
        D2[small] = -(it * it).sum(1)
    st = ~small & (r >= R_STIRLING)
    if np.any(st):
        yy, rr = y[st], r[st]
        ry, l1 = rr + yy, np.log1p(yy / rr)
        rry = rr * ry
        G[st] = yy * np.log(ry) - yy + (rr - 0.5) * l1 + (stirling_c(ry) - stirling_c(rr))
        D1[st] = l1 + yy / (2.0 * rry) + (stirling_d(rr) - stirling_d(ry))
        D2[st] = -yy / rry - yy * (2.0 * rr + yy) / (2.0 * rry * rry) - (stirling_e(rr) - stirling_e(ry))
    pl = ~small & ~st
    if np.any(pl):
        G[pl], D1[pl], D2[pl] = plain_diffs(y[pl], r[pl])
    return G, D1, D2


def plain_diffs(y, r):
    """The differences as the textbook writes them: what the stable arrangement replaces where r >> y."""
    return (special.gammaln(y + r) - special.gammaln(r), special.digamma(y + r) - special.digamma(r),
            special.zeta(2, y + r) - special.zeta(2, r))


def lgamma_diff(y, r):
    return gamma_diffs(y, r)[0]


def digamma_diff(y, r):
    return gamma_diffs(y, r)[1]


def trigamma_diff(y, r):
    return gamma_diffs(y, r)[2]


# ---------------------------------------------------------------------------------------------------- log p and its derivatives
def size(f1):
    return np.clip(np.exp(np.minimum(f1, LIM_VAL)), LO, HI)


def _terms(y, f0, f1, diffs):
    r = size(f1)
    z = np.minimum(f0, LIM_VAL) - np.log(r)
    a = np.exp(-np.abs(z))
    inv = 1.0 / (1.0 + a)
    sp = np.maximum(z, 0.0) + np.log1p(a)
    p, q = np.where(z >= 0.0, inv, a * inv), np.where(z >= 0.0, a * inv, inv)
    G, D1, D2 = diffs(y, r)
    return r, z, sp, p, q, G, D1, D2


def logpdf_and_derivatives(y, f0, f1, diffs=gamma_diffs):
    """(log p, d/df0, d2/df0^2, d/df1, d2/df1^2) at f = (f0, f1), broadcast."""
    r, z, sp, p, q, G, D1, D2 = _terms(y, f0, f1, diffs)
    d0 = y * q - r * p
    ppq = (r + y) * p * q
    c = r * D1 - r * sp
    return G - special.gammaln(y + 1.0) + y * z - (r + y) * sp, d0, -ppq, c - d0, c + r * r * D2 + 2.0 * r * p - ppq


def _nodes(y, m, v, T=20):
    y = np.asarray(y, float).reshape(-1)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = gh(T)
    f0 = (x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])[:, :, None]
    f1 = (x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[:, None, :]
    return y[:, None, None], f0, f1, w[:, None] * w[None, :]


def var_exp(y, m, v, diffs=gamma_diffs, T=20):
    """y [N], m, v [N, 2] -> ve [N], dm [N, 2], dv [N, 2].  `diffs` swaps the difference functions (the corruption check); T = 20 is
    the contract's rule, any other T a finer / coarser one for convergence checks."""
    yy, f0, f1, W = _nodes(y, m, v, T)
    lp, d0, h0, d1, h1 = logpdf_and_derivatives(yy, f0, f1, diffs)
    s = lambda a: (a * W).sum((1, 2))
    return s(lp), np.stack([s(d0), s(d1)], 1), 0.5 * np.stack([s(h0), s(h1)], 1)


def var_exp_scale(y, m, v):
    """The condition scale S [N, 5] of (ve, dm_0, dm_1, dv_0, dv_1) in float64: the rule's sum over the ABSOLUTE values of the addends
    G, -lgamma(y+1), y z, -r sp, -y sp (and likewise for the derivative formulas), each difference G, D1, D2 counted as ONE addend."""
    yy, f0, f1, W = _nodes(y, m, v)
    r, z, sp, p, q, G, D1, D2 = _terms(yy, f0, f1, gamma_diffs)
    s = lambda a: (a * W).sum((1, 2))
    pq = (r + yy) * p * q
    return np.stack([s(np.abs(G) + special.gammaln(yy + 1.0) + yy * np.abs(z) + (r + yy) * sp),
                     s(yy * q + r * p),
                     s(r * D1 + r * sp + yy * q + r * p),
                     0.5 * s(pq),
                     0.5 * s(r * D1 + r * sp + r * r * np.abs(D2) + 2.0 * r * p + pq)], 1)


# ---------------------------------------------------------------------------------------------------- predictive, moments
def predictive(m, v):
    """Closed form under q(f0) q(f1) (clips ignored, overflow is +inf):  mean = exp(m0 + v0/2),
    variance = mean + exp(2 m0 + 2 v0) exp(-m1 + v1/2) + (exp(v0) - 1) exp(2 m0 + v0).  (N, 1) each."""
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    m0, m1, v0, v1 = m[:, 0], m[:, 1], v[:, 0], v[:, 1]
    with np.errstate(over="ignore"):
        mean = np.exp(m0 + 0.5 * v0)
        third = np.where(v0 > 0.0, np.expm1(v0) * np.exp(2.0 * m0 + v0), 0.0)
        var = mean + np.exp(2.0 * m0 + 2.0 * v0 - m1 + 0.5 * v1) + third
    return mean[:, None], var[:, None]


def moments(f0, f1):
    """Mean and variance of y given f (no clip): mu, mu + mu^2 / r."""
    mu = np.exp(f0)
    return mu, mu + mu * mu * np.exp(-f1)


def draw(rng, f0, f1):
    """Seeded draws y ~ NB(mean exp(f0), size r(f1)) as floats, from NumPy's Gamma-Poisson mixture."""
    r = size(np.asarray(f1, float))
    return rng.poisson(np.exp(np.asarray(f0, float)) * rng.gamma(r) / r).astype(float)
