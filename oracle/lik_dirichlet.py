"""Float64 NumPy / SciPy restatement of the Dirichlet likelihood of DESIGN 9d, all four building blocks.  The reference's
likelihoods/dirichlet.py is a constructor only, so this file restates the project's own contract:

    y on the open simplex, K functions, a_k = clip(safe_exp(f_k), 1e-9, 1e9), A = sum_k a_k
    log p(y | f) = lgamma(A) - sum_k lgamma(a_k) + sum_k (a_k - 1) log y_k

and the variational expectations in the DECOMPOSED form the contract defines them in (10 nodes per dimension, weights w / sqrt(pi)
once per dimension, W = prod_k w_{i_k}):

    ve   = sum_nodes W lgamma(A)  - sum_k sum_i w_i lgamma(a_k(i))    + sum_k (sum_i w_i a_k(i) - 1) log y_k
    dm_k = sum_nodes W a_k psi(A) - sum_i w_i a_k(i) psi(a_k(i))      + (sum_i w_i a_k(i)) log y_k
    dv_k = 1/2 [ dm_k + sum_nodes W a_k^2 psi'(A) - sum_i w_i a_k(i)^2 psi'(a_k(i)) ]

It imports nothing from hetmogp_amd.  Special functions are SciPy's (gammaln, psi, zeta(2, .)); the sums run in NumPy's order (einsum over
the whole tensor), not the kernel's lane-strided one.  A is summed k = 0, 1, .. like the kernel's: `predictive` forms A - a_k literally as
the contract writes it, and that difference amplifies a different rounding of A where one a_k dominates."""
import numpy as np
from scipy import special

LIM_VAL = 709.782712893384
MAXK = 4


def safe_exp(f):
    return np.exp(np.minimum(f, LIM_VAL))


def alpha_of(f):
    return np.clip(safe_exp(f), 1e-9, 1e9)


def gh(T=10):
    x, w = np.polynomial.hermite.hermgauss(T)
    return x, w / np.sqrt(np.pi)


def _rows(y, m, v, K):
    K = int(K)
    assert 2 <= K <= MAXK
    return K, np.asarray(y, float).reshape(-1, K), np.asarray(m, float).reshape(-1, K), np.asarray(v, float).reshape(-1, K)


def _tensor(a, w):
    """a [N, K, T] -> A [N, T, .., T] (summed k = 0, 1, ..), W [T, .., T], and a_k broadcast views."""
    N, K, T = a.shape
    views, A, W = [], None, None
    for k in range(K):
        shape = [1] * K
        shape[k] = T
        ak = a[:, k, :].reshape([N] + shape)
        wk = w.reshape(shape)
        views.append(ak)
        A = ak if A is None else A + ak
        W = wk if W is None else W * wk
    return A, W, views


def _sum_nodes(X):
    return X.reshape(X.shape[0], -1).sum(1)


def var_exp(y, m, v, K, chunk=64, scales=False, T=10):
    """y [N, K] compositions, m, v [N, K] -> ve [N], dm [N, K], dv [N, K]; with `scales` the condition scales S instead (the sum of
    the weighted absolute values of the same addends, tests/dirichlet_ref_mp.py).  T: nodes per dimension (10 is the contract's rule)."""
    K, y, m, v = _rows(y, m, v, K)
    N = len(y)
    x, w = gh(T)
    ly = np.log(y)
    ve, dm, dv = np.zeros(N), np.zeros((N, K)), np.zeros((N, K))
    ab = np.abs if scales else (lambda t: t)
    sg = 1.0 if scales else -1.0
    for s in range(0, N, chunk):
        e = slice(s, min(N, s + chunk))
        a = alpha_of(m[e, :, None] + np.sqrt(2.0 * v[e, :, None]) * x[None, None, :])            # [n, K, T]
        A, W, ak = _tensor(a, w)
        s1 = a @ w                                                                             # sum_i w_i a_k(i)
        one = 1.0 if scales else -1.0
        ve[e] = _sum_nodes(W * ab(special.gammaln(A))) + sg * (ab(special.gammaln(a)) @ w).sum(1) + ((s1 + one) * ab(ly[e])).sum(1)
        pA, zA = ab(special.psi(A)), special.zeta(2.0, A)
        for k in range(K):
            g = _sum_nodes(W * ak[k] * pA) + sg * ((a[:, k] * ab(special.psi(a[:, k]))) @ w) + s1[:, k] * ab(ly[e, k])
            h = _sum_nodes(W * ak[k] * ak[k] * zA) + sg * ((a[:, k] ** 2 * special.zeta(2.0, a[:, k])) @ w)
            dm[e, k] = g
            dv[e, k] = 0.5 * (g + h)
    return ve, dm, dv


def var_exp_scale(y, m, v, K):
    """The condition scale S in float64, [N, 1 + 2 K] (a scale needs no more than float64)."""
    ve, dm, dv = var_exp(y, m, v, K, scales=True)
    return np.concatenate([ve[:, None], dm, dv], 1)


def var_exp_full(y, m, v, K):
    """The plain tensor sum of log p and its two derivatives (NOT the contract's form: equal to it up to sum(w) - 1)."""
    K, y, m, v = _rows(y, m, v, K)
    x, w = gh(10)
    ly = np.log(y)
    a = alpha_of(m[:, :, None] + np.sqrt(2.0 * v[:, :, None]) * x[None, None, :])
    A, W, ak = _tensor(a, w)
    lp = special.gammaln(A)
    for k in range(K):
        lp = lp - special.gammaln(ak[k]) + (ak[k] - 1.0) * ly[:, k].reshape([-1] + [1] * K)
    ve = _sum_nodes(W * lp)
    dm, dv = np.zeros_like(m), np.zeros_like(m)
    for k in range(K):
        lk = ly[:, k].reshape([-1] + [1] * K)
        d1 = ak[k] * (special.psi(A) - special.psi(ak[k]) + lk)
        d2 = d1 + ak[k] ** 2 * (special.zeta(2.0, A) - special.zeta(2.0, ak[k]))
        dm[:, k], dv[:, k] = _sum_nodes(W * d1), 0.5 * _sum_nodes(W * d2)
    return ve, dm, dv


def logpdf(y, f):
    """log p(y | f); y [N, K], f [N, K] or [N, S, K]."""
    y, f = np.asarray(y, float), np.asarray(f, float)
    a = alpha_of(f)
    ly = np.log(y) if f.ndim == 2 else np.log(y)[:, None, :]
    return special.gammaln(a.sum(-1)) - special.gammaln(a).sum(-1) + ((a - 1.0) * ly).sum(-1)


def predictive(m, v, K, gh_T=20, chunk=16):
    """mean_k = E[a_k / A], var_k = E[a_k (A - a_k) / (A^2 (A + 1))] + E[(a_k / A)^2] - mean_k^2 under the gh_T^K tensor rule: [N, K] each."""
    K = int(K)
    m, v = np.asarray(m, float).reshape(-1, K), np.asarray(v, float).reshape(-1, K)
    x, w = gh(gh_T)
    mean, var = np.zeros_like(m), np.zeros_like(m)
    for s in range(0, len(m), chunk):
        e = slice(s, min(len(m), s + chunk))
        a = alpha_of(m[e, :, None] + np.sqrt(2.0 * v[e, :, None]) * x[None, None, :])
        A, W, ak = _tensor(a, w)
        den = A * A * (A + 1.0)
        for k in range(K):
            p = ak[k] / A
            mu = _sum_nodes(W * p)
            mean[e, k] = mu
            var[e, k] = _sum_nodes(W * (ak[k] * (A - ak[k]) / den)) + _sum_nodes(W * (p * p)) - mu * mu
    return mean, var


def moments(f):
    """mean and variance of every part at one f: a / A and a (A - a) / (A^2 (A + 1)); f [K] or [N, K]."""
    a = alpha_of(np.asarray(f, float))
    A = a.sum(-1, keepdims=True)
    return a / A, a * (A - a) / (A * A * (A + 1.0))


def samples(F, rng):
    a = alpha_of(np.asarray(F, float))
    g = rng.gamma(a)
    return g / g.sum(-1, keepdims=True)


def log_predictive_rows(y, m, v, num_samples, rng, K):
    """(estimate [N], its standard error [N]) of log E_q[p(y | f)] from `num_samples` draws of f (delta method)."""
    K, y, m, v = _rows(y, m, v, K)
    f = m[:, None, :] + np.sqrt(v)[:, None, :] * rng.randn(len(y), num_samples, K)
    l = logpdf(y, f)
    mx = l.max(1, keepdims=True)
    p = np.exp(l - mx)
    est = mx[:, 0] + np.log(p.mean(1))
    return est, p.std(1, ddof=1) / np.sqrt(num_samples) / p.mean(1)
