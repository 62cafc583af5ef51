"""TEST INFRASTRUCTURE ONLY -- float64 NumPy / SciPy restatement of the Binomial and Beta-Binomial likelihoods of DESIGN 9l, the two
families' oracle (registered with oracle.likelihoods_oracle by the fixture of tests/test_binom_gpu.py; `oracle/` itself is not edited).

A row is (k, n): k successes out of n trials, integers with 1 <= n <= 1e9, 0 <= k <= n, and
lc = lgamma(n+1) - lgamma(k+1) - lgamma(n-k+1), each lgamma on its own.

Binomial, one function, Bernoulli's link and clip p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9), e^f = exp(min(f, LIM_VAL)):

    lp = lc + k log p + (n - k) log(1 - p)      d1 = ((k - n p) / (1 - p)) (1 / (1 + e^f))      d2 = -(n p) / (1 + e^f)

under the 20-node rule, ve = sum w lp, dm = sum w d1, dv = 1/2 sum w d2 (Bernoulli's own expression shapes: the row is n Bernoulli rows
collapsed into one).

Beta-Binomial, two functions, Beta's links and clips a = clip(exp(min(f0, LIM_VAL)), 1e-9, 1e9), b likewise, s = a + b.  With
G(y, r) = lgamma(y+r) - lgamma(r), D1 = psi(y+r) - psi(r), D2 = psi'(y+r) - psi'(r) in the arrangement of negbin_ref.gamma_diffs:

    log p    = lc + G(k, a) + G(n-k, b) - G(n, s)
    d/df0    = a [D1(k, a) - D1(n, s)]            d2/df0^2 = d/df0 + a^2 [D2(k, a) - D2(n, s)]
    d/df1    = b [D1(n-k, b) - D1(n, s)]          d2/df1^2 = d/df1 + b^2 [D2(n-k, b) - D2(n, s)]       (the clips are ignored)

under the 20 x 20 tensor rule, weights w / sqrt(pi) once per dimension.

C_ORACLE: the worst |float64 restatement - 50-digit R| / (2^-52 S) over tests/golden/bngrid.npz per family, class and output, measured
on the CPU on 2026-10-19 (tests/test_binom_cpu.py::test_restatements_agree prints the raw figures) and rounded up to the next power of
two; the kernels get max(16, 4 C_ORACLE), the project's rule."""
import contextlib
import os

import numpy as np
from scipy import special

from negbin_ref import gamma_diffs, plain_diffs  # noqa: F401  (plain_diffs: the corruption check)

LIM_VAL = np.log(np.finfo(np.float64).max)
LO, HI = 1e-9, 1e9
EPS = 2.0 ** -52
OUTPUTS = {"Binomial": ("ve", "dm", "dv"), "BetaBinomial": ("ve", "dm_0", "dm_1", "dv_0", "dv_1")}
DIM_F = {"Binomial": 1, "BetaBinomial": 2}

# raw worst figures of the float64 restatement over the grid (2026-10-19), per (family, class) in the order of OUTPUTS; class 0 bulk, 1 edge
# Binomial, clip, ve: 1.27e8 is log(1 - p) at the lower clip p = 1e-9 on a row with k = 0, n = 1 (m = -25, v = 0).  1 - p is rounded to
# float64 (1.1e-16 absolute) before the logarithm, and the row's whole scale is |log(1 - p)| = 1e-9.  This is Bernoulli's own expression
# shape, which the collapse identity requires; it is not folded into S.  The rows with p at a clip at every node (|m| >= 25) are a class
# of their own, so that the figure does not set the constant of the other edge rows (n = 1e9, v = 0, ...).  Their dm 2.0 and dv 8.0 are
# results of 1e-309 that are off by one subnormal quantum.
C_ORACLE_RAW = {
    ("Binomial", 0): (1.834, 0.7814, 1.959),
    ("Binomial", 1): (1.582, 1.607, 0.9697),
    ("Binomial", 2): (1.274e8, 2.0, 8.0),
    ("BetaBinomial", 0): (0.3582, 0.7382, 0.598, 0.6632, 0.905),
    ("BetaBinomial", 1): (0.784, 1.682, 1.939, 1.71, 2.634),
}


GRID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bngrid.npz")
PREFIX = {"Binomial": "b_", "BetaBinomial": "bb_"}
BULK, EDGE, CLIP = 0, 1, 2      # CLIP: the Binomial's designed rows with p at one of its clips at every node (|m| >= 25)
CLASSES = (BULK, EDGE, CLIP)
CLASS_NAMES = ("bulk", "edge", "clip")


def load_grid(family, path=GRID):
    """The family's arrays of tests/golden/bngrid.npz: y [n, 2], m, v [n, J], cls, R, S [n, 1 + 2 J]."""
    g = np.load(path)
    return {k: g[PREFIX[family] + k] for k in ("y", "m", "v", "cls", "R", "S")}


def ratios(got, R, S):
    """|got - R| / (2^-52 S) per element, formed as (|got - R| / S) / 2^-52 so that a scale in the subnormal range does not underflow to
    a zero bound; 0 where got == R."""
    d = np.abs(np.asarray(got, float) - R)
    with np.errstate(all="ignore"):
        return np.where(d == 0.0, 0.0, (d / S) / EPS)


def worst(family, got, g, rows=None):
    """{class: worst ratio per output} over the grid (or its `rows`)."""
    idx = np.arange(len(g["cls"])) if rows is None else np.asarray(rows)
    r = ratios(got, g["R"][idx], g["S"][idx])
    return {c: tuple(float(x) for x in r[g["cls"][idx] == c].max(0)) for c in CLASSES if np.any(g["cls"][idx] == c)}


def assert_grid(family, got, g, bound, what, rows=None):
    """Every element within bound(family, class, output) 2^-52 S of R; prints the worst raw figure per class and output first."""
    idx = np.arange(len(g["cls"])) if rows is None else np.asarray(rows)
    assert np.all(np.isfinite(got)), (what, np.argwhere(~np.isfinite(got))[:8])
    r = ratios(got, g["R"][idx], g["S"][idx])
    for c, fig in worst(family, got, g, rows).items():
        print("[bngrid] %-44s %-12s %-4s %s" % (what, family, CLASS_NAMES[c], " ".join("%s %.3g" % (o, x) for o, x in zip(OUTPUTS[family], fig))))
    for c in CLASSES:
        for o, name in enumerate(OUTPUTS[family]):
            sel = g["cls"][idx] == c
            if np.any(sel):
                i = int(np.argmax(np.where(sel, r[:, o], -1.0)))
                assert r[i, o] <= bound(family, c, o), "%s: %s %s row %d (y %r m %r v %r): %.4g > %g" % (
                    what, family, name, idx[i], g["y"][idx[i]], g["m"][idx[i]], g["v"][idx[i]], r[i, o], bound(family, c, o))


def _pow2_up(x):
    """The next power of two (at least 1); a figure within 2 % of a power of two takes the one after it, the margin
    tests/test_negbin_cpu.py introduced ("0.988 takes 2"): NumPy's exp / log differ by an ulp between CPU generations, and
    the restatement must stay below its own constant on each of them."""
    p = float(2.0 ** np.ceil(np.log2(max(x, 1.0))))
    return 2.0 * p if x > 0.98 * p else p


def c_oracle(family, cls, out):
    return _pow2_up(C_ORACLE_RAW[(family, int(cls))][out])


def c_kernel(family, cls, out):
    return max(16.0, 4.0 * c_oracle(family, cls, out))


def c_sum(family, cls, out):
    """Kernel against the float64 restatement instead of R: each sits within its own constant of the true value, so the two add."""
    return c_kernel(family, cls, out) + c_oracle(family, cls, out)


def gh(T=20):
    x, w = np.polynomial.hermite.hermgauss(T)
    return x, w / np.sqrt(np.pi)


def log_choose(k, n):
    k, n = np.asarray(k, float), np.asarray(n, float)
    return special.gammaln(n + 1.0) - special.gammaln(k + 1.0) - special.gammaln(n - k + 1.0)


def _kn(y):
    y = np.asarray(y, float).reshape(-1, 2)
    return y[:, 0], y[:, 1]


# ---------------------------------------------------------------------------------------------------- Binomial
def _safe_exp(f):
    return np.exp(np.minimum(f, LIM_VAL))


def prob(f):
    ef = _safe_exp(f)
    return np.clip(ef / (1.0 + ef), LO, 1.0 - LO), ef


def binom_terms(k, n, f):
    """(lp - lc, d1, d2) at f, broadcast."""
    p, ef = prob(f)
    return (k * np.log(p) + (n - k) * np.log(1.0 - p), ((k - n * p) / (1.0 - p)) * (1.0 / (1.0 + ef)), -(n * p) / (1.0 + ef))


def _nodes1(y, m, v, T):
    k, n = _kn(y)
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    x, w = gh(T)
    return k[:, None], n[:, None], x[None, :] * np.sqrt(2.0 * v)[:, None] + m[:, None], w[None, :]


def binom_var_exp(y, m, v, T=20):
    """y [N, 2] = (k, n), m, v [N] -> ve [N], dm [N, 1], dv [N, 1]."""
    k, n, f, w = _nodes1(y, m, v, T)
    lp, d1, d2 = binom_terms(k, n, f)
    return ((lp + log_choose(k, n)) * w).sum(1), (d1 * w).sum(1)[:, None], 0.5 * (d2 * w).sum(1)[:, None]


def binom_scale(y, m, v):
    """S [N, 3] of (ve, dm, dv): the rule's sum over the absolute values of the addends -- ve: the three lgammas of lc each on its own,
    k log p, (n - k) log(1 - p); dm: the two terms of d1; dv: half of d2."""
    k, n, f, w = _nodes1(y, m, v, 20)
    p, ef = prob(f)
    lg = special.gammaln(n + 1.0) + special.gammaln(k + 1.0) + special.gammaln(n - k + 1.0)
    c = 1.0 / ((1.0 - p) * (1.0 + ef))
    # (a scale is free to take log1p: log(1 - p) at p = 1e-9 carries the rounding of 1 - p, 3e-8 of its value)
    return np.stack([((lg + k * np.abs(np.log(p)) + (n - k) * np.abs(np.log1p(-p))) * w).sum(1),
                     ((k * c + n * p * c) * w).sum(1), 0.5 * ((n * p / (1.0 + ef)) * w).sum(1)], 1)


# ---------------------------------------------------------------------------------------------------- Beta-Binomial
def alpha(f):
    return np.clip(_safe_exp(f), LO, HI)


def bb_terms(k, n, a, b, diffs=gamma_diffs):
    """The nine differences at (a, b), broadcast: (Gk, D1k, D2k) of (k, a), (Gn, ..) of (n - k, b), (Gs, ..) of (n, a + b)."""
    return diffs(k, a) + diffs(n - k, b) + diffs(n, a + b)


def bb_logpdf_and_derivatives(k, n, f0, f1, diffs=gamma_diffs):
    """(log p, d/df0, d2/df0^2, d/df1, d2/df1^2) at f = (f0, f1), broadcast."""
    k, n, f0, f1 = np.broadcast_arrays(np.asarray(k, float), np.asarray(n, float), np.asarray(f0, float), np.asarray(f1, float))
    a, b = alpha(f0), alpha(f1)
    Gk, D1k, D2k, Gn, D1n, D2n, Gs, D1s, D2s = bb_terms(k, n, a, b, diffs)
    d0 = a * D1k - a * D1s
    d1 = b * D1n - b * D1s
    return (log_choose(k, n) + Gk + Gn - Gs, d0, d0 + (a * a * D2k - a * a * D2s), d1, d1 + (b * b * D2n - b * b * D2s))


def _nodes2(y, m, v, T):
    k, n = _kn(y)
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = gh(T)
    f0 = (x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])[:, :, None]
    f1 = (x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[:, None, :]
    return k[:, None, None], n[:, None, None], f0, f1, w[:, None] * w[None, :]


def bb_var_exp(y, m, v, diffs=gamma_diffs, T=20):
    """y [N, 2] = (k, n), m, v [N, 2] -> ve [N], dm [N, 2], dv [N, 2].  `diffs` swaps the difference functions (the corruption check)."""
    k, n, f0, f1, W = _nodes2(y, m, v, T)
    lp, d0, h0, d1, h1 = bb_logpdf_and_derivatives(k, n, f0, f1, diffs)
    s = lambda t: (t * W).sum((1, 2))
    return s(lp), np.stack([s(d0), s(d1)], 1), 0.5 * np.stack([s(h0), s(h1)], 1)


def bb_scale(y, m, v):
    """S [N, 5] of (ve, dm_0, dm_1, dv_0, dv_1): the three lgammas of lc, then G(k,a), G(n-k,b), G(n,s); a D1(k,a), a D1(n,s); those plus
    a^2 D2(k,a), a^2 D2(n,s), halved; likewise for f1.  Each difference counts as ONE addend."""
    k, n, f0, f1, W = _nodes2(y, m, v, 20)
    k, n, f0, f1 = np.broadcast_arrays(k, n, f0, f1)
    a, b = alpha(f0), alpha(f1)
    Gk, D1k, D2k, Gn, D1n, D2n, Gs, D1s, D2s = bb_terms(k, n, a, b)
    lg = special.gammaln(n + 1.0) + special.gammaln(k + 1.0) + special.gammaln(n - k + 1.0)
    s = lambda t: (t * W).sum((1, 2))
    g0, g1 = a * D1k + a * D1s, b * D1n + b * D1s
    return np.stack([s(lg + np.abs(Gk) + np.abs(Gn) + np.abs(Gs)), s(g0), s(g1),
                     0.5 * s(g0 + a * a * np.abs(D2k) + a * a * np.abs(D2s)), 0.5 * s(g1 + b * b * np.abs(D2n) + b * b * np.abs(D2s))], 1)


# ---------------------------------------------------------------------------------------------------- both, by name
def var_exp(family, y, m, v, **kw):
    return binom_var_exp(y, m, v, **kw) if family == "Binomial" else bb_var_exp(y, m, v, **kw)


def var_exp_scale(family, y, m, v):
    return binom_scale(y, m, v) if family == "Binomial" else bb_scale(y, m, v)


def stack(ve, dm, dv):
    """(ve, dm, dv) -> [N, 1 + 2 J] in the order of OUTPUTS."""
    return np.hstack([np.asarray(ve).reshape(-1, 1), dm, dv])


def logpdf(family, y, F):
    """log p(y | f): y [N, 2], F [N, J] -> [N]; or F [N, S, J] -> [N, S]."""
    k, n = _kn(y)
    F = np.asarray(F, float)
    if F.ndim == 3:
        k, n = k[:, None], n[:, None]
    if family == "Binomial":
        return binom_terms(k, n, F[..., 0])[0] + log_choose(k, n)
    return bb_logpdf_and_derivatives(k, n, F[..., 0], F[..., 1])[0]


def lpd(family, y, m, v, T=20):
    """Deterministic log predictive density of DESIGN 9j, (lpd [N], ess [N], S [N]): log sum_nodes W p(y | f_node), the effective number of
    nodes, and the criterion's scale S = 1 + sum wbar |addends of log p| (the addends of var_exp_scale)."""
    J = DIM_F[family]
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    x, w = gh(T)
    idx = np.stack(np.meshgrid(*([np.arange(T)] * J), indexing="ij"), -1).reshape(-1, J)
    F = m[:, None, :] + np.sqrt(2.0 * v)[:, None, :] * x[idx][None, :, :]
    W = np.prod(w[idx], 1)
    lp = logpdf(family, y, F)
    k, n = _kn(y)
    k, n = k[:, None], n[:, None]
    lg = special.gammaln(n + 1.0) + special.gammaln(k + 1.0) + special.gammaln(n - k + 1.0)
    if family == "Binomial":
        p, _ = prob(F[..., 0])
        A = lg + k * np.abs(np.log(p)) + (n - k) * np.abs(np.log1p(-p))
    else:
        t = bb_terms(*np.broadcast_arrays(k, n, alpha(F[..., 0]), alpha(F[..., 1])))
        A = lg + np.abs(t[0]) + np.abs(t[3]) + np.abs(t[6])
    mx = lp.max(1, keepdims=True)
    e = W[None, :] * np.exp(lp - mx)
    s1 = e.sum(1)
    return mx[:, 0] + np.log(s1), s1 * s1 / (e * e).sum(1), 1.0 + ((e / s1[:, None]) * A).sum(1)


def lpd_dense(family, y, m, v, T):
    """The integral log E_q[p(y | f)] itself by a T-node-per-dimension rule (T = 150 and 120 agree where the integrand is resolved)."""
    J = DIM_F[family]
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    x, w = gh(T)
    idx = np.stack(np.meshgrid(*([np.arange(T)] * J), indexing="ij"), -1).reshape(-1, J)
    lw = np.log(np.prod(w[idx], 1))[None, :]
    out, chunk = np.empty(len(m)), max(1, int(2e5 // T ** J))
    for r0 in range(0, len(m), chunk):
        sl = slice(r0, r0 + chunk)
        out[sl] = special.logsumexp(lw + logpdf(family, y[sl], m[sl][:, None, :] + np.sqrt(2.0 * v[sl])[:, None, :] * x[idx][None]), axis=1)
    return out


def envelope_rows(family, N, seed):
    """Seeded rows of the log predictive envelope (the ranges of DESIGN 9j: m in [-3, 3], v log-uniform in [1e-3, 4]; n log-uniform in
    1 .. 2000, k from the row's law at a draw f ~ q(f))."""
    rng = np.random.RandomState(seed)
    J = DIM_F[family]
    m, v = rng.uniform(-3.0, 3.0, (N, J)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, J)))
    n = np.floor(np.exp(rng.uniform(0.0, np.log(2001.0), N))).clip(1, 2000)
    return np.stack([draw(rng, family, n, m + np.sqrt(v) * rng.randn(N, J)), n], 1), m, v


# ---------------------------------------------------------------------------------------------------- predictive, moments, draws
def predictive(family, m, v, trials=1, T=20):
    """Mean and variance (N, 1) of a count out of `trials` trials under q(f), by the T-node (T x T) rule:
    Binomial      mean = n* E[p],   var = n* E[p (1 - p)] + n*^2 (E[p^2] - E[p]^2)
    BetaBinomial  mean = n* E[mu],  var = n* E[mu (1 - mu) (s + n*) / (s + 1)] + n*^2 (E[mu^2] - E[mu]^2),  mu = a / s.
    The last term is the variance of p (of mu) under the rule, summed as sum w (p - E[p])^2: the difference of the two moments would
    carry n*^2 2^-52, which is n* 2^-52 of the result."""
    nt = float(trials)
    x, w = gh(T)
    if family == "Binomial":
        m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
        p, _ = prob(x[None, :] * np.sqrt(2.0 * v)[:, None] + m[:, None])
        e1, ev = (p * w).sum(1), (p * (1.0 - p) * w).sum(1)
        vq = ((p - e1[:, None]) ** 2 * w).sum(1)
    else:
        m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
        a = alpha(x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1])[:, :, None]
        b = alpha(x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[:, None, :]
        W = (w[:, None] * w[None, :])[None]
        s = a + b
        mu = a / s
        e1, ev = (mu * W).sum((1, 2)), (mu * (b / s) * ((s + nt) / (s + 1.0)) * W).sum((1, 2))
        vq = ((mu - e1[:, None, None]) ** 2 * W).sum((1, 2))
    return (nt * e1)[:, None], (nt * ev + nt * nt * vq)[:, None]


def moments(family, trials, f):
    """Mean, variance and fourth central moment of a count out of `trials` trials given f (exact: the pmf is summed)."""
    from scipy import stats
    n = int(trials)
    ks = np.arange(n + 1, dtype=float)
    f = np.asarray(f, float).reshape(-1)
    pm = stats.binom.pmf(ks, n, prob(f[0])[0]) if family == "Binomial" else stats.betabinom.pmf(ks, n, alpha(f[0]), alpha(f[1]))
    mean = (ks * pm).sum()
    return mean, ((ks - mean) ** 2 * pm).sum(), ((ks - mean) ** 4 * pm).sum()


def draw(rng, family, n, m):
    """Seeded counts k from the row's own law at the mean parameters m: (N,) for trials n (N,)."""
    n = np.asarray(n).astype(np.int64)
    m = np.asarray(m, float).reshape(len(n), -1)
    p = prob(m[:, 0])[0] if family == "Binomial" else rng.beta(alpha(m[:, 0]), alpha(m[:, 1]))
    return rng.binomial(n, p).astype(float)


def bulk_rows(family, N, seed):
    """Seeded bulk rows of the grid's class: m in [-1.5, 1.5] per dimension, v log-uniform in [1e-3, 0.5], n log-uniform in [1, 2000],
    k from the row's own law.  -> y [N, 2], m, v [N, J]."""
    rng = np.random.RandomState(seed)
    J = DIM_F[family]
    m = rng.uniform(-1.5, 1.5, (N, J))
    v = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, J)))
    n = np.floor(np.exp(rng.uniform(0.0, np.log(2001.0), N))).clip(1, 2000)
    return np.stack([draw(rng, family, n, m), n], 1), m, v


# ---------------------------------------------------------------------------------------------------- the oracle's contract objects
class BinomialContract(object):
    """What oracle.likelihoods_oracle._CONTRACT expects of a family: var_exp(Y, m, v, **kwargs of the spec) -> (ve, dm, dv)."""
    @staticmethod
    def var_exp(Y, m, v, **kw):
        return binom_var_exp(Y, np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1))

    @staticmethod
    def predictive(m, v, pred_trials=1, **kw):
        return predictive("Binomial", m, v, trials=pred_trials)


class BetaBinomialContract(object):
    @staticmethod
    def var_exp(Y, m, v, **kw):
        return bb_var_exp(Y, m, v)

    @staticmethod
    def predictive(m, v, pred_trials=1, **kw):
        return predictive("BetaBinomial", m, v, trials=pred_trials)


@contextlib.contextmanager
def in_the_oracle(others=()):
    """Registers the two contract objects (and `others`: (name, module, id, dim_f)) with oracle.likelihoods_oracle -- contract, id and
    dim_f -- and undoes it on exit.  `oracle/` itself is not edited."""
    import pytest
    from oracle import likelihoods_oracle as lo
    patch = pytest.MonkeyPatch()
    dims = {"Binomial": 1, "BetaBinomial": 2}
    for name, mod, lid, J in (("Binomial", BinomialContract, 13, 1), ("BetaBinomial", BetaBinomialContract, 14, 2)) + tuple(others):
        patch.setitem(lo._CONTRACT, name, mod)
        patch.setitem(lo.LIK_IDS, name, lid)
        dims[name] = J
    dim_f = lo.dim_f
    patch.setattr(lo, "dim_f", lambda name, K=None: dims[name] if name in dims else dim_f(name, K))
    try:
        yield
    finally:
        patch.undo()


def count_rows(rng, family, N, hi=60):
    """(N, 2) rows with n uniform in 1 .. hi and k from a moderate law (p in [0.1, 0.9]; Beta-Binomial: over-dispersed by Beta(2, 3))."""
    n = rng.randint(1, hi + 1, N)
    p = rng.uniform(0.1, 0.9, N) if family == "Binomial" else rng.beta(2.0, 3.0, N)
    return np.stack([rng.binomial(n, p), n], 1).astype(float)


def collapse_pair(seed=91, N=40, hi=6, M=16, Q=2):
    """The two formulations of one data set: a Binomial task of N rows (k, n), n <= hi, and a Bernoulli task holding every row n times
    (k ones, then n - k zeros, at the row's input).  -> (prm, (prob, X, Y) of the Binomial model, (prob, X, Y) of the Bernoulli model,
    sum of lc).  Needs `in_the_oracle`."""
    import model_cases as mc
    from oracle import svmogp_oracle as so
    prm, _, X, _ = mc.family_case(seed, [("Bernoulli", {})], [N], M, Q, 1)
    Yb = count_rows(np.random.RandomState(seed + 2), "Binomial", N, hi)
    k, n = Yb[:, 0].astype(int), Yb[:, 1].astype(int)
    Xr = np.repeat(X[0], n, axis=0)
    Yr = np.concatenate([np.r_[np.ones(a), np.zeros(b - a)] for a, b in zip(k, n)])[:, None]
    return (prm, (so.make_problem([("Binomial", {})], Q, M, 1), X, [Yb]), (so.make_problem([("Bernoulli", {})], Q, M, 1), [Xr], [Yr]),
            float(log_choose(Yb[:, 0], Yb[:, 1]).sum()))


def collapse_differences(a, b, sum_lc):
    """{key: max |a - b| / max |b|} between the Binomial formulation's outputs `a` (its ELBO less sum lc) and the Bernoulli one's `b`."""
    rel = lambda x, y: float(np.max(np.abs(np.asarray(x, float) - np.asarray(y, float))) / (np.max(np.abs(np.asarray(y, float))) + 1e-300))
    d = {k: rel(a[k], b[k]) for k in a if k.startswith("g_")}
    d["elbo"] = rel(np.asarray(a["elbo"], float) - sum_lc, b["elbo"])
    return d
