"""Float64 NumPy / SciPy restatement of the Ordinal (ordered probit) likelihood of DESIGN 9b, all four building blocks.  The
reference's likelihoods/ordinal.py is a constructor only, so this file restates the project's own contract:

    p(y = k | f) = Phi((b_k - f) / sigma) - Phi((b_{k-1} - f) / sigma),   labels 1..K, b_0 = -inf, b_K = +inf, no clip.

It imports nothing from hetmogp_amd.  Where float64 leaves a choice the algebra differs from the kernel's (csrc/lik_device.h): the
probabilities of `predictive` are differences of SciPy's ndtr taken on the lower side (the kernel sums survival functions), the
tail difference is E(b) - exp(-d) E(a) with np.exp (the kernel splits it around expm1), and the straddling bin goes through
ndtr.  What cannot differ is the stable evaluation itself -- mirror to the lower tail, erfcx with exp(-b^2 / 2) factored out,
log1p of the two tails -- because the plain formula does not survive float64 (log P of a P next to 1 or below DBL_MIN)."""
import numpy as np
from scipy import special

SQRT_2_OVER_PI = np.sqrt(2.0 / np.pi)
INV_SQRT_2PI = 1.0 / np.sqrt(2.0 * np.pi)


def edges_of(K=None, bin_edges=None):
    if bin_edges is None:
        return np.arange(1, int(K), dtype=float) - 0.5 * int(K)
    e = np.asarray(bin_edges, float).reshape(-1)
    assert K is None or len(e) == int(K) - 1
    return e


def cuts(y, edges):
    """labels [N] -> (lower, upper) cut point per row."""
    k = np.asarray(y, float).reshape(-1).astype(int)
    ext = np.concatenate([[-np.inf], edges, [np.inf]])
    return ext[k - 1], ext[k]


def node(a, b, scales=False):
    """a < b arrays (one of the two may be infinite) -> log P, g = (phi(a) - phi(b)) / P, h = (a phi(a) - b phi(b)) / P; with
    `scales` also the sums of the absolute values of the two terms of g and of h."""
    a, b = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float))
    with np.errstate(all="ignore"):
        flip = a + b > 0.0
        a, b = np.where(flip, -b, a), np.where(flip, -a, b)
        sgn = np.where(flip, -1.0, 1.0)
        # the bin straddles f and holds more than half of the mass
        Q = special.ndtr(a) + special.ndtr(-b)
        strad = (b > 0.0) & (Q < 0.5)
        P = 1.0 - Q
        pa, pb = INV_SQRT_2PI * np.exp(-0.5 * a * a), INV_SQRT_2PI * np.exp(-0.5 * b * b)
        apa = np.where(np.isinf(a), 0.0, a * pa)
        bpb = np.where(np.isinf(b), 0.0, b * pb)
        lp1, g1, h1 = np.log1p(-Q), (pa - pb) / P, (apa - bpb) / P
        # everything else: lower tail, exp(-b^2 / 2) factored out
        Ea, Eb = special.erfcx(-a / np.sqrt(2.0)), special.erfcx(-b / np.sqrt(2.0))
        d = 0.5 * (a - b) * (a + b)                           # (a^2 - b^2) / 2 >= 0, +inf for a = -inf
        ed = np.exp(-d)
        D = Eb - ed * Ea
        lp2 = -0.5 * b * b + np.log(0.5 * D)
        g2 = SQRT_2_OVER_PI * np.expm1(-d) / D
        h2 = SQRT_2_OVER_PI * (np.where(np.isinf(a), 0.0, a * ed) - b) / D
        out = (np.where(strad, lp1, lp2), sgn * np.where(strad, g1, g2), np.where(strad, h1, h2))
        if not scales:
            return out
        ra, rb = np.where(strad, pa / P, SQRT_2_OVER_PI * ed / D), np.where(strad, pb / P, SQRT_2_OVER_PI / D)   # phi(a) / P, phi(b) / P
        return out + (ra + rb, np.where(np.isinf(a), 0.0, np.abs(a) * ra) + np.where(np.isinf(b), 0.0, np.abs(b) * rb))


def gh20():
    x, w = np.polynomial.hermite.hermgauss(20)
    return x, w / np.sqrt(np.pi)


def var_exp(y, m, v, K=None, bin_edges=None, sigma=1.0):
    """y [N] labels, m, v [N] or [N, 1] -> ve [N], dm [N, 1], dv [N, 1] (the 20-node rule of the other 1-D families)."""
    e = edges_of(K, bin_edges)
    lo, hi = cuts(y, e)
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    x, w = gh20()
    f = m[:, None] + np.sqrt(2.0 * v)[:, None] * x[None, :]
    lp, g, h = node((lo[:, None] - f) / sigma, (hi[:, None] - f) / sigma)
    d1 = g / sigma
    d2 = h / (sigma * sigma) - d1 * d1
    return lp @ w, (d1 @ w)[:, None], 0.5 * (d2 @ w)[:, None]


def var_exp_scale(y, m, v, K=None, bin_edges=None, sigma=1.0):
    """The condition scale S of tests/ordinal_ref_mp.py in float64, [N, 3] for ve, dm, dv: sum over nodes of weight times the
    absolute values of the addends (a scale needs no more than float64)."""
    lo, hi = cuts(y, edges_of(K, bin_edges))
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    x, w = gh20()
    f = m[:, None] + np.sqrt(2.0 * v)[:, None] * x[None, :]
    lp, g, h, sg, sh = node((lo[:, None] - f) / sigma, (hi[:, None] - f) / sigma, scales=True)
    return np.stack([np.abs(lp) @ w, (sg / sigma) @ w, 0.5 * ((sh / sigma ** 2 + (g / sigma) ** 2) @ w)], 1)


def logpdf(y, f, K=None, bin_edges=None, sigma=1.0):
    """log p(y | f), un-clipped; y, f broadcast against each other."""
    e = edges_of(K, bin_edges)
    y = np.asarray(y, float)
    lo, hi = cuts(y, e)
    lo, hi = lo.reshape(y.shape), hi.reshape(y.shape)
    return node((lo - f) / sigma, (hi - f) / sigma)[0]


def class_probs(m, v, K=None, bin_edges=None, sigma=1.0):
    """P_k(m, v) [N, K], k = 1..K: each difference taken where both values are lower-tail ones."""
    e = edges_of(K, bin_edges)
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    z = (np.concatenate([[-np.inf], e, [np.inf]])[None, :] - m[:, None]) / np.sqrt(sigma * sigma + v)[:, None]
    zl, zu = z[:, :-1], z[:, 1:]
    with np.errstate(invalid="ignore"):
        low = special.ndtr(zu) - special.ndtr(zl)
        up = special.ndtr(-zl) - special.ndtr(-zu)
        return np.where(zl + zu > 0.0, up, low)


def predictive(m, v, K=None, bin_edges=None, sigma=1.0):
    """mean and variance of the label under q(f) = N(m, v): [N, 1] each."""
    P = class_probs(m, v, K, bin_edges, sigma)
    k = np.arange(1, P.shape[1] + 1, dtype=float)
    mean = P @ k
    return mean[:, None], (P @ (k * k) - mean * mean)[:, None]


def log_prob(y, m, v, K=None, bin_edges=None, sigma=1.0):
    """closed form log P_y(m, v) = log of the integral of p(y | f) against N(f; m, v)."""
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    lo, hi = cuts(y, edges_of(K, bin_edges))
    s = np.sqrt(sigma * sigma + v)
    return node((lo - m) / s, (hi - m) / s)[0]


def samples(F, rng, K=None, bin_edges=None, sigma=1.0):
    e = edges_of(K, bin_edges)
    F = np.asarray(F, float).reshape(-1, 1)
    return (1 + (F + sigma * rng.randn(*F.shape) > e[None, :]).sum(1, keepdims=True)).astype(float)


def log_predictive_rows(y, m, v, num_samples, rng, K=None, bin_edges=None, sigma=1.0):
    """(estimate [N], its standard error [N]) of log E_q[p(y | f)] from `num_samples` draws of f (delta method)."""
    y = np.asarray(y, float).reshape(-1)
    m, v = np.asarray(m, float).reshape(-1), np.asarray(v, float).reshape(-1)
    f = m[:, None] + np.sqrt(v)[:, None] * rng.randn(len(y), num_samples)
    l = logpdf(y[:, None] * np.ones_like(f), f, K, bin_edges, sigma)
    mx = l.max(1, keepdims=True)
    p = np.exp(l - mx)
    est = mx[:, 0] + np.log(p.mean(1))
    return est, p.std(1, ddof=1) / np.sqrt(num_samples) / p.mean(1)
