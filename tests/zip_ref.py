"""TEST INFRASTRUCTURE ONLY -- float64 NumPy restatement of the zero-inflated Poisson likelihood of DESIGN 9n, the family's oracle
(registered with oracle.likelihoods_oracle by the fixture of tests/test_zip_gpu.py; `oracle/` itself is not edited).

Counts y = 0, 1, 2, ..: a structural zero with probability pi, else Poisson(lambda).  f0 = log of the rate, lambda = safe_exp(f0)
(Poisson's link); f1 = logit of pi = clip(e^f1 / (1 + e^f1), 1e-9, 1 - 1e-9) (Bernoulli's link and clip, in Bernoulli's expression shapes
ef = safe_exp(f), p = clip(ef / (1 + ef), ..)).  The clip's own derivative is ignored.

  y >= 1   log p = [-lambda + y f0 - lgamma(y+1)] + log(1 - pi)       Poisson's log p in f0 plus Bernoulli's log p of the label 0 in f1
           d/df0 = y - lambda,  d2/df0^2 = -lambda,  d/df1, d2/df1^2 = Bernoulli's d1, d2 at y = 0
  y  = 0   lpi = log pi, l1 = log(1 - pi), u = l1 - lambda - lpi, rho = sigmoid(u), t = lambda rho:
           log p0 = lpi + softplus(u)                                softplus(u) = max(u, 0) + log1p(exp(-|u|))
           d/df0 = -t                  d2/df0^2 = -t + (lambda t) (1 - rho)
           d/df1 = g                   d2/df1^2 = g (rho - pi)       g = pi (1 - pi) (-expm1(-lambda)) exp(-log p0)

Variational expectations (weights w / sqrt(pi) once per dimension; they sum to 1): a row with y >= 1 is the SUM of two 20-node rules,
Poisson's over f0 and Bernoulli's (label 0) over f1; a row with y = 0 is the 20 x 20 tensor rule.

C_ORACLE: the largest |zip_ref - R| / (2^-52 S) over tests/golden/zipgrid.npz, per class (bulk / edge / clip) and per output, no element
left out, rounded up to a power of two; the raw figures and their date are C_ORACLE_RAW below, re-measured by
tests/test_zip_cpu.py::test_float64_restatement_against_high_precision_grid."""
import numpy as np
from scipy import special

LIM_VAL = np.log(np.finfo(np.float64).max)
PLO, PHI = 1e-9, 1.0 - 1e-9


def gh(T=20):
    x, w = np.polynomial.hermite.hermgauss(T)
    return x, w / np.sqrt(np.pi)


def rate(f0):
    return np.exp(np.minimum(f0, LIM_VAL))


def zero_prob(f1):
    """(ef, pi) in Bernoulli's expression shapes."""
    ef = np.exp(np.minimum(f1, LIM_VAL))
    return ef, np.clip(ef / (1.0 + ef), PLO, PHI)


# ---------------------------------------------------------------------------------------------------- log p and its derivatives
def one_minus_pi(f1):
    """1 - pi without the rounding of pi next to 1 (for the condition scale only: the contract's expression is 1.0 - p): 1 / (1 + ef)
    under the same clip; 1 - PHI and 1 - PLO are exact in float64."""
    ef = np.exp(np.minimum(f1, LIM_VAL))
    return np.clip(1.0 / (1.0 + ef), 1.0 - PHI, 1.0 - PLO)


def zero_terms(f0, f1, plain_g=False, for_scale=False):
    """Everything of a y = 0 node: (lpi, sp, lam, rho, rhoc, pi, t, g).  plain_g: g as the difference (1 - rho) - pi (the corruption check)."""
    lam = rate(f0)
    _, p = zero_prob(f1)
    q = one_minus_pi(f1) if for_scale else 1.0 - p
    with np.errstate(all="ignore"):
        lpi, l1 = np.log(p), np.log(q)
        if for_scale:   # log pi without the rounding of pi next to 1, under the same clip
            lpi = np.clip(-np.log1p(np.exp(-np.minimum(f1, LIM_VAL))), np.log(PLO), np.log1p(-(1.0 - PHI)))
        u = l1 - lam - lpi
        e = np.exp(-np.abs(u))
        inv = 1.0 / (1.0 + e)
        sp = np.maximum(u, 0.0) + np.log1p(e)
        rho, rhoc = np.where(u >= 0.0, inv, e * inv), np.where(u >= 0.0, e * inv, inv)
        t = lam * rho
        g = rhoc - p if plain_g else (p * q) * (-np.expm1(-lam)) * np.exp(-(lpi + sp))
    return lpi, sp, lam, rho, rhoc, p, t, g


def logpdf_and_derivatives(y, f0, f1, plain_g=False):
    """(log p, d/df0, d2/df0^2, d/df1, d2/df1^2) at f = (f0, f1), broadcast."""
    y, f0, f1 = np.broadcast_arrays(np.asarray(y, float), np.asarray(f0, float), np.asarray(f1, float))
    lpi, sp, lam, rho, rhoc, p, t, g = zero_terms(f0, f1, plain_g)
    ef, _ = zero_prob(f1)
    with np.errstate(all="ignore"):
        pos = ((-lam + y * f0 - special.gammaln(y + 1.0)) + np.log(1.0 - p), -lam + y, -lam,
               ((0.0 - p) / (1.0 - p)) * (1.0 / (1.0 + ef)), -p / (1.0 + ef))
        zero = (lpi + sp, -t, -t + (lam * t) * rhoc, g, g * (rho - p))
    return tuple(np.where(y > 0.0, a, b) for a, b in zip(pos, zero))


def logpdf(y, F):
    """log p(y | f): y [N], F [N, 2] -> [N]; or F [N, S, 2] -> [N, S]."""
    y, F = np.asarray(y, float).reshape(-1), np.asarray(F, float)
    return logpdf_and_derivatives(y[:, None] if F.ndim == 3 else y, F[..., 0], F[..., 1])[0]


def _rows(y, m, v):
    return np.asarray(y, float).reshape(-1), np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)


def _nodes(m, v, T):
    x, w = gh(T)
    return x[None, :] * np.sqrt(2.0 * v[:, :1]) + m[:, :1], x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:], w


def var_exp(y, m, v, T=20, plain_g=False, tensor=False, **_):
    """y [N] (or [N, 1]), m, v [N, 2] -> ve [N], dm [N, 2], dv [N, 2].  T = 20 is the contract's rule.  tensor: the rows with y >= 1 by the
    T x T tensor rule as well (mathematically the same; the contract is the separable form).  plain_g: the corruption check."""
    y, m, v = _rows(y, m, v)
    f0, f1, w = _nodes(m, v, T)
    # the tensor rule (the contract of the rows with y = 0)
    out = logpdf_and_derivatives(y[:, None, None] if tensor else np.zeros((len(y), 1, 1)), f0[:, :, None], f1[:, None, :], plain_g)
    W = w[:, None] * w[None, :]
    z = [(a * W).sum((1, 2)) for a in out]
    if not tensor:
        # the separable form (the contract of the rows with y >= 1): Poisson's rule over f0, Bernoulli's (label 0) over f1
        yy = y[:, None]
        lam = rate(f0)
        ef, p = zero_prob(f1)
        with np.errstate(all="ignore"):
            s = [((-lam + yy * f0 - special.gammaln(yy + 1.0)) * w).sum(1) + (np.log(1.0 - p) * w).sum(1), ((-lam + yy) * w).sum(1),
                 (-lam * w).sum(1), ((((0.0 - p) / (1.0 - p)) * (1.0 / (1.0 + ef))) * w).sum(1), ((-p / (1.0 + ef)) * w).sum(1)]
        z = [np.where(y > 0.0, a, b) for a, b in zip(s, z)]
    return z[0], np.stack([z[1], z[3]], 1), 0.5 * np.stack([z[2], z[4]], 1)


def var_exp_scale(y, m, v):
    """The condition scale S [N, 5] of (ve, dm_0, dm_1, dv_0, dv_1) in float64: the rule's sum over the ABSOLUTE values of the addends.
    y = 0: lpi and softplus(u) for ve; t; -t and lambda t (1 - rho); g as ONE addend; g (rho - pi) as one addend.  y >= 1: Poisson's
    (-lambda, y f0, -lgamma(y+1); y, -lambda; -lambda) and Bernoulli's at the label 0 (log(1 - p); -p / ((1 - p)(1 + ef)); -p / (1 + ef))."""
    y, m, v = _rows(y, m, v)
    f0, f1, w = _nodes(m, v, 20)
    lpi, sp, lam, rho, rhoc, p, t, g = zero_terms(f0[:, :, None], f1[:, None, :], for_scale=True)
    W = w[:, None] * w[None, :]
    s2 = lambda a: (a * W).sum((1, 2))
    with np.errstate(all="ignore"):
        zero = [s2(np.abs(lpi) + sp), s2(t), s2(g), 0.5 * s2(t + (lam * t) * rhoc), 0.5 * s2(np.abs(g * (rho - p)))]
        yy = y[:, None]
        lam1 = rate(f0)
        ef, p1 = zero_prob(f1)
        q1 = one_minus_pi(f1)
        s1 = lambda a: (a * w).sum(1)
        pos = [s1(lam1 + yy * np.abs(f0) + special.gammaln(yy + 1.0)) + s1(np.abs(np.log(q1))), s1(yy + lam1),
               s1(p1 / (q1 * (1.0 + ef))), 0.5 * s1(lam1), 0.5 * s1(p1 / (1.0 + ef))]
    return np.stack([np.where(y > 0.0, a, b) for a, b in zip(pos, zero)], 1)


# ---------------------------------------------------------------------------------------------------- log predictive density
def _tensor(m, v, T):
    x, w = gh(T)
    i, j = np.divmod(np.arange(T * T), T)
    F = np.stack([m[:, :1] + np.sqrt(2.0 * v[:, :1]) * x[i][None, :], m[:, 1:] + np.sqrt(2.0 * v[:, 1:]) * x[j][None, :]], -1)
    return F, w[i] * w[j]


def lpd(y, m, v, T=20):
    """Deterministic log predictive density of DESIGN 9j, (lpd [N], ess [N]): log sum_nodes W p(y | f_node) over the T x T nodes (every
    row, y >= 1 included: the density does not separate under the logarithm's sum) and the effective number of nodes."""
    y, m, v = _rows(y, m, v)
    F, W = _tensor(m, v, T)
    lp = logpdf(y, F)
    mx = lp.max(1, keepdims=True)
    e = W[None, :] * np.exp(lp - mx)
    s1 = e.sum(1)
    return mx[:, 0] + np.log(s1), s1 * s1 / (e * e).sum(1)


def lpd_scale(y, m, v, T=20):
    """The scale of the lpd's criterion, as tests/binom_ref.py forms it: S = 1 + sum wbar |addends of log p|, wbar the nodes' normalised
    posterior weights W p / sum W p."""
    y, m, v = _rows(y, m, v)
    F, W = _tensor(m, v, T)
    lp = logpdf(y, F)
    e = W[None, :] * np.exp(lp - lp.max(1, keepdims=True))
    lpi, sp, lam, _, _, _, _, _ = zero_terms(F[..., 0], F[..., 1], for_scale=True)
    yy = y[:, None]
    with np.errstate(all="ignore"):
        A = np.where(yy > 0.0, lam + yy * np.abs(F[..., 0]) + special.gammaln(yy + 1.0) + np.abs(np.log(one_minus_pi(F[..., 1]))), np.abs(lpi) + sp)
    return 1.0 + ((e / e.sum(1, keepdims=True)) * A).sum(1)


def lpd_dense(y, m, v, T=120):
    """The integral log E_q[p(y | f)] itself by a T-node-per-dimension rule (T = 150 and 120 agree where the integrand is resolved)."""
    y, m, v = _rows(y, m, v)
    out, chunk = np.empty(len(y)), max(1, int(4e6 // (T * T)))
    for r0 in range(0, len(y), chunk):
        sl = slice(r0, r0 + chunk)
        F, W = _tensor(m[sl], v[sl], T)
        with np.errstate(divide="ignore"):
            out[sl] = special.logsumexp(np.log(W)[None, :] + logpdf(y[sl], F), axis=1)
    return out


def dense(y, m, v, T=120):
    """ve by the T x T tensor rule of every row: the accuracy envelope's yardstick (tools/zip_envelope.py)."""
    return var_exp(y, m, v, T=T, tensor=True)[0]


def envelope_rows(N, seed, vlo=1e-3, vhi=4.0):
    """Seeded rows of the envelopes (the ranges of DESIGN 9j: m in [-3, 3]^2, v log-uniform in [vlo, vhi]; y from the model at a draw
    f ~ q(f))."""
    rng = np.random.RandomState(seed)
    m, v = rng.uniform(-3.0, 3.0, (N, 2)), np.exp(rng.uniform(np.log(vlo), np.log(vhi), (N, 2)))
    f = m + np.sqrt(v) * rng.randn(N, 2)
    return draw(rng, f[:, 0], f[:, 1]), m, v


# ---------------------------------------------------------------------------------------------------- predictive, moments, draws
def predictive(m, v, T=20, **_):
    """Under q(f0) q(f1), pbar = E[pi] by the T-node rule (pi's clip kept, every other clip ignored, overflow is +inf):
    mean = (1 - pbar) exp(m0 + v0/2),  variance = (1 - pbar) (exp(m0 + v0/2) + exp(2 m0 + 2 v0)) - mean^2.  (N, 1) each."""
    m, v = np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    x, w = gh(T)
    pb = (zero_prob(x[None, :] * np.sqrt(2.0 * v[:, 1:]) + m[:, 1:])[1] * w).sum(1)
    with np.errstate(over="ignore", invalid="ignore"):
        e1, e2 = np.exp(m[:, 0] + 0.5 * v[:, 0]), np.exp(2.0 * m[:, 0] + 2.0 * v[:, 0])
        mean = (1.0 - pb) * e1
        a = (1.0 - pb) * (e1 + e2)
        var = np.where(a < np.inf, a - mean * mean, np.inf)
    return mean[:, None], var[:, None]


def moments(f0, f1):
    """Mean, variance and zero share of y given f: (1 - pi) lambda, (1 - pi) lambda (1 + pi lambda), pi + (1 - pi) exp(-lambda)."""
    lam, p = rate(np.asarray(f0, float)), zero_prob(np.asarray(f1, float))[1]
    return (1.0 - p) * lam, (1.0 - p) * lam * (1.0 + p * lam), p + (1.0 - p) * np.exp(-lam)


def draw(rng, f0, f1):
    """Seeded draws y ~ ZIP(lambda(f0), pi(f1)) as floats."""
    f0, f1 = np.broadcast_arrays(np.asarray(f0, float), np.asarray(f1, float))
    zero = rng.rand(*f0.shape) < zero_prob(f1)[1]
    return np.where(zero, 0.0, rng.poisson(rate(f0))).astype(float)


def bulk_rows(rng, N):
    """Seeded bulk rows: m in [-3, 3]^2, v log-uniform in [1e-3, 4], y drawn from the model at the row's own mean parameters."""
    m = rng.uniform(-3.0, 3.0, (N, 2))
    v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, 2)))
    return draw(rng, m[:, 0], m[:, 1]), m, v


# ---------------------------------------------------------------------------------------------------- the grid and its criterion
import contextlib  # noqa: E402
import os  # noqa: E402

GRID = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "zipgrid.npz")
EPS = 2.0 ** -52
BULK, EDGE, CLIP = 0, 1, 2      # CLIP: the designed rows at which some node of f1 reaches 19 in absolute value (tools/make_zip_grid.py)
CLASSES = (BULK, EDGE, CLIP)
CLASS_NAMES = ("bulk", "edge", "clip")
OUTPUTS = ("ve", "dm_0", "dm_1", "dv_0", "dv_1", "lpd")

# raw worst figures of this restatement over the grid (2026-10-20, NumPy / SciPy on the CPU), per class in the order of OUTPUTS (the
# sixth is the 20 x 20 log predictive density against the grid's lpd block, in units of 2^-52 lpd_scale).
#   edge dm_0, dv_0 208: y = 0, f0 = 400, v0 = 1e4 (t = lambda rho of 5e-38: the rounding of f0 = m + sqrt(2 v) x_i at |f0| of several hundred,
#   amplified by |f0| in exp(f0), Poisson's own edge figure);  edge lpd 147: the same rounding on the rows with v0 = 1e4.
#   clip 8.1e7: log(pi), log(1 - pi), 1 / (1 - pi) at a pi rounded within 2e-9 of 1 (f1 = 20): 2^-53 / 2e-9 of the addend, Bernoulli's own
#   2^27; the expression shapes are Bernoulli's on purpose (the tie of the y >= 1 rows), and this is not folded into S.
C_ORACLE_RAW = {
    BULK: (1.627, 3.876, 3.139, 4.475, 3.398, 0.6766),
    EDGE: (4.077, 208.3, 1.91, 208.3, 1.786, 146.9),
    CLIP: (8.094e7, 8.094e7, 8.094e7, 7.323e7, 8.094e7, 2.145e5),
}


def load_grid(path=GRID):
    return np.load(path)


def pack(ve, dm, dv):
    """(ve, dm, dv) -> [N, 5] in the order of OUTPUTS."""
    dm, dv = np.asarray(dm).reshape(-1, 2), np.asarray(dv).reshape(-1, 2)
    return np.stack([np.asarray(ve).reshape(-1), dm[:, 0], dm[:, 1], dv[:, 0], dv[:, 1]], 1)


def ratios(got, R, S):
    """|got - R| / (2^-52 S) per element, formed as (|got - R| / S) / 2^-52 so that a tiny scale does not underflow to a zero bound; 0
    where got == R."""
    d = np.abs(np.asarray(got, float) - R)
    with np.errstate(all="ignore"):
        return np.where(d == 0.0, 0.0, (d / S) / EPS)


def _pow2_up(x):
    """The next power of two (at least 1); a figure within 2 % of a power of two takes the one after it (the margin of DESIGN 9h: NumPy's
    exp / log differ by an ulp between CPU generations)."""
    p = float(2.0 ** np.ceil(np.log2(max(x, 1.0))))
    return 2.0 * p if x > 0.98 * p else p


def c_oracle(cls, out):
    return _pow2_up(C_ORACLE_RAW[int(cls)][out])


def c_kernel(cls, out):
    """The kernels' constants: max(16, 4 C_ORACLE), the rule of DESIGN 9a (wave-shuffle summation order, 1-2 ulp device functions)."""
    return max(16.0, 4.0 * c_oracle(cls, out))


def c_sum(cls, out):
    """Kernel against the float64 restatement instead of R: each sits within its own constant of the true value, so the two add."""
    return c_kernel(cls, out) + c_oracle(cls, out)


def worst(r, cls):
    return {c: tuple(float(x) for x in r[cls == c].max(0)) for c in CLASSES if np.any(cls == c)}


def assert_rows(got, R, S, cls, bound, what, outputs=OUTPUTS[:5]):
    """Every element within bound(class, output) 2^-52 S of R; prints the worst raw figure per class and output first."""
    got = np.asarray(got, float).reshape(len(cls), -1)
    R, S = np.asarray(R, float).reshape(got.shape), np.asarray(S, float).reshape(got.shape)
    assert np.all(np.isfinite(got)), (what, np.argwhere(~np.isfinite(got))[:8])
    r = ratios(got, R, S)
    w = worst(r, cls)
    for c, fig in w.items():
        print("[zipgrid] %-48s %-4s %s" % (what, CLASS_NAMES[c], " ".join("%s %.3g" % (o, x) for o, x in zip(outputs, fig))))
    for c in w:
        for k, name in enumerate(outputs):
            o = OUTPUTS.index(name)
            i = int(np.argmax(np.where(cls == c, r[:, k], -1.0)))
            assert r[i, k] <= bound(c, o), "%s: %s row %d of class %s: %.4g > %g" % (what, name, i, CLASS_NAMES[c], r[i, k], bound(c, o))
    return w


def assert_grid(g, got, bound, what, rows=None):
    idx = np.arange(len(g["y"])) if rows is None else np.asarray(rows)
    return assert_rows(got, g["R"][idx], g["S"][idx], g["cls"][idx], bound, what)


# ---------------------------------------------------------------------------------------------------- the oracle's contract object
class ZIPoissonContract(object):
    """What oracle.likelihoods_oracle._CONTRACT expects of a family: var_exp(Y, m, v, **kwargs of the spec) -> (ve, dm, dv), predictive."""
    var_exp = staticmethod(var_exp)
    predictive = staticmethod(predictive)


@contextlib.contextmanager
def in_the_oracle():
    """Registers the family with oracle.likelihoods_oracle -- contract, id 15 and dim_f = 2 -- and undoes it on exit.  `oracle/` itself is
    not edited."""
    import pytest
    from oracle import likelihoods_oracle as lo
    patch = pytest.MonkeyPatch()
    patch.setitem(lo._CONTRACT, "ZIPoisson", ZIPoissonContract)
    patch.setitem(lo.LIK_IDS, "ZIPoisson", 15)
    dim_f = lo.dim_f
    patch.setattr(lo, "dim_f", lambda name, K=None: 2 if name == "ZIPoisson" else dim_f(name, K))
    try:
        yield
    finally:
        patch.undo()
