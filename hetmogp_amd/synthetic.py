"""Synthetic workloads in the style of the reference's demo (notebooks/demo.ipynb cells 1-3, hetmogp/util.py:21-50,
92-103): sorted uniform inputs per task, sinusoid-mixture latent functions mixed by W, observations drawn from each
task's likelihood; inducing inputs on a grid; lengthscale = c * (inducing spacing) so that K_uu stays well
conditioned at large M.  Used by bench.py, smoke() and the size-property tests."""
import numpy as np

_DIM_F = dict(Gaussian=1, Bernoulli=1, HetGaussian=2, Poisson=1, Exponential=1, Gamma=2, Beta=2, Student=2, Ordinal=1,
              NegBinomial=2, Weibull=2, Binomial=1, BetaBinomial=2, ZIPoisson=2)


def _dim_f(name, kw):
    return kw["K"] - 1 if name == "Categorical" else (kw["K"] if name == "Dirichlet" else _DIM_F[name])


def _true_u(rng, x, Q):
    """util.true_u_functions: three-sinusoid mixtures per latent (evaluated on the first input coordinate)."""
    amp = rng.uniform(0.5, 1.5, (Q, 3))
    freq = rng.uniform(1.0, 3.0, (Q, 3))
    shift = 2.0 * rng.rand(Q, 3)
    t = x[:, :1]
    return np.hstack([3 * amp[q, 0] * np.cos(freq[q, 0] * np.pi * t + shift[q, 0] * np.pi)
                      - 2 * amp[q, 1] * np.sin(2 * freq[q, 1] * np.pi * t + shift[q, 1] * np.pi)
                      + amp[q, 2] * np.cos(4 * freq[q, 2] * np.pi * t + shift[q, 2] * np.pi) for q in range(Q)])


def _sample(rng, name, kw, F):
    """The reference's `<likelihood>.samples` link functions, on a damped F so that counts / rates stay moderate."""
    F = 0.3 * F
    n = F.shape[0]
    if name == "Gaussian":
        return F[:, :1] + kw.get("sigma", 0.5) * rng.randn(n, 1)
    if name == "HetGaussian":
        return F[:, :1] + np.exp(0.5 * F[:, 1:2]) * rng.randn(n, 1)
    if name == "Bernoulli":
        return (rng.rand(n, 1) < 1.0 / (1.0 + np.exp(-F[:, :1]))).astype(float)
    if name == "Poisson":
        return rng.poisson(np.exp(np.clip(F[:, :1], -5, 3))).astype(float)
    if name == "Exponential":
        return rng.exponential(np.exp(-np.clip(F[:, :1], -3, 3)))
    if name == "Gamma":
        return rng.gamma(np.exp(np.clip(F[:, :1], -2, 2)), 1.0 / np.exp(np.clip(F[:, 1:2], -2, 2))) + 1e-6
    if name == "Beta":
        return np.clip(rng.beta(np.exp(np.clip(F[:, :1], -2, 2)), np.exp(np.clip(F[:, 1:2], -2, 2))), 1e-6, 1 - 1e-6)
    if name == "Student":
        nu = kw.get("deg_free", 5.0)
        return F[:, :1] + np.exp(0.5 * F[:, 1:2]) * rng.standard_t(nu, (n, 1))
    if name == "NegBinomial":                  # Gamma-Poisson mixture: mean exp(f0), size exp(f1)
        r = np.exp(np.clip(F[:, 1:2], -2, 3))
        return rng.poisson(np.exp(np.clip(F[:, :1], -5, 3)) * rng.gamma(r) / r).astype(float)
    if name == "ZIPoisson":                    # a structural zero with probability sigmoid(f1), else Poisson(exp(f0))
        lam = np.exp(np.clip(F[:, :1], -5, 3))
        zero = rng.rand(n, 1) < 1.0 / (1.0 + np.exp(-np.clip(F[:, 1:2], -3, 3)))
        return np.where(zero, 0.0, rng.poisson(lam)).astype(float)
    if name == "Weibull":                      # (time, event indicator): censored at an independent Weibull censoring time
        return weibull_censored(rng, np.clip(F[:, :1], -3, 3), np.clip(F[:, 1:2], -1, 1.5), kw.get("censored", 0.3))
    if name in ("Binomial", "BetaBinomial"):   # (successes, trials): the trials drawn per row from kw["trials"] = (lo, hi), inclusive
        lo, hi = kw.get("trials", (1, 30))
        return binomial_counts(rng, name, F, lo, hi)
    if name == "Ordinal":                      # labels 1..K drawn from the model; F spread so that every class occurs
        from .engine import ordinal_edges
        edges = ordinal_edges(kw.get("K"), kw.get("bin_edges"))
        f = F[:, :1]
        f = (f - f.mean()) / max(f.std(), 1e-12) * 0.5 * max(edges[-1] - edges[0], 1.0) + 0.5 * (edges[0] + edges[-1])
        z = f + kw.get("sigma", 1.0) * rng.randn(n, 1)
        return (1 + (z > edges[None, :]).sum(1, keepdims=True)).astype(float)
    if name == "Dirichlet":                    # compositions drawn from the model, kept off the boundary and renormalised
        g = np.maximum(rng.gamma(np.exp(np.clip(F[:, :kw["K"]], -2, 2))), 1e-6)
        return g / g.sum(1, keepdims=True)
    if name == "Categorical":
        K = kw["K"]
        e = np.exp(F[:, :K - 1])
        p = np.hstack([e, np.ones((n, 1))]) / (1.0 + e.sum(1, keepdims=True))
        return (1 + (rng.rand(n, 1) > np.cumsum(p, 1)).sum(1, keepdims=True)).astype(float).clip(1, K)
    raise ValueError(name)


def weibull_censored(rng, f0, f1, censored=0.3):
    """(N, 2) rows (y, delta) of a Weibull task: event times t = exp(f0) (-log U)^(1 / k), k = exp(f1), censored at an independent
    censoring time c = s exp(f0) (-log U')^(1 / k): y = min(t, c), delta = 1 where t <= c.  With the same scale function and shape,
    (t / c)^k is a ratio of two unit exponentials times s^-k, so P(censored) = 1 / (1 + s^k) for every row; s is chosen per row to
    make that the stated share `censored` (0 <= censored < 1; 0: no row is censored)."""
    f0, f1 = np.asarray(f0, float).reshape(-1, 1), np.asarray(f1, float).reshape(-1, 1)
    if not 0.0 <= censored < 1.0:
        raise ValueError("censored must lie in [0, 1), got %r" % (censored,))
    ik = 1.0 / np.exp(f1)
    t = np.exp(f0) * (-np.log(1.0 - rng.rand(*f0.shape))) ** ik
    u = -np.log(1.0 - rng.rand(*f0.shape))
    if censored == 0.0:
        return np.hstack([t, np.ones_like(t)])
    c = np.exp(f0) * ((1.0 - censored) / censored * u) ** ik          # s^k = (1 - censored) / censored
    return np.hstack([np.minimum(t, c), (t <= c).astype(float)])


def binomial_counts(rng, name, F, lo=1, hi=30):
    """(N, 2) rows (k, n) of a Binomial or BetaBinomial task: the trial count n of each row is drawn uniformly from the integers
    lo .. hi (1 <= lo <= hi <= 1e9), k from the row's own law -- Binomial(n, sigmoid(f0)), or Binomial(n, p) with
    p ~ Beta(exp f0, exp f1) (f clipped to [-2, 3] so that the draws stay off the ends)."""
    lo, hi = int(lo), int(hi)
    if not 1 <= lo <= hi <= 10 ** 9:
        raise ValueError("trials must satisfy 1 <= lo <= hi <= 1e9, got %r" % ((lo, hi),))
    F = np.asarray(F, float)
    n = rng.randint(lo, hi + 1, (F.shape[0], 1))
    if name == "Binomial":
        p = 1.0 / (1.0 + np.exp(-F[:, :1]))
    else:
        p = rng.beta(np.exp(np.clip(F[:, :1], -2, 3)), np.exp(np.clip(F[:, 1:2], -2, 3)))
    return np.hstack([rng.binomial(n, p).astype(float), n.astype(float)])


def make_case(specs, Ns, M, Q, P=1, seed=0, c=(0.8, 1.0, 1.3, 1.1, 0.9, 1.2, 1.0, 0.85)):
    """Returns (params dict for Engine.elbo_grad, X list, Y list)."""
    rng = np.random.RandomState(seed)
    Df = sum(_dim_f(n, k) for n, k in specs)
    X = [np.sort(rng.rand(n, P), axis=0) if P == 1 else rng.rand(n, P) for n in Ns]
    W = np.where(rng.rand(Q, Df) < 0.5, 1.0, -1.0) * rng.normal(0.5, 0.5, (Q, Df))     # util.random_W_kappas
    Y, d = [], 0
    for (name, kw), x in zip(specs, X):
        J = _dim_f(name, kw)
        Y.append(_sample(rng, name, kw, _true_u(rng, x, Q) @ W[:, d:d + J]))
        d += J
    if P == 1:
        base, h = np.linspace(0, 1, M)[:, None], 1.0 / max(M - 1, 1)
    else:
        g = int(np.ceil(M ** (1.0 / P)))
        base = np.stack(np.meshgrid(*[np.linspace(0, 1, g)] * P, indexing="ij"), -1).reshape(-1, P)[:M]
        h = 1.0 / max(g - 1, 1)
    Z = np.tile(base, (1, Q))                                                          # svmogp.py:52
    r, cc = np.tril_indices(M)
    L = [np.eye(M) + 0.05 / np.sqrt(M) * np.tril(rng.randn(M, M), -1) for _ in range(Q)]
    prm = dict(Z=Z, m_u=2.5 * rng.randn(M, Q) * 0.2, L_flat=np.stack([l[r, cc] for l in L], 1),
               variance=np.full(Q, 0.5), lengthscale=np.array([c[q % len(c)] for q in range(Q)]) * h, W=W,
               kappa=np.zeros((Q, Df)))
    return prm, X, Y
