"""Reference for `hmogp_sample`: the exact law of one draw, the statistics that hold a sampler to it, the designed cases, and a
NumPy uint64 restatement of the device generator (`RowRng` and every `lik_sample` branch of lik_device.h).

Three pieces:
  law(name, f, **kw)        the conditional law of one draw given the row's f (links and clips of `lik_sample`), as a scipy.stats frozen
                            distribution (parameters may be arrays: one law per row) or an explicit pmf
  the statistics            PIT chi-square + Kolmogorov-Smirnov (continuous), chi-square over the law's own quantile bins (discrete),
                            binomial tests (binary outcomes, thresholds of laws whose mass lies below float64's range), lag correlations
  restated_sample(...)      the device algorithm restated on uint64 arrays, vectorised over rows with per-row counters (a rejected row
                            alone advances); `corrupt` names one seeded defect (CORRUPTIONS), for the sharpness tests

run_case(case, draw) runs one designed case through `draw(name, F, seed, **kw)` -- the restatement on the CPU, `engine.sample` on the
device -- and returns {statistic: p-value}.  Every statistic must reach P_MIN; N_STATISTICS counts them (asserted <= MAX_STATISTICS, so
that with fixed seeds a correct sampler fails anywhere with probability <= MAX_STATISTICS * P_MIN = 1e-3)."""
import numpy as np
from scipy import special, stats

N_ROWS = 200000
P_MIN = 1e-6
MAX_STATISTICS = 1000
DBL_MIN = 2.2250738585072014e-308
LIM_VAL = 709.782712893384

# ------------------------------------------------------------------------------------------------ links and clips


def safe_exp(f):
    return np.exp(np.minimum(f, LIM_VAL))


def clip9(x):
    return np.clip(x, 1e-9, 1e9)


def clip_p(x):
    return np.clip(x, 1e-9, 1.0 - 1e-9)


def sigmoid_clipped(f):
    ef = safe_exp(f)
    return clip_p(ef / (1.0 + ef))


def weibull_shape(f1):
    return np.clip(safe_exp(f1), 1e-3, 1e3)


def categorical_pmf(F, K):
    """(N, K): clip each p_k, then renormalise, class K included (the order of `lik_sample`'s Categorical branch)."""
    e = safe_exp(np.asarray(F, float).reshape(-1, K - 1))
    with np.errstate(over="ignore"):     # (two f beyond safe_exp's bound: den = inf, as in float64 on the device and in the reference)
        den = 1.0 + e.sum(1, keepdims=True)
    p = np.hstack([clip_p(e / den), clip_p(1.0 / den)])
    return p / p.sum(1, keepdims=True)


class ZipLaw(object):
    """pi delta_0 + (1 - pi) Poisson(lam), with the cdf / ppf / pmf interface the discrete statistics use."""

    def __init__(self, pi, lam):
        self.pi, self.lam = pi, lam

    def cdf(self, k):
        return np.where(np.asarray(k) < 0, 0.0, self.pi + (1.0 - self.pi) * stats.poisson.cdf(k, self.lam))

    def ppf(self, q):
        return stats.poisson.ppf(np.clip((np.asarray(q) - self.pi) / (1.0 - self.pi), 0.0, 1.0), self.lam)

    def stats(self, moments="mv"):
        m = (1.0 - self.pi) * self.lam
        return m, m * (1.0 + self.pi * self.lam)


def law(name, f, **kw):
    """The exact law of one draw given f (N, J) or (J,).  Continuous and count families: a frozen scipy.stats distribution over the rows;
    Bernoulli: the success probability; Categorical: the (N, K) pmf; Dirichlet: the list of K marginals Beta(a_k, A - a_k)."""
    f = np.asarray(f, float)
    f = f.reshape(1, -1) if f.ndim == 1 else f
    f0 = f[:, 0]
    f1 = f[:, 1] if f.shape[1] > 1 else None
    if name == "Gaussian":
        return stats.norm(f0, kw.get("sigma", 0.5))
    if name == "HetGaussian":
        return stats.norm(f0, np.sqrt(safe_exp(f1)))
    if name == "Student":
        return stats.t(kw.get("deg_free", 5.0), loc=f0, scale=safe_exp(0.5 * f1))
    if name == "Exponential":
        return stats.expon(scale=clip9(safe_exp(-f0)))
    if name == "Gamma":
        return stats.gamma(clip9(safe_exp(f0)), scale=1.0 / clip9(safe_exp(f1)))
    if name == "Beta":
        return stats.beta(clip9(safe_exp(f0)), clip9(safe_exp(f1)))
    if name == "Weibull":
        return stats.weibull_min(weibull_shape(f1), scale=safe_exp(f0))
    if name == "Poisson":
        return stats.poisson(safe_exp(f0))
    if name == "NegBinomial":
        mu, r = safe_exp(f0), clip9(safe_exp(f1))
        return stats.nbinom(r, r / (r + mu))
    if name == "Binomial":
        return stats.binom(int(kw.get("pred_trials", 1)) or 1, sigmoid_clipped(f0))
    if name == "BetaBinomial":
        return stats.betabinom(int(kw.get("pred_trials", 1)) or 1, clip9(safe_exp(f0)), clip9(safe_exp(f1)))
    if name == "ZIPoisson":
        return ZipLaw(sigmoid_clipped(f1), safe_exp(f0))
    if name == "Bernoulli":
        return sigmoid_clipped(f0)
    if name == "Categorical":
        return categorical_pmf(f, int(kw["K"]))
    if name == "Dirichlet":
        a = clip9(safe_exp(f))
        A = a.sum(1)
        return [stats.beta(a[:, k], A - a[:, k]) for k in range(a.shape[1])]
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ statistics
N_STATISTICS = [0]


def _count(p):
    N_STATISTICS[0] += 1
    assert N_STATISTICS[0] <= MAX_STATISTICS, "more than %d statistics: the family-wise level no longer holds" % MAX_STATISTICS
    return float(p)


def pit_tests(u, bins=64):
    """u should be uniform on [0, 1]: chi-square over `bins` equiprobable bins, and Kolmogorov-Smirnov."""
    u = np.asarray(u, float)
    assert np.all((u >= 0.0) & (u <= 1.0)), "a draw outside the law's support (or NaN)"
    cnt = np.bincount(np.minimum((u * bins).astype(np.int64), bins - 1), minlength=bins)
    return {"chi2": _count(stats.chisquare(cnt).pvalue), "ks": _count(stats.kstest(u, "uniform").pvalue)}


def discrete_test(y, dist, levels=32):
    """Chi-square over bins cut at the law's own quantiles, expected counts from cdf differences, neighbours merged until every
    expectation is >= 20.  A law that leaves one bin (all mass on a point at this N) is tested as a binomial count of that point."""
    y = np.asarray(y, float)
    n = y.size
    edges = np.unique(np.asarray(dist.ppf((np.arange(levels - 1) + 1.0) / levels), float))
    edges = edges[np.isfinite(edges)]
    cdf = np.concatenate([[0.0], np.asarray(dist.cdf(edges), float), [1.0]])
    exp = n * np.diff(cdf)
    obs = np.bincount(np.searchsorted(edges, y, side="left"), minlength=edges.size + 1).astype(float)   # bin j: edges[j-1] < y <= edges[j]
    eo, oo = [], []
    ce = co = 0.0
    for e, o in zip(exp, obs):
        ce, co = ce + e, co + o
        if ce >= 20.0:
            eo.append(ce), oo.append(co)
            ce = co = 0.0
    if eo:
        eo[-1] += ce
        oo[-1] += co
    if len(eo) < 2:
        k = int(np.sum(y <= edges[0]))
        return _count(stats.binomtest(k, n, min(float(np.ravel(dist.cdf(edges[0]))[0]), 1.0)).pvalue)
    eo = np.array(eo)
    return _count(stats.chisquare(np.array(oo), eo * (n / eo.sum())).pvalue)


def pmf_test(labels, pmf):
    """Labels 1..K against an explicit pmf: chi-square, classes merged (smallest first) until every expectation is >= 20.  A pmf that
    leaves one class (all mass on a label at this N) is tested as a binomial count of that label, as in `discrete_test`."""
    labels = np.asarray(labels)
    n, K = labels.size, len(pmf)
    assert np.all((labels >= 1) & (labels <= K) & (labels == np.floor(labels))), "a label outside 1..K"
    obs = np.bincount(labels.astype(np.int64) - 1, minlength=K).astype(float)
    exp = n * np.asarray(pmf, float)
    top = int(np.argmax(exp))
    n_top, p_top = obs[top], float(np.asarray(pmf, float)[top])
    order = np.argsort(exp)
    obs, exp = obs[order], exp[order]
    while exp.size > 1 and exp[0] < 20.0:
        exp = np.concatenate([[exp[0] + exp[1]], exp[2:]])
        obs = np.concatenate([[obs[0] + obs[1]], obs[2:]])
        o2 = np.argsort(exp)
        obs, exp = obs[o2], exp[o2]
    if exp.size < 2:
        return binom_test(n_top, n, p_top)
    return _count(stats.chisquare(obs, exp * (n / exp.sum())).pvalue)


def binom_test(k, n, p):
    return _count(stats.binomtest(int(k), int(n), float(min(max(p, 0.0), 1.0))).pvalue)


def lag_test(a, b):
    """|r| sqrt(N) of the correlation of a with b against the normal law.  Perfect dependence (no spread left) is p = 0."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.std() < 1e-9 or b.std() < 1e-9:
        return _count(0.0)
    r = np.corrcoef(a, b)[0, 1]
    return _count(2.0 * stats.norm.sf(abs(r) * np.sqrt(a.size)))


# ------------------------------------------------------------------------------------------------ the generator, restated
U64 = np.uint64
_GOLD, _M1, _M2, _ROWMUL = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB), U64(0xD1342543DE82EF95)

CORRUPTIONS = ("boost_exponent", "squeeze_always", "ptrs_fast_accept", "inversion_from_one", "no_reflection", "normal_one_counter",
               "key_ignores_row", "student_gamma_nu", "categorical_no_renorm")


def splitmix64(x):
    x = x + _GOLD
    x = (x ^ (x >> U64(30))) * _M1
    x = (x ^ (x >> U64(27))) * _M2
    return x ^ (x >> U64(31))


class RowRng(object):
    """`RowRng` of lik_device.h for rows 0..N-1 at once.  Every method takes the index array of the rows that draw (their counters alone
    advance) and the parameters of those rows."""

    def __init__(self, seed, N, corrupt=None):
        assert corrupt is None or corrupt in CORRUPTIONS
        self.corrupt = corrupt
        rows = np.arange(N, dtype=U64)
        if corrupt == "key_ignores_row":
            rows = rows * U64(0)
        self.key = splitmix64(np.full(N, int(seed) & (2 ** 64 - 1), dtype=U64) ^ rows * _ROWMUL)
        self.ctr = np.zeros(N, dtype=U64)

    def uniform(self, idx):
        self.ctr[idx] += U64(1)
        h = splitmix64(self.key[idx] ^ self.ctr[idx] * _GOLD)
        return ((h >> U64(11)).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)

    def normal(self, idx):
        u1 = self.uniform(idx)
        u2 = u1 if self.corrupt == "normal_one_counter" else self.uniform(idx)
        return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)

    def gamma(self, idx, a):
        a = np.array(a, float)
        boost = np.ones(idx.size)
        lt = a < 1.0
        if lt.any():
            expo = 1.0 / (a[lt] + 1.0) if self.corrupt == "boost_exponent" else 1.0 / a[lt]
            boost[lt] = np.power(self.uniform(idx[lt]), expo)
            a[lt] += 1.0
        d = a - 1.0 / 3.0
        c = 1.0 / np.sqrt(9.0 * d)
        out = boost * d
        act = np.arange(idx.size)
        for _ in range(1000):
            if act.size == 0:
                break
            x = self.normal(idx[act])
            t = 1.0 + c[act] * x
            pos = t > 0.0
            ap, xp, tp = act[pos], x[pos], t[pos]
            vv = tp * tp * tp
            u = self.uniform(idx[ap])
            with np.errstate(divide="ignore"):
                acc = (u < 1.0 - 0.0331 * (xp * xp) * (xp * xp)) | (np.log(u) < 0.5 * xp * xp + d[ap] * (1.0 - vv + np.log(vv)))
            if self.corrupt == "squeeze_always":
                acc = np.ones_like(acc)
            out[ap[acc]] = boost[ap[acc]] * d[ap[acc]] * vv[acc]
            keep = np.ones(act.size, bool)
            keep[np.flatnonzero(pos)[acc]] = False
            act = act[keep]
        return out

    def poisson(self, idx, lam):
        lam = np.array(lam, float)
        out = np.zeros(idx.size)
        small = (lam > 0.0) & (lam < 10.0)
        if small.any():
            s = np.flatnonzero(small)
            L = np.exp(-lam[s])
            k = np.full(s.size, 1.0 if self.corrupt == "inversion_from_one" else 0.0)
            p = self.uniform(idx[s])
            act = np.flatnonzero(p > L)
            while act.size:
                k[act] += 1.0
                p[act] *= self.uniform(idx[s[act]])
                act = act[p[act] > L[act]]
            out[s] = k
        huge = lam > 1e15
        out[huge] = lam[huge]
        big = (lam >= 10.0) & ~huge
        if big.any():
            s = np.flatnonzero(big)
            lm = lam[s]
            slam, loglam = np.sqrt(lm), np.log(lm)
            b = 0.931 + 2.53 * slam
            a = -0.059 + 0.02483 * b
            invalpha = 1.1239 + 1.1328 / (b - 3.4)
            vr = (0.99 if self.corrupt == "ptrs_fast_accept" else 0.9277) - 3.6224 / (b - 2.0)
            res = np.floor(lm)
            act = np.arange(s.size)
            for _ in range(1000):
                if act.size == 0:
                    break
                U = self.uniform(idx[s[act]]) - 0.5
                V = self.uniform(idx[s[act]])
                us = 0.5 - np.abs(U)
                k = np.floor((2.0 * a[act] / us + b[act]) * U + lm[act] + 0.43)
                fast = (us >= 0.07) & (V <= vr[act])
                rej = ~fast & ((k < 0.0) | ((us < 0.013) & (V > us)))
                with np.errstate(invalid="ignore", divide="ignore"):
                    slow = (np.log(V) + np.log(invalpha[act]) - np.log(a[act] / (us * us) + b[act]) <=
                            -lm[act] + k * loglam[act] - special.gammaln(np.where(k >= 0.0, k, 0.0) + 1.0))
                acc = fast | (~rej & slow)
                res[act[acc]] = k[acc]
                act = act[~acc]
            out[s] = res
        return out

    def binomial(self, idx, n, p):
        n, p = np.broadcast_to(np.asarray(n, float), idx.shape).copy(), np.array(p, float)
        out = np.zeros(idx.size)
        out[~(p < 1.0)] = n[~(p < 1.0)]
        live = (p > 0.0) & (p < 1.0)
        flip = live & (p > 0.5)
        q = np.where(flip, 1.0 - p, p)
        inv = live & (n * q < 10.0)
        if inv.any():
            s = np.flatnonzero(inv)
            ns, qs = n[s], q[s]
            r = qs / (1.0 - qs)
            pk = np.exp(ns * np.log1p(-qs))
            u = self.uniform(idx[s])
            k = np.full(s.size, 1.0 if self.corrupt == "inversion_from_one" else 0.0)
            act = np.arange(s.size)
            for _ in range(256):
                act = act[~((u[act] <= pk[act]) | (k[act] >= ns[act]))]
                if act.size == 0:
                    break
                u[act] -= pk[act]
                pk[act] *= r[act] * ((ns[act] - k[act]) / (k[act] + 1.0))
                k[act] += 1.0
            out[s] = k
        btrs = live & ~inv
        if btrs.any():
            s = np.flatnonzero(btrs)
            ns, qs = n[s], q[s]
            spq = np.sqrt(ns * qs * (1.0 - qs))
            b = 1.15 + 2.53 * spq
            a = -0.0873 + 0.0248 * b + 0.01 * qs
            c = ns * qs + 0.5
            vr = 0.92 - 4.2 / b
            alpha = (2.83 + 5.1 / b) * spq
            lr = np.log(qs / (1.0 - qs))
            md = np.floor((ns + 1.0) * qs)
            h = special.gammaln(md + 1.0) + special.gammaln(ns - md + 1.0)
            k = np.floor(ns * qs)
            act = np.arange(s.size)
            for _ in range(1000):
                if act.size == 0:
                    break
                U = self.uniform(idx[s[act]]) - 0.5
                V = self.uniform(idx[s[act]])
                us = 0.5 - np.abs(U)
                kk = np.floor((2.0 * a[act] / us + b[act]) * U + c[act])
                ok = ~((kk < 0.0) | (kk > ns[act]))
                kc = np.where(ok, kk, 0.0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    acc = ok & (((us >= 0.07) & (V <= vr[act])) |
                                (np.log(V * alpha[act] / (a[act] / (us * us) + b[act])) <=
                                 h[act] - special.gammaln(kc + 1.0) - special.gammaln(ns[act] - kc + 1.0) + (kc - md[act]) * lr[act]))
                k[act[acc]] = kk[acc]
                act = act[~acc]
            out[s] = k
        if self.corrupt != "no_reflection":
            out[flip] = n[flip] - out[flip]
        return out


def restated_sample(name, F, seed=0, corrupt=None, **kw):
    """`hmogp_sample` restated: (N, 1), (N, K) for Dirichlet.  The draws equal the device's except where an ulp of the device libm flips
    a comparison."""
    J = {"Categorical": lambda: int(kw["K"]) - 1, "Dirichlet": lambda: int(kw["K"])}.get(
        name, lambda: dict(Gaussian=1, Bernoulli=1, HetGaussian=2, Poisson=1, Exponential=1, Gamma=2, Beta=2, Student=2, Ordinal=1,
                           NegBinomial=2, Weibull=2, Binomial=1, BetaBinomial=2, ZIPoisson=2)[name])()
    F = np.asarray(F, float).reshape(-1, J)
    N = F.shape[0]
    g = RowRng(seed, N, corrupt)
    al = np.arange(N)
    f0 = F[:, 0]
    f1 = F[:, 1] if J > 1 else None
    with np.errstate(over="ignore", under="ignore"):
        if name == "Gaussian":
            y = f0 + kw.get("sigma", 0.5) * g.normal(al)
        elif name == "Bernoulli":
            y = (g.uniform(al) < sigmoid_clipped(f0)).astype(float)
        elif name == "HetGaussian":
            y = f0 + np.sqrt(safe_exp(f1)) * g.normal(al)
        elif name == "Poisson":
            y = g.poisson(al, safe_exp(f0))
        elif name == "Exponential":
            y = -clip9(safe_exp(-f0)) * np.log(g.uniform(al))
        elif name == "Gamma":
            y = g.gamma(al, clip9(safe_exp(f0))) / clip9(safe_exp(f1))
        elif name == "Beta":
            a, b = clip9(safe_exp(f0)), clip9(safe_exp(f1))
            x = g.gamma(al, a)
            yv = g.gamma(al, b)
            y = np.empty(N)
            ok = x + yv > 0.0
            y[ok] = x[ok] / (x[ok] + yv[ok])
            z = np.flatnonzero(~ok)
            y[z] = (g.uniform(z) * (a[z] + b[z]) < a[z]).astype(float)
        elif name == "Student":
            nu = float(kw.get("deg_free", 5.0))
            z = g.normal(al)
            G = g.gamma(al, np.full(N, nu if corrupt == "student_gamma_nu" else 0.5 * nu))
            with np.errstate(divide="ignore"):
                y = f0 + safe_exp(0.5 * f1) * z * np.sqrt(nu / (2.0 * G))
        elif name == "NegBinomial":
            r = clip9(safe_exp(f1))
            y = g.poisson(al, safe_exp(f0) * g.gamma(al, r) / r)
        elif name == "Weibull":
            with np.errstate(divide="ignore"):
                y = safe_exp(f0) * np.power(-np.log(g.uniform(al)), 1.0 / weibull_shape(f1))
        elif name == "Binomial":
            y = g.binomial(al, float(int(kw.get("pred_trials", 1)) or 1), sigmoid_clipped(f0))
        elif name == "BetaBinomial":
            a, b = clip9(safe_exp(f0)), clip9(safe_exp(f1))
            x = g.gamma(al, a)
            yv = g.gamma(al, b)
            p = np.empty(N)
            ok = x + yv > 0.0
            p[ok] = x[ok] / (x[ok] + yv[ok])
            z = np.flatnonzero(~ok)
            p[z] = (g.uniform(z) * (a[z] + b[z]) < a[z]).astype(float)
            y = g.binomial(al, float(int(kw.get("pred_trials", 1)) or 1), p)
        elif name == "ZIPoisson":
            zero = g.uniform(al) < sigmoid_clipped(f1)
            y = np.zeros(N)
            nz = np.flatnonzero(~zero)
            y[nz] = g.poisson(nz, safe_exp(f0[nz]))
        elif name == "Categorical":
            K = int(kw["K"])
            e = safe_exp(F)
            den = 1.0 + _sum_in_order(e)
            e = clip_p(e / den[:, None])
            psum = clip_p(1.0 / den)
            for k in range(K - 1):
                psum = psum + e[:, k]
            u = g.uniform(al) * (1.0 if corrupt == "categorical_no_renorm" else psum)
            y = np.full(N, float(K))
            cum = np.zeros(N)
            found = np.zeros(N, bool)
            for k in range(K - 1):
                cum = cum + e[:, k]
                hit = ~found & (u < cum)
                y[hit] = k + 1.0
                found |= hit
        elif name == "Ordinal":
            edges = np.asarray(kw["bin_edges"], float) if kw.get("bin_edges") is not None else np.arange(1, int(kw["K"]), dtype=float) - 0.5 * int(kw["K"])
            z = f0 + float(kw.get("sigma", 1.0)) * g.normal(al)
            y = 1.0 + (z[:, None] > edges[None, :]).sum(1)
        elif name == "Dirichlet":
            K = int(kw["K"])
            a = clip9(safe_exp(F))
            x = np.stack([g.gamma(al, a[:, k]) for k in range(K)], 1)
            A, s = _sum_in_order(a), _sum_in_order(x)
            y = np.zeros((N, K))
            ok = s > 0.0
            y[ok] = x[ok] / s[ok, None]
            z = np.flatnonzero(~ok)
            u = g.uniform(z) * A[z]
            cum = np.zeros(z.size)
            found = np.zeros(z.size, bool)
            for k in range(K):
                cum = cum + a[z, k]
                hit = ~found & ((u < cum) | (k == K - 1))
                y[z[hit], k] = 1.0
                found |= hit
            return y
        else:
            raise KeyError(name)
    return y.reshape(N, 1)


def _sum_in_order(x):
    s = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        s = s + x[:, k]
    return s


# ------------------------------------------------------------------------------------------------ the designed cases
def _groups(rows, n=N_ROWS):
    """n rows in len(rows) equal groups of constant f: F (n, J) and the list of index arrays."""
    rows = np.asarray(rows, float)
    gid = np.arange(n) % len(rows)
    return rows[gid], [np.flatnonzero(gid == g) for g in range(len(rows))]


def _logit(p):
    return float(np.log(p) - np.log1p(-p))


def _case(cid, name, kind, seed, kw=None, **more):
    d = dict(id=cid, name=name, kind=kind, seed=seed, kw=kw or {})
    d.update(more)
    return d


def cases():
    """Every designed case of the issue: id, family, kwargs, seed, F (built from the case's own fixed seed) and the kind of statistic.
      pit     f varies per row; PIT chi-square + KS (Dirichlet: of every marginal); lag=True adds the two lag correlations
      thresh  groups of constant f, law with mass below float64's range: binomial counts of draws <= x_j
      disc    groups of constant f: chi-square over the law's quantile bins (randomised PIT for the lag statistics)
      binary  groups of constant f: binomial test of the share of ones
      pmf     groups of constant f: labels against the explicit pmf
      vertex  groups of constant f, every Dirichlet shape tiny: the vertex frequencies against a_k / A"""
    out = []
    L = np.log
    for i, sg in enumerate((1e-3, 0.7, 50.0)):
        rng = np.random.RandomState(100 + i)
        out.append(_case("gaussian_sigma_%g" % sg, "Gaussian", "pit", 1000 + i, {"sigma": sg}, F=rng.uniform(-3, 3, (N_ROWS, 1)), lag=(sg == 0.7)))
    rng = np.random.RandomState(110)
    out.append(_case("hetgaussian", "HetGaussian", "pit", 1010, F=np.column_stack([rng.uniform(-3, 3, N_ROWS), rng.uniform(-20, 20, N_ROWS)])))
    for i, nu in enumerate((0.5, 1.0, 2.5, 5.0, 30.0, 1e3)):
        rng = np.random.RandomState(120 + i)
        out.append(_case("student_nu_%g" % nu, "Student", "pit", 1020 + i, {"deg_free": nu},
                         F=np.column_stack([rng.uniform(-3, 3, N_ROWS), rng.uniform(-6, 6, N_ROWS)])))
    rng = np.random.RandomState(130)
    out.append(_case("exponential", "Exponential", "pit", 1030, F=rng.uniform(-25, 25, (N_ROWS, 1))))
    rng = np.random.RandomState(140)   # half the rows at a in [0.02, 20] (boost, a low acceptance rate), half up to beyond the 1e9 clip
    f0 = np.where(np.arange(N_ROWS) % 2 == 0, rng.uniform(L(0.02), L(20.0), N_ROWS), rng.uniform(L(20.0), 22.0, N_ROWS))
    out.append(_case("gamma", "Gamma", "pit", 1040, F=np.column_stack([f0, rng.uniform(-25, 25, N_ROWS)]), lag=True))
    rng = np.random.RandomState(141)   # shapes with no boost in front and the lowest acceptance rate: where the squeeze and the exact test decide
    out.append(_case("gamma_shape_1_4", "Gamma", "pit", 1041, F=np.column_stack([rng.uniform(0.0, L(4.0), N_ROWS), rng.uniform(-2, 2, N_ROWS)])))
    rng = np.random.RandomState(150)   # b >= 0.5: below it a share (2^-53)^b of the law lies between 1 and the double next to it, where a
    # draw has no PIT of its own (0 has doubles all the way down, 1 has not); b in [0.02, 0.5] is the threshold case beta_small_b
    out.append(_case("beta", "Beta", "pit", 1050, F=np.column_stack([rng.uniform(L(0.02), L(1e4), N_ROWS), rng.uniform(L(0.5), L(1e4), N_ROWS)])))
    rng = np.random.RandomState(160)   # shape from 0.02 (below it the draw leaves float64's range: weibull_tiny) to beyond the 1e3 clip
    out.append(_case("weibull", "Weibull", "pit", 1060, F=np.column_stack([rng.uniform(-2, 2, N_ROWS), rng.uniform(L(0.02), 9.0, N_ROWS)])))
    for i, K in enumerate((2, 3, 4)):   # (every K the library builds: HMOGP_DIRICHLET_MAXK = 4)
        rng = np.random.RandomState(170 + i)
        # (A - a_k >= 0.5 for every k, for the reason given at the Beta case)
        out.append(_case("dirichlet_K%d" % K, "Dirichlet", "pit", 1070 + i, {"K": K}, F=rng.uniform(L(0.5 if K == 2 else 0.25), L(50.0), (N_ROWS, K))))
    # laws with mass below float64's range
    F, grp = _groups([[L(0.01), 0.0], [L(1e-3), 0.0], [L(1e-3), 25.0], [L(1e-5), -25.0], [L(1e-7), 1.0], [-25.0, 0.0]])
    out.append(_case("gamma_tiny", "Gamma", "thresh", 1080, F=F, groups=grp))
    F, grp = _groups([[0.0, -9.0], [1.0, -6.0], [-1.0, -4.5]])
    out.append(_case("weibull_tiny", "Weibull", "thresh", 1081, F=F, groups=grp))
    F, grp = _groups([[-5.0, -5.0], [-7.0, -7.0], [-7.0, -9.0], [-12.0, -10.0], [-25.0, -25.0], [-25.0, -21.0], [-1.5, -1.5]])
    out.append(_case("beta_tiny", "Beta", "thresh", 1082, F=F, groups=grp))
    F, grp = _groups([[L(0.02), L(0.02)], [L(5.0), L(0.02)], [L(1e4), L(0.05)], [L(0.3), L(0.2)], [L(50.0), L(0.3)], [L(0.02), L(0.45)]])
    out.append(_case("beta_small_b", "Beta", "thresh", 1086, F=F, groups=grp, xs=[1e-3, 0.1, 0.5, 0.9, 0.99, 1.0 - 1e-3]))
    for i, K in enumerate((2, 3, 4)):
        rows = [[-14.0 - 0.7 * k for k in range(K)], [-25.0] * K, [-25.0] + [-21.0] * (K - 1)]
        F, grp = _groups(rows)
        out.append(_case("dirichlet_tiny_K%d" % K, "Dirichlet", "vertex", 1083 + i, {"K": K}, F=F, groups=grp))
    # discrete families
    F, grp = _groups([[L(lam)] for lam in (1e-3, 0.5, 9.99, 10.01, 33.0, 403.0, 1e5, 1e9)] + [[36.5]])
    out.append(_case("poisson", "Poisson", "disc", 1090, F=F, groups=grp, exact_last=True, lag=True))
    F, grp = _groups([[L(1e5)]])   # every row at one large rate: PTRS's acceptance bounds move the law by 5e-4 per draw in chi-square terms
    out.append(_case("poisson_ptrs", "Poisson", "disc", 1089, F=F, groups=grp))
    F, grp = _groups([[L(mu), L(r)] for r in (0.05, 0.5, 1.0, 7.4, 1e3) for mu in (0.2, 5.0, 200.0)])
    out.append(_case("negbinomial", "NegBinomial", "disc", 1091, F=F, groups=grp))
    for i, (n, ps) in enumerate(((1, (0.3, 0.7)), (7, (0.3, 0.7)), (1000, (0.3, 0.7, 0.00999, 0.01001, 0.99001, 0.98999)), (1000000, (1e-6, 0.4)))):
        rows = [[_logit(p)] for p in ps] + ([[-25.0], [25.0]] if n == 1000 else [])
        F, grp = _groups(rows)
        out.append(_case("binomial_n%d" % n, "Binomial", "disc", 1092 + i, {"pred_trials": n}, F=F, groups=grp))
    for i, n in enumerate((1, 20, 500)):
        F, grp = _groups([[L(2.0), L(3.0)], [L(0.5), L(0.5)], [L(1e-4), L(2e-4)], [-25.0, -25.0]])
        out.append(_case("betabinomial_n%d" % n, "BetaBinomial", "disc", 1096 + i, {"pred_trials": n}, F=F, groups=grp))
    F, grp = _groups([[L(lam), f1] for lam in (2.0, 50.0) for f1 in (-25.0, -1.0, 1.0, 25.0)])
    out.append(_case("zipoisson", "ZIPoisson", "disc", 1099, F=F, groups=grp))
    F, grp = _groups([[-25.0], [-3.0], [0.0], [3.0], [25.0]])
    out.append(_case("bernoulli", "Bernoulli", "binary", 1100, F=F, groups=grp))
    for i, K in enumerate((2, 3, 4, 5, 6)):
        rng = np.random.RandomState(180 + i)
        hot = [0.0] * (K - 1)
        hot[0] = 30.0
        F, grp = _groups([list(rng.uniform(-1.5, 1.5, K - 1)), hot, [-30.0] * (K - 1)])
        out.append(_case("categorical_K%d" % K, "Categorical", "pmf", 1101 + i, {"K": K}, F=F, groups=grp))
    # Two f beyond safe_exp's bound: 1 + sum_k exp(f_k) overflows, every e_k / den and 1 / den is 0 and is clipped to 1e-9, so the K clipped
    # probabilities sum to K 1e-9 and the renormalisation alone makes the draw what float64 (and the reference's NumPy) makes of this row:
    # uniform over the K classes.  The only rows at which the renormalisation moves the law by more than (K - 1) 1e-9.
    for i, K in enumerate((3, 4, 6)):
        F, grp = _groups([[750.0, 750.0] + [0.0] * (K - 3), [750.0] * (K - 1)])
        out.append(_case("categorical_den_overflow_K%d" % K, "Categorical", "pmf", 1106 + i, {"K": K}, F=F, groups=grp))
    return out


def _is_normal(x):
    return np.isfinite(x) and abs(x) >= DBL_MIN


def run_case(case, draw):
    """The statistics of one designed case over the draws of `draw(name, F, seed, **kw)`: {statistic: p-value}.  Properties that are no
    statistics (support, finiteness, rows summing to 1, lambda > 1e15 returned as it is) are asserted on the way."""
    name, kw, F, seed, kind = case["name"], case["kw"], case["F"], case["seed"], case["kind"]
    y = np.asarray(draw(name, F, seed, **kw), float)
    assert y.shape == (F.shape[0], int(kw["K"]) if name == "Dirichlet" else 1) and not np.any(np.isnan(y)), (case["id"], "shape or NaN")
    p = {}
    if kind == "pit":
        if name == "Dirichlet":
            assert np.all((y >= 0.0) & (y <= 1.0))
            assert np.all(np.abs(y.sum(1) - 1.0) <= 4 * 2.0 ** -52), (case["id"], "a row does not sum to 1 within 4 ulp")
            for k, lw in enumerate(law(name, F, **kw)):
                for s, v in pit_tests(lw.cdf(y[:, k])).items():
                    p["%s[%d]" % (s, k)] = v
            return p
        lw = law(name, F, **kw)
        u = lw.cdf(y[:, 0])
        p.update(pit_tests(u))
        if case.get("lag"):
            p["lag_rows"] = lag_test(u[:-1], u[1:])
            u2 = lw.cdf(np.asarray(draw(name, F, seed + 1, **kw), float)[:, 0])
            p["lag_seeds"] = lag_test(u, u2)
        return p
    y = y if name == "Dirichlet" else y[:, 0]
    for gi, idx in enumerate(case["groups"]):
        f, yg = F[idx[0]], y[idx]
        tag = "g%d" % gi
        if kind == "thresh":
            lw = law(name, f, **kw)
            with np.errstate(over="ignore"):
                qs = np.ravel(lw.ppf([0.5, 0.9, 0.99]))
            if name == "Beta":     # the ratio of two underflowing variates keeps only its side of 1/2: thresholds in the middle
                assert np.all(np.isfinite(yg) & (yg >= 0.0) & (yg <= 1.0)), (case["id"], gi, "a draw outside [0, 1]")
                xs = case.get("xs") or [0.5] + [float(q) for q in qs if 1e-3 <= q <= 1.0 - 1e-3 and q != 0.5]
            else:
                assert np.all(yg >= 0.0), (case["id"], gi, "a negative draw")
                if name == "Gamma":
                    assert np.all(np.isfinite(yg)), (case["id"], gi, "a draw that is not finite")
                xs = [DBL_MIN] + [float(q) for q in qs if _is_normal(q)]
            for j, x in enumerate(xs):
                p["%s_le_%.3g" % (tag, x)] = binom_test(np.sum(yg <= x), yg.size, float(np.ravel(lw.cdf(x))[0]))
        elif kind == "vertex":
            a = clip9(safe_exp(f))
            assert np.all(np.isfinite(yg) & (yg >= 0.0) & (yg <= 1.0)) and np.all(np.abs(yg.sum(1) - 1.0) <= 4 * 2.0 ** -52), (case["id"], gi)
            p[tag] = pmf_test(1 + np.argmax(yg, 1), a / a.sum())
        elif kind == "disc":
            if case.get("exact_last") and gi == len(case["groups"]) - 1:
                lam = float(safe_exp(f[0]))
                assert lam > 1e15 and np.all(yg == yg[0]) and abs(yg[0] - lam) <= np.spacing(lam), (case["id"], "lambda > 1e15 is its own draw")
                continue
            lw = law(name, f, **kw)
            n = float(int(kw.get("pred_trials", 0)) or np.inf)
            assert np.all((yg >= 0.0) & (yg <= n) & (yg == np.floor(yg))), (case["id"], gi, "a draw that is no count of the support")
            p[tag] = discrete_test(yg, lw)
        elif kind == "binary":
            assert set(np.unique(yg)) <= {0.0, 1.0}
            p[tag] = binom_test(np.sum(yg == 1.0), yg.size, float(law(name, f, **kw)[0]))
        elif kind == "pmf":
            p[tag] = pmf_test(yg, law(name, f, **kw)[0])
    if case.get("lag"):     # randomised PIT over the groups with a law (the exact group left out)
        use = np.concatenate(case["groups"][:-1]) if case.get("exact_last") else np.arange(F.shape[0])
        use.sort()
        lw = law(name, F[use], **kw)
        v = np.random.RandomState(seed).uniform(size=use.size)
        y2 = np.asarray(draw(name, F, seed + 1, **kw), float)[:, 0]
        u = lw.cdf(y[use] - 1.0) + v * lw.pmf(y[use])
        u2 = lw.cdf(y2[use] - 1.0) + v[::-1] * lw.pmf(y2[use])
        p["lag_rows"] = lag_test(u[:-1], u[1:])
        p["lag_seeds"] = lag_test(u, u2)
    return p


# ------------------------------------------------------------------------------------------------ the generator pin
# branch-free samplers: the device draws equal the restated ones row by row (labels equal; continuous draws within 1e-12 of the row's
# scale -- the law's scale or the draw's own size, whichever is larger: a Weibull draw is its scale times a power that reaches 1e78)
PIN_CASES = ("gaussian_sigma_0.7", "hetgaussian", "exponential", "weibull", "bernoulli", "categorical_K2", "categorical_K4", "categorical_K6",
             "categorical_den_overflow_K4")
PIN_LABELS = ("Bernoulli", "Categorical", "Ordinal")
REJECTION_CASES = ("gamma", "beta", "student_nu_5", "poisson", "negbinomial", "binomial_n1000", "betabinomial_n20", "zipoisson", "dirichlet_K3")


def ordinal_pin_case():
    rng = np.random.RandomState(190)
    return _case("ordinal", "Ordinal", "pin", 1110, {"bin_edges": [-1.3, -0.2, 0.4, 2.0], "sigma": 0.8}, F=rng.uniform(-3, 3, (N_ROWS, 1)))


def pin_scale(case, y_ref):
    name, F, kw = case["name"], case["F"], case["kw"]
    if name == "Gaussian":
        s = np.full(F.shape[0], kw["sigma"])
    elif name == "HetGaussian":
        s = np.sqrt(safe_exp(F[:, 1]))
    elif name == "Exponential":
        s = clip9(safe_exp(-F[:, 0]))
    else:
        s = safe_exp(F[:, 0])
    with np.errstate(invalid="ignore"):
        return np.maximum(s, np.where(np.isfinite(y_ref), np.abs(y_ref), 0.0))


# ------------------------------------------------------------------------------------------------ what two moments would have seen
def moments_within_5se(name, f, kw, corrupt, S=40000, seed=77):
    """The check the suite had before: 40 000 draws at one f, mean and variance within 5 standard errors of the law's.  True: the
    corrupted sampler would have passed it."""
    lw = law(name, f, **kw)
    y = restated_sample(name, np.tile(np.asarray(f, float)[None, :], (S, 1)), seed, corrupt=corrupt, **kw)[:, 0]
    if hasattr(lw, "stats") and not isinstance(lw, ZipLaw):
        m, v, _, k = [float(np.ravel(t)[0]) for t in lw.stats(moments="mvsk")]
        m4 = (k + 3.0) * v * v
    else:
        m, v = [float(np.ravel(t)[0]) for t in lw.stats()]
        m4 = 3.0 * v * v
    return bool(abs(y.mean() - m) <= 5.0 * np.sqrt(v / S) and abs(y.var() - v) <= 5.0 * np.sqrt(max(m4 - v * v, 0.0) / S))
