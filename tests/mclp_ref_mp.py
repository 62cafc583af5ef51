"""High-precision restatement (mpmath, 50 digits) of the Monte-Carlo log predictive density of DESIGN 9q (`hmogp_log_predictive`), with the
conventions of tests/logpred_ref_mp.py: the float64 inputs are exact numbers, everything else is carried in high precision.

The draw: h, h2 from the integer hash (Python integers), u1 = ((h >> 11) + 1) / 2^53 and u2 = (h2 >> 11) / 2^53 exact float64 numbers, the
angle fl(fl(2 pi) u2) the ONE float64 product the kernel forms (an exact number from there on); r = sqrt(-2 log u1), cos, sin, sqrt(v),
f = m + sqrt(v) z, the addends of log p and the log-sum in 50 digits.

Addends of log p at a sample: `logpred_ref_mp.addends`, and here
  Gaussian      -log(2 pi)/2,  -(y - f)^2 / 2                                   (sigma ignored: quirk Q6)
  HetGaussian   -log(2 pi)/2,  -f1 / 2,  -min(y - f0, sqrt(DBL_MAX))^2 / (2 safe_exp(f1))
  Binomial      p = clip(ef / (1 + ef), 1e-9, 1 - 1e-9):  lgamma(n + 1),  -lgamma(k + 1),  -lgamma(n - k + 1),  k log p,  (n - k) log(1 - p)
  BetaBinomial  a = clip9(safe_exp(f0)), b = clip9(safe_exp(f1)):  the three lgammas of log C(n, k),  lgamma(k + a) - lgamma(a),
                lgamma(n - k + b) - lgamma(b),  -(lgamma(n + a + b) - lgamma(a + b))         (each difference ONE addend)
  ZIPoisson     lam = safe_exp(f0), pi = clip(ef / (1 + ef), 1e-9, 1 - 1e-9) of f1;  y >= 1: -lam, y f0, -lgamma(y + 1), log(1 - pi);
                y = 0: log pi, softplus(log(1 - pi) - lam - log pi)

A sample whose log p is -inf or below -DBL_MAX contributes nothing.  Per row, with wbar the normalised exp(l_s), A_s the sum of the absolute
addends at sample s and d_j l_s a central difference in f_j at 50 digits:

  R  = -log S + log sum_s exp(l_s)
  Sc = 1 + |log S| + sum_s wbar_s (A_s + sum_j |d_j l_s| (|m_j| + 4 sqrt(v_j) |z_sj|))

Independent of the float64 code (imports neither hetmogp_amd nor mclp_ref)."""
import math

import mpmath
import numpy as np

import logpred_ref_mp as lmp

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
M64 = 2 ** 64 - 1
NINF = lmp.NINF
DBL_MAX = lmp.DBL_MAX
TWO_PI_F64 = 2.0 * math.pi          # fl(2 pi): doubling is exact


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniforms(seed, n, s, pair):
    """(u1, u2) as exact float64 numbers."""
    h = splitmix64(splitmix64((seed ^ (n * 0xD1342543DE82EF95)) & M64) ^ ((s << 8) & M64) ^ pair)
    h2 = splitmix64(h)
    return ((h >> 11) + 1) * 2.0 ** -53, (h2 >> 11) * 2.0 ** -53


def normal_pair(seed, n, s, pair):
    u1, u2 = uniforms(int(seed), int(n), int(s), int(pair))
    ang = mpf(TWO_PI_F64 * u2)
    r = mpmath.sqrt(-2 * mpmath.log(mpf(u1)))
    return r * mpmath.cos(ang), r * mpmath.sin(ang)


def addends(name, y, f, kw):
    if name == "Gaussian":
        d = mpf(float(y)) - f[0]
        return [-mpmath.log(2 * mpmath.pi) / 2, -d * d / 2]
    if name == "HetGaussian":
        d = min(mpf(float(y)) - f[0], lmp.SQRT_DBL_MAX)           # safe_square clips from above alone
        return [-mpmath.log(2 * mpmath.pi) / 2, -f[1] / 2, -d * d / (2 * lmp._sexp(f[1]))]
    if name == "Binomial":
        k, n = mpf(float(y[0])), mpf(float(y[1]))
        ef = lmp._sexp(f[0])
        p = lmp._clip(ef / (1 + ef), 1e-9, 1.0 - 1e-9)
        return [mpmath.loggamma(n + 1), -mpmath.loggamma(k + 1), -mpmath.loggamma(n - k + 1), k * mpmath.log(p), (n - k) * mpmath.log(1 - p)]
    if name == "BetaBinomial":
        k, n = mpf(float(y[0])), mpf(float(y[1]))
        a, b = lmp._clip(lmp._sexp(f[0]), 1e-9, 1e9), lmp._clip(lmp._sexp(f[1]), 1e-9, 1e9)
        return [mpmath.loggamma(n + 1), -mpmath.loggamma(k + 1), -mpmath.loggamma(n - k + 1), mpmath.loggamma(k + a) - mpmath.loggamma(a),
                mpmath.loggamma(n - k + b) - mpmath.loggamma(b), -(mpmath.loggamma(n + a + b) - mpmath.loggamma(a + b))]
    if name == "ZIPoisson":
        yy = mpf(float(y))
        lam = lmp._sexp(f[0])
        ef = lmp._sexp(f[1])
        p = lmp._clip(ef / (1 + ef), 1e-9, 1.0 - 1e-9)
        if yy > 0:
            return [-lam, yy * f[0], -mpmath.loggamma(yy + 1), mpmath.log(1 - p)]
        lpi = mpmath.log(p)
        u = mpmath.log(1 - p) - lam - lpi
        return [lpi, max(u, 0) + mpmath.log1p(mpmath.exp(-abs(u)))]
    return lmp.addends(name, y, f, kw)


def _is_out(l):
    return l == NINF or l < -DBL_MAX


def row(name, y, m, v, S, seed, n, **kw):
    """One row (index n of its call): y a float or a tuple of floats, m, v [J] float64 -> (R, Sc, the number of samples that contribute
    nothing, the smallest | |l| / DBL_MAX - 1 | over the samples with l > -inf: how far the row stays from where float64 and 50 digits could
    disagree about -inf)."""
    m, v = [float(t) for t in np.ravel(m)], [float(t) for t in np.ravel(v)]
    J = len(m)
    with mp.workdps(WORK_DPS):
        sd = [mpmath.sqrt(mpf(t)) for t in v]
        h = mpf(10) ** -25
        ls, As, Ds = [], [], []
        n_out, near = 0, mpf("inf")
        for s in range(int(S)):
            z = []
            for p in range((J + 1) // 2):
                z += list(normal_pair(seed, n, s, p))
            f = [mpf(m[j]) + sd[j] * z[j] for j in range(J)]
            t = addends(name, y, f, kw)
            l = sum(t)
            if l != NINF:
                near = min(near, abs(abs(l) / DBL_MAX - 1))
            if _is_out(l):
                n_out += 1
                continue
            D = mpf(0)
            for j in range(J):
                if v[j] == 0.0 and m[j] == 0.0:
                    continue
                hj = h * max(1, abs(f[j]))
                fp, fm = list(f), list(f)
                fp[j] += hj
                fm[j] -= hj
                D += abs((sum(addends(name, y, fp, kw)) - sum(addends(name, y, fm, kw))) / (2 * hj)) * (abs(mpf(m[j])) + 4 * sd[j] * abs(z[j]))
            ls.append(l), As.append(sum(abs(a) for a in t)), Ds.append(D)
        if not ls:
            return -np.inf, 1.0 + abs(math.log(S)), n_out, float(near)
        mx = max(ls)
        e = [mpmath.exp(l - mx) for l in ls]
        tot = sum(e)
        R = -mpmath.log(mpf(int(S))) + mx + mpmath.log(tot)
        Sc = 1 + abs(mpmath.log(mpf(int(S)))) + sum(w * (a + d) for w, a, d in zip(e, As, Ds)) / tot
        return float(R), float(Sc), n_out, float(near)
