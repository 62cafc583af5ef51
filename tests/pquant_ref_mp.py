"""High-precision restatement (mpmath, 50 digits) of the predictive cdf and survival function of DESIGN 9k, with the conventions of
tests/logpred_ref_mp.py: the float64 inputs (y, m, v, the likelihood's parameters, the clips' constants) and the float64 Gauss-Hermite
tables are exact numbers, everything else is carried in high precision.  Per row:

  R = (cdf, sf):  cdf = sum_i w_i C_i,  sf = sum_i w_i S_i      (C_i, S_i: the conditional pair at node i, listed in tests/pquant_ref.py)
  S = (S_cdf, S_sf):  1 + sum_i (w_i G_i / sum_j w_j G_j) A_i,  G = C or S,  A_i = the magnitude of the conditional exponent at node i:
      z^2 / 2 (Gaussian, HetGaussian, Ordinal), y / b (Exponential), e + |z| (Weibull), 0 (Bernoulli); S = 1 where the output is 0 in float64

Independent of the float64 code (imports neither hetmogp_amd nor pquant_ref)."""
import itertools

import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
LIM_VAL = mpf(709.782712893384)
ZMAX = mpf(680)
INF = mpf("inf")


def gh(T):
    x, w = np.polynomial.hermite.hermgauss(int(T))
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def _sexp(f):
    return mpmath.exp(min(f, LIM_VAL))


def _clip(x, lo, hi):
    return min(max(x, mpf(lo)), mpf(hi))


def _phi_pair(z):
    if z == INF:
        return mpf(1), mpf(0)
    if z == -INF:
        return mpf(0), mpf(1)
    r = mpmath.sqrt(mpf(1) / 2)
    return mpmath.erfc(-z * r) / 2, mpmath.erfc(z * r) / 2


def _out(x):
    """float64 of a high-precision value; a positive value below the smallest subnormal stays what float() makes of it."""
    return float(x)


def row(name, y, m, v, gh_T=0, **kw):
    """One row: y a float (Ordinal: the label; Weibull: the time), m, v [J] float64 -> (R [2] = cdf, sf; S [2]) as float64."""
    m, v = [float(t) for t in np.ravel(m)], [float(t) for t in np.ravel(v)]
    y = float(y)
    with mp.workdps(WORK_DPS):
        T = int(gh_T) or 20
        nodes = []     # (weight, C, S, A)
        if name in ("Gaussian", "Ordinal"):
            s = kw.get("sigma")
            s = (0.5 if s is None or not s > 0.0 else float(s)) if name == "Gaussian" else float(kw.get("sigma", 1.0))
            sd = mpmath.sqrt(mpf(s) ** 2 + mpf(v[0]))
            if name == "Ordinal":
                edges = kw.get("bin_edges")
                if edges is None:
                    edges = [k - 0.5 * int(kw["K"]) for k in range(1, int(kw["K"]))]
                ext = [mpf(float(t)) for t in edges] + [INF]
                yy = ext[int(y) - 1]
            else:
                yy = mpf(y)
            z = (yy - mpf(m[0])) / sd
            C, S = _phi_pair(z)
            nodes.append((mpf(1), C, S, z * z / 2 if abs(z) != INF else mpf(0)))
        elif name == "HetGaussian":
            x, w = gh(T)
            for xi, wi in zip(x, w):
                sd = mpmath.sqrt(mpf(v[0]) + _sexp(mpf(m[1]) + mpmath.sqrt(2 * mpf(v[1])) * xi))
                z = (mpf(y) - mpf(m[0])) / sd
                C, S = _phi_pair(z)
                nodes.append((wi, C, S, z * z / 2))
        else:
            x, w = gh(T)
            J = len(m)
            fd = [[mpf(m[k]) + mpmath.sqrt(2 * mpf(v[k])) * xi for xi in x] for k in range(J)]
            for idx in itertools.product(range(T), repeat=J):
                W = mpf(1)
                for i in idx:
                    W *= w[i]
                f = [fd[k][i] for k, i in enumerate(idx)]
                if name == "Bernoulli":
                    ef = _sexp(f[0])
                    p = _clip(ef / (1 + ef), 1e-9, 1.0 - 1e-9)
                    C, S = (mpf(0), mpf(1)) if y < 0.0 else ((1 - p, p) if y < 1.0 else (mpf(1), mpf(0)))
                    A = mpf(0)
                elif name == "Exponential":
                    b = _clip(_sexp(-f[0]), 1e-9, 1e9)
                    if y <= 0.0:
                        C, S, A = mpf(0), mpf(1), mpf(0)
                    else:
                        a = mpf(y) / b
                        C, S, A = -mpmath.expm1(-a), mpmath.exp(-a), a
                elif name == "Weibull":
                    if y <= 0.0:
                        C, S, A = mpf(0), mpf(1), mpf(0)
                    else:
                        k = _clip(_sexp(f[1]), 1e-3, 1e3)
                        z = min(k * (mpmath.log(mpf(y)) - f[0]), ZMAX)
                        e = mpmath.exp(z)
                        C, S, A = -mpmath.expm1(-e), mpmath.exp(-e), e + abs(z)
                else:
                    raise KeyError(name)
                nodes.append((W, C, S, A))
        R, Sc = [], []
        for col in (1, 2):
            tot = sum(t[0] * t[col] for t in nodes)
            R.append(_out(tot))
            Sc.append(_out(1 + sum(t[0] * t[col] * t[3] for t in nodes) / tot) if float(tot) > 0.0 else 1.0)   # (an exact 0: no scale)
        return np.array(R), np.array(Sc)
