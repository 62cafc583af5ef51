"""High-precision restatement (mpmath, 50 digits) of the Binomial and Beta-Binomial likelihoods of DESIGN 9l, with the conventions of
tests/negbin_ref_mp.py: the float64 inputs (k, n, m, v) and the float64 Gauss-Hermite tables are exact numbers, everything else is
carried in high precision, and every output element comes as

  R  the value, sum of weight * addend over the addends the contract writes;
  S  the condition scale, the same sum over the absolute values of those addends.

Binomial, per node i of the 20-node rule, p = clip(e / (1 + e), 1e-9, fl(1 - 1e-9)), e = exp(min(f_i, LIM)):
  ve:  lgamma(n+1),  -lgamma(k+1),  -lgamma(n-k+1)  (each on its own: this is how lc is formed),  k log p,  (n-k) log(1-p)
  dm:  k / ((1-p)(1+e)),  -n p / ((1-p)(1+e))
  dv:  half of:  -n p / (1+e)

Beta-Binomial, per node (i, j) of the 20 x 20 rule, a_i = clip(exp(min(f0_i, LIM)), 1e-9, 1e9), b_j likewise, s = a_i + b_j, and the
differences G, D1, D2 of lgamma, psi, psi' between y + r and r, each counted as ONE addend:
  ve:    the three lgammas,  G(k,a),  G(n-k,b),  -G(n,s)
  dm_0:  a D1(k,a),  -a D1(n,s)                      dm_1:  b D1(n-k,b),  -b D1(n,s)
  dv_0:  half of:  those of dm_0,  a^2 D2(k,a),  -a^2 D2(n,s)             dv_1 likewise with b, n-k

Independent of the float64 code (imports neither hetmogp_amd nor binom_ref).  At 50 digits the plain differences are exact far beyond
float64 (at s = 2e9, n = 1e9 they lose eleven digits of fifty).  psi' is dirichlet_ref_mp's."""
import mpmath
import numpy as np

from dirichlet_ref_mp import trigamma

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
LIM_VAL = 709.782712893384
LO, HI = 1e-9, 1e9


def gh20():
    x, w = np.polynomial.hermite.hermgauss(20)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def diffs(y, r):
    """(G, D1, D2) at high precision (y, r: mpf); y = 0: exactly zero."""
    if y == 0:
        return mpf(0), mpf(0), mpf(0)
    return (mpmath.loggamma(y + r) - mpmath.loggamma(r), mpmath.psi(0, y + r) - mpmath.psi(0, r), trigamma(y + r) - trigamma(r))


def _finish(R, S, halves):
    for k in halves:
        R[k], S[k] = R[k] / 2, S[k] / 2
    return np.array([float(t) for t in R]), np.array([float(t) for t in S])


def _acc(R, S, W, adds):
    for k, t in enumerate(adds):
        R[k] += W * sum(t)
        S[k] += W * sum(abs(u) for u in t)


def _lgammas(k, n):
    return (mpmath.loggamma(n + 1), -mpmath.loggamma(k + 1), -mpmath.loggamma(n - k + 1))


def binom_row(y, m, v):
    """One Binomial row: y = (k, n), m, v float64 -> (R [3], S [3]) for ve, dm, dv as float64 (R rounded to nearest)."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        k, n = mpf(float(y[0])), mpf(float(y[1]))
        lg = _lgammas(k, n)
        R, S = [mpf(0)] * 3, [mpf(0)] * 3
        for xi, wi in zip(x, w):
            f = mpf(float(m)) + mpmath.sqrt(2 * mpf(float(v))) * xi
            e = mpmath.exp(min(f, mpf(LIM_VAL)))
            p = min(max(e / (1 + e), mpf(LO)), mpf(1.0 - LO))       # (the upper clip is the float64 number 1.0 - 1e-9)
            c = 1 / ((1 - p) * (1 + e))
            _acc(R, S, wi, (lg + (k * mpmath.log(p), (n - k) * mpmath.log(1 - p)), (k * c, -n * p * c), (-n * p / (1 + e),)))
        return _finish(R, S, (2,))


def bb_row(y, m, v):
    """One Beta-Binomial row: y = (k, n), m, v [2] float64 -> (R [5], S [5]) for ve, dm_0, dm_1, dv_0, dv_1."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        k, n = mpf(float(y[0])), mpf(float(y[1]))
        lg = _lgammas(k, n)

        def table(md, vd, cnt):
            out = []
            for xi in x:
                r = min(max(mpmath.exp(min(mpf(float(md)) + mpmath.sqrt(2 * mpf(float(vd))) * xi, mpf(LIM_VAL))), mpf(LO)), mpf(HI))
                out.append((r,) + diffs(cnt, r))
            return out
        ta, tb = table(m[0], v[0], k), table(m[1], v[1], n - k)
        R, S = [mpf(0)] * 5, [mpf(0)] * 5
        for i in range(20):
            a, Gk, D1k, D2k = ta[i]
            for j in range(20):
                b, Gn, D1n, D2n = tb[j]
                Gs, D1s, D2s = diffs(n, a + b)
                g0, g1 = (a * D1k, -a * D1s), (b * D1n, -b * D1s)
                _acc(R, S, w[i] * w[j], (lg + (Gk, Gn, -Gs), g0, g1, g0 + (a * a * D2k, -a * a * D2s), g1 + (b * b * D2n, -b * b * D2s)))
        return _finish(R, S, (3, 4))


def row(family, y, m, v):
    return binom_row(y, np.ravel(m)[0], np.ravel(v)[0]) if family == "Binomial" else bb_row(y, np.ravel(m), np.ravel(v))
