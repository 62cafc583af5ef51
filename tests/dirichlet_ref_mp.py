"""High-precision restatement (mpmath) of the Dirichlet likelihood of DESIGN 9d, from the contract's decomposed formulas, with the
conventions of tests/lik_ref_mp.py and tests/ordinal_ref_mp.py: the float64 inputs (y, m, v) and the float64 Gauss-Hermite tables
are exact numbers, everything else is carried in high precision, and every output element comes as

  R  the value, sum of weight * addend over the addends the formula writes;
  S  the condition scale, the same sum over the absolute values of those addends.

Addends (10 nodes per dimension, weights w / sqrt(pi) once per dimension, W = prod_k w_{i_k}, a_k(i) = clip(exp(min(f_k(i), LIM)), 1e-9, 1e9),
A = sum_k a_k):
  ve:    W lgamma(A) per node;  -w_i lgamma(a_k(i)),  w_i a_k(i) log y_k  per (k, i);  -log y_k per k
  dm_k:  W a_k psi(A) per node;  -w_i a_k(i) psi(a_k(i)),  w_i a_k(i) log y_k  per i
  dv_k:  half of: the addends of dm_k,  W a_k^2 psi'(A) per node,  -w_i a_k(i)^2 psi'(a_k(i)) per i

Independent of the float64 code (imports neither hetmogp_amd nor lik_dirichlet).  The clip bounds and LIM are the float64 numbers of the
contract.  psi' is evaluated by its recurrence and asymptotic series here (mpmath.psi(1, .) goes through the Hurwitz zeta function and
costs twenty times as much; the two are compared in tests/test_dirichlet_cpu.py).  40 working digits: R is wanted to well below
2^-52 S, a bound relative to the sum of the ABSOLUTE addends, which no cancellation between them touches."""
import itertools

import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 40
LIM_VAL = 709.782712893384
LO, HI = 1e-9, 1e9


def gh10():
    x, w = np.polynomial.hermite.hermgauss(10)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


_BERN = [mpmath.bernfrac(2 * k) for k in range(1, 61)]      # B_2, B_4, ..: exact fractions


def trigamma(x):
    """psi'(x), x > 0: recurrence up to x >= 25, then 1/x + 1/(2 x^2) + sum_k B_2k / x^(2k+1) until the terms drop below the precision.
    Carried in integer fixed point with 48 guard bits (a tenth of the cost of mpf operations in pure Python)."""
    P = mp.prec + 48
    one = 1 << P
    X = int(mpmath.floor(mpmath.ldexp(x, P)))
    s = 0
    while X < 25 * one:
        s += (one << (2 * P)) // (X * X)
        X += one
    ix = (one << P) // X
    z = (ix * ix) >> P
    s += ix + (z >> 1)
    t = (ix * z) >> P
    for num, den in _BERN:
        term = t * num // den
        s += term
        if abs(term) >> 8 == 0:
            return mpmath.ldexp(mpf(s), -P)
        t = (t * z) >> P
    raise ArithmeticError("trigamma series did not converge")


def alpha(f):
    a = mpmath.exp(min(f, mpf(LIM_VAL)))
    return min(max(a, mpf(LO)), mpf(HI))


def row(y, m, v):
    """One row of var_exp: y, m, v [K] float64 -> (R [1 + 2 K], S [1 + 2 K]) for ve, dm_0.., dv_0.. as float64 (R rounded to nearest)."""
    K = len(y)
    with mp.workdps(WORK_DPS):
        x, w = gh10()
        ly = [mpmath.log(mpf(float(t))) for t in y]
        a = [[alpha(mpf(float(m[k])) + mpmath.sqrt(2 * mpf(float(v[k]))) * xi) for xi in x] for k in range(K)]
        # running sums: ve, and per k the first-derivative addends (g) and the psi' addends (h); dv = (g + h) / 2
        R0 = S0 = mpf(0)
        Rg, Sg, Rh, Sh = [mpf(0)] * K, [mpf(0)] * K, [mpf(0)] * K, [mpf(0)] * K
        for idx in itertools.product(range(10), repeat=K):
            W, A = mpf(1), mpf(0)
            for k, i in enumerate(idx):
                W *= w[i]
                A += a[k][i]
            t = W * mpmath.loggamma(A)
            R0 += t
            S0 += abs(t)
            pA, zA = W * mpmath.psi(0, A), W * trigamma(A)
            apA = abs(pA)
            for k, i in enumerate(idx):
                ak = a[k][i]
                Rg[k] += pA * ak
                Sg[k] += apA * ak
                Rh[k] += zA * ak * ak                  # (positive: its own absolute value)
        Sh = list(Rh)
        for k in range(K):
            R0 -= ly[k]
            S0 += abs(ly[k])
            for i in range(10):
                ak = a[k][i]
                t = w[i] * mpmath.loggamma(ak)
                R0 -= t
                S0 += abs(t)
                t = w[i] * ak * ly[k]
                R0 += t
                S0 += abs(t)
                Rg[k] += t
                Sg[k] += abs(t)
                t = w[i] * ak * mpmath.psi(0, ak)
                Rg[k] -= t
                Sg[k] += abs(t)
                t = w[i] * ak * ak * trigamma(ak)
                Rh[k] -= t
                Sh[k] += t
        R = [R0] + Rg + [(g + h) / 2 for g, h in zip(Rg, Rh)]
        S = [S0] + Sg + [(g + h) / 2 for g, h in zip(Sg, Sh)]
        return np.array([float(r) for r in R]), np.array([float(s) for s in S])


def var_exp(y, m, v, K):
    """y, m, v [N, K] -> R, S [N, 1 + 2 K]."""
    y, m, v = (np.asarray(t, float).reshape(-1, K) for t in (y, m, v))
    out = [row(yy, mm, vv) for yy, mm, vv in zip(y, m, v)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
