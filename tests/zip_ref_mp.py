"""High-precision restatement (mpmath, 50 digits) of the zero-inflated Poisson likelihood of DESIGN 9n, with the conventions of
tests/lik_ref_mp.py and tests/negbin_ref_mp.py: the float64 inputs (y, m, v) and the float64 Gauss-Hermite tables are exact numbers,
everything else is carried in high precision, and every output element comes as

  R  the value, sum of weight * addend over the addends the contract writes;
  S  the condition scale, the same sum over the absolute values of those addends.

lambda_i = exp(min(f0_i, LIM)), pi_j = clip(ef / (1 + ef), 1e-9, 1 - 1e-9) with ef = exp(min(f1_j, LIM)) (the clip's bounds are the float64
numbers 1e-9 and 1 - 1e-9).

Rows with y >= 1 -- the sum of two 20-node rules, weights w_i over f0 and w_j over f1 (Poisson's and Bernoulli's addends, tests/lik_ref_mp.py):
  ve:    w_i: -lambda, y f0, -lgamma(y+1);   w_j: log(1 - pi)
  dm_0:  w_i: y, -lambda                     dm_1:  w_j: -pi / ((1 - pi) (1 + ef))
  dv_0:  half of w_i: -lambda                dv_1:  half of w_j: -pi / (1 + ef)
Rows with y = 0 -- the 20 x 20 rule, W = w_i w_j, lpi = log pi, u = log(1 - pi) - lambda - lpi, rho = sigmoid(u), t = lambda rho,
log p0 = lpi + softplus(u), g = pi (1 - pi) (1 - exp(-lambda)) / p0:
  ve:    lpi, softplus(u)
  dm_0:  -t                                  dm_1:  g (ONE addend)
  dv_0:  half of: -t, lambda t (1 - rho)     dv_1:  half of: g (rho - pi) (one addend)

Independent of the float64 code (imports neither hetmogp_amd nor zip_ref).  lpd_row: the deterministic log predictive density of DESIGN 9j
over the 20 x 20 nodes, for the device test's fixture."""
import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
LIM_VAL = 709.782712893384
PLO, PHI = 1e-9, 1.0 - 1e-9


def gh20():
    x, w = np.polynomial.hermite.hermgauss(20)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def _tables(m, v, x):
    f0 = [mpf(float(m[0])) + mpmath.sqrt(2 * mpf(float(v[0]))) * xi for xi in x]
    f1 = [mpf(float(m[1])) + mpmath.sqrt(2 * mpf(float(v[1]))) * xj for xj in x]
    lam = [mpmath.exp(min(f, mpf(LIM_VAL))) for f in f0]
    ef = [mpmath.exp(min(f, mpf(LIM_VAL))) for f in f1]
    pi = [min(max(e / (1 + e), mpf(PLO)), mpf(PHI)) for e in ef]
    return f0, lam, ef, pi


def _zero_node(lam, pi):
    lpi = mpmath.log(pi)
    u = mpmath.log(1 - pi) - lam - lpi
    a = mpmath.exp(-abs(u))
    sp = max(u, mpf(0)) + mpmath.log1p(a)
    inv = 1 / (1 + a)
    rho, rhoc = (inv, a * inv) if u >= 0 else (a * inv, inv)
    return lpi, sp, rho, rhoc


def row(y, m, v):
    """One row of var_exp: y float64, m, v [2] float64 -> (R [5], S [5]) for ve, dm_0, dm_1, dv_0, dv_1 as float64 (R rounded to nearest)."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        y = mpf(float(y))
        f0, lam, ef, pi = _tables(m, v, x)
        R, S = [mpf(0)] * 5, [mpf(0)] * 5

        def add(k, W, t):
            R[k] += W * sum(t)
            S[k] += W * sum(abs(a) for a in t)
        if y > 0:
            lgy1 = mpmath.loggamma(y + 1)
            for i in range(20):
                add(0, w[i], (-lam[i], y * f0[i], -lgy1))
                add(1, w[i], (y, -lam[i]))
                add(3, w[i], (-lam[i],))
            for j in range(20):
                add(0, w[j], (mpmath.log(1 - pi[j]),))
                add(2, w[j], (-pi[j] / ((1 - pi[j]) * (1 + ef[j])),))
                add(4, w[j], (-pi[j] / (1 + ef[j]),))
        else:
            for i in range(20):
                for j in range(20):
                    W = w[i] * w[j]
                    lpi, sp, rho, rhoc = _zero_node(lam[i], pi[j])
                    t = lam[i] * rho
                    g = pi[j] * (1 - pi[j]) * (-mpmath.expm1(-lam[i])) * mpmath.exp(-(lpi + sp))
                    add(0, W, (lpi, sp))
                    add(1, W, (-t,))
                    add(2, W, (g,))
                    add(3, W, (-t, lam[i] * t * rhoc))
                    add(4, W, (g * (rho - pi[j]),))
        for k in (3, 4):
            R[k], S[k] = R[k] / 2, S[k] / 2
        return np.array([float(t) for t in R]), np.array([float(t) for t in S])


def var_exp(y, m, v):
    """y [N], m, v [N, 2] -> R, S [N, 5]."""
    y, m, v = np.asarray(y, float).reshape(-1), np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    out = [row(yy, mm, vv) for yy, mm, vv in zip(y, m, v)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def lpd_row(y, m, v):
    """log sum_ij w_i w_j p(y | f0_i, f1_j) of one row, as float64."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        y = mpf(float(y))
        f0, lam, ef, pi = _tables(m, v, x)
        lgy1 = mpmath.loggamma(y + 1)
        tot = mpf(0)
        for i in range(20):
            for j in range(20):
                if y > 0:
                    p = (1 - pi[j]) * mpmath.exp(-lam[i] + y * f0[i] - lgy1)
                else:
                    p = pi[j] + (1 - pi[j]) * mpmath.exp(-lam[i])
                tot += w[i] * w[j] * p
        return float(mpmath.log(tot))
