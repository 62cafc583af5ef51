"""High-precision restatement (mpmath, 50 digits) of the right-censored Weibull likelihood of DESIGN 9i, with the conventions of
tests/lik_ref_mp.py and tests/negbin_ref_mp.py: the float64 inputs (y, delta, m, v) and the float64 Gauss-Hermite tables are exact
numbers, everything else (log y included) is carried in high precision, and every output element comes as

  R  the value, sum of weight * addend over the addends the contract writes;
  S  the condition scale, the same sum over the absolute values of those addends.

Addends per node (i, j) of the 20 x 20 rule, W = w_i w_j (weights w / sqrt(pi) once per dimension), k_j = clip(exp(min(f1_j, LIM)), 1e-3, 1e3),
lk_j = log k_j, ly = log y, z_ij = min(k_j (ly - f0_i), 680), e = exp(z):
  ve:    delta lk,  -delta ly,  delta z,  -e
  dm_0:  k e,  -k delta
  dm_1:  delta,  delta z,  -e z
  dv_0:  half of:  -k^2 e
  dv_1:  half of:  delta z,  -e z,  -e z^2

The amplification of a rounding of z by |z| in exp(z) is NOT folded into S (DESIGN 9a's rule).  Independent of the float64 code
(imports neither hetmogp_amd nor weibull_ref)."""
import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 50
LIM_VAL = 709.782712893384
K_LO, K_HI = 1e-3, 1e3
Z_MAX = 680


def gh20():
    x, w = np.polynomial.hermite.hermgauss(20)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def row(y, delta, m, v):
    """One row of var_exp: y, delta float64, m, v [2] float64 -> (R [5], S [5]) for ve, dm_0, dm_1, dv_0, dv_1 as float64 (R rounded to
    nearest)."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        d = mpf(float(delta))
        ly = mpmath.log(mpf(float(y)))
        a = [ly - (mpf(float(m[0])) + mpmath.sqrt(2 * mpf(float(v[0]))) * xi) for xi in x]
        cols = []
        for xj in x:
            f1 = mpf(float(m[1])) + mpmath.sqrt(2 * mpf(float(v[1]))) * xj
            k = min(max(mpmath.exp(min(f1, mpf(LIM_VAL))), mpf(K_LO)), mpf(K_HI))
            cols.append((k, mpmath.log(k)))
        # sums over the nodes of W z, W |z|, W e, W e z, W e |z|, W e z^2 and of their products with k, k^2: every addend above is one
        # of these times a constant of the row (delta, ly) or of the column j (k, lk), and e > 0
        R, S = [mpf(0)] * 5, [mpf(0)] * 5
        zmax = mpf(Z_MAX)
        for j in range(20):
            k, lk = cols[j]
            sz = saz = se = sez = seaz = sezz = mpf(0)
            for i in range(20):
                z = min(k * a[i], zmax)
                e = w[i] * mpmath.exp(z)
                wz = w[i] * z
                ez = e * z
                sz += wz
                saz += abs(wz)
                se += e
                sez += ez
                seaz += abs(ez)
                sezz += ez * z
            wj, sw = w[j], sum(w)                               # (the weights sum to one up to their own rounding: kept as a sum)
            R[0] += wj * (d * lk * sw - d * ly * sw + d * sz - se)
            S[0] += wj * (d * abs(lk) * sw + d * abs(ly) * sw + d * saz + se)
            R[1] += wj * k * (se - d * sw)
            S[1] += wj * k * (se + d * sw)
            R[2] += wj * (d * sw + d * sz - sez)
            S[2] += wj * (d * sw + d * saz + seaz)
            R[3] -= wj * k * k * se
            S[3] += wj * k * k * se
            R[4] += wj * (d * sz - sez - sezz)
            S[4] += wj * (d * saz + seaz + sezz)
        for n in (3, 4):
            R[n], S[n] = R[n] / 2, S[n] / 2
        return np.array([float(t) for t in R]), np.array([float(t) for t in S])


def var_exp(Y, m, v):
    """Y [N, 2] = (y, delta), m, v [N, 2] -> R, S [N, 5]."""
    Y, m, v = np.asarray(Y, float).reshape(-1, 2), np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    out = [row(yy[0], yy[1], mm, vv) for yy, mm, vv in zip(Y, m, v)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
