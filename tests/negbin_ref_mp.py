"""High-precision restatement (mpmath, 50 digits) of the Negative Binomial likelihood of DESIGN 9h, with the conventions of
tests/lik_ref_mp.py and tests/dirichlet_ref_mp.py: the float64 inputs (y, m, v) and the float64 Gauss-Hermite tables are exact
numbers, everything else is carried in high precision, and every output element comes as

  R  the value, sum of weight * addend over the addends the contract writes;
  S  the condition scale, the same sum over the absolute values of those addends.

Addends per node (i, j) of the 20 x 20 rule, W = w_i w_j (weights w / sqrt(pi) once per dimension), r_j = clip(exp(min(f1_j, LIM)), 1e-9, 1e9),
z_ij = min(f0_i, LIM) - log r_j, sp = softplus(z), p = sigmoid(z), q = 1 - p, and the three differences G_j, D1_j, D2_j of lgamma, psi, psi'
between y + r_j and r_j, each counted as ONE addend:
  ve:    G_j,  -lgamma(y+1),  y z,  -r sp,  -y sp
  dm_0:  y q,  -r p
  dm_1:  r D1,  -r sp,  -y q,  r p
  dv_0:  half of:  -r p q,  -y p q
  dv_1:  half of:  r D1,  -r sp,  r^2 D2,  2 r p,  -r p q,  -y p q

Independent of the float64 code (imports neither hetmogp_amd nor negbin_ref).  At 50 digits the plain differences are exact far beyond
float64 (at r = 1e9 they lose ten digits of fifty).  psi' is dirichlet_ref_mp's (recurrence + asymptotic series in fixed point)."""
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
    """(G, D1, D2) at high precision (y, r: mpf)."""
    return (mpmath.loggamma(y + r) - mpmath.loggamma(r), mpmath.psi(0, y + r) - mpmath.psi(0, r), trigamma(y + r) - trigamma(r))


def row(y, m, v):
    """One row of var_exp: y float64, m, v [2] float64 -> (R [5], S [5]) for ve, dm_0, dm_1, dv_0, dv_1 as float64 (R rounded to nearest)."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        y = mpf(float(y))
        lgy1 = mpmath.loggamma(y + 1)
        f0 = [min(mpf(float(m[0])) + mpmath.sqrt(2 * mpf(float(v[0]))) * xi, mpf(LIM_VAL)) for xi in x]
        cols = []
        for xj in x:
            f1 = mpf(float(m[1])) + mpmath.sqrt(2 * mpf(float(v[1]))) * xj
            r = min(max(mpmath.exp(min(f1, mpf(LIM_VAL))), mpf(LO)), mpf(HI))
            cols.append((r, mpmath.log(r)) + diffs(y, r))
        R, S = [mpf(0)] * 5, [mpf(0)] * 5
        for i in range(20):
            for j in range(20):
                W = w[i] * w[j]
                r, lr, G, D1, D2 = cols[j]
                z = f0[i] - lr
                a = mpmath.exp(-abs(z))
                sp = max(z, mpf(0)) + mpmath.log1p(a)
                inv = 1 / (1 + a)
                p, q = (inv, a * inv) if z >= 0 else (a * inv, inv)
                adds = ((G, -lgy1, y * z, -r * sp, -y * sp),
                        (y * q, -r * p),
                        (r * D1, -r * sp, -y * q, r * p),
                        (-r * p * q, -y * p * q),
                        (r * D1, -r * sp, r * r * D2, 2 * r * p, -r * p * q, -y * p * q))
                for k, t in enumerate(adds):
                    R[k] += W * sum(t)
                    S[k] += W * sum(abs(u) for u in t)
        for k in (3, 4):
            R[k], S[k] = R[k] / 2, S[k] / 2
        return np.array([float(t) for t in R]), np.array([float(t) for t in S])


def var_exp(y, m, v):
    """y [N], m, v [N, 2] -> R, S [N, 5]."""
    y, m, v = np.asarray(y, float).reshape(-1), np.asarray(m, float).reshape(-1, 2), np.asarray(v, float).reshape(-1, 2)
    out = [row(yy, mm, vv) for yy, mm, vv in zip(y, m, v)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
