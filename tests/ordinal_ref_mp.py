"""High-precision restatement (mpmath) of the Ordinal (ordered probit) likelihood of DESIGN 9b, node by node from the contract's
formulas, with the conventions of tests/lik_ref_mp.py: the float64 inputs (label's cut points, sigma, m, v) and the float64
Gauss-Hermite tables are exact numbers, everything else is carried in high precision, and every output element comes as

  R  the value, sum over nodes of weight * (sum of the addends the formula writes);
  S  the condition scale, sum over nodes of weight * (sum of the absolute values of those addends).

Addends of one node, with a = (lo - f) / sigma, b = (hi - f) / sigma, P = Phi(b) - Phi(a):
  log p:        log P
  dlog p/df:    phi(a) / (sigma P),   -phi(b) / (sigma P)
  d2log p/df2:  a phi(a) / (sigma^2 P),   -b phi(b) / (sigma^2 P),   -(dlog p/df)^2       (terms with an infinite a or b are 0)

Independent of the float64 code (imports neither hetmogp_amd nor lik_ordinal).  Precision: P itself needs two rewrites that no
number of digits buys back -- in the upper tail Phi(b) - Phi(a) is 1 - 1 to 10^5 digits -- so the bin is mirrored onto the lower
side and a bin that straddles f is 1 - (two tails); after that the only cancellation left is a narrow bin's (6 digits at 1e-6
sigma), and 120 working digits are ample for results rounded to 50."""
import mpmath
import numpy as np

mp = mpmath.mp
mpf = mpmath.mpf
WORK_DPS = 120
INF = float("inf")


def gh20():
    x, w = np.polynomial.hermite.hermgauss(20)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def _lower(x):
    """Phi(x) for x <= 0 (x may be -inf)."""
    if x == -mpmath.inf:
        return mpf(0)
    return mpmath.erfc(-x / mpmath.sqrt(2)) / 2


def _phi(x):
    if mpmath.isinf(x):
        return mpf(0)
    return mpmath.exp(-x * x / 2) / mpmath.sqrt(2 * mpmath.pi)


def prob_terms(a, b):
    """(log P, P) of P = Phi(b) - Phi(a), a < b, either may be infinite (not both)."""
    if a + b > 0:
        a, b = -b, -a
    if b <= 0:
        P = _lower(b) - _lower(a)
        return mpmath.log(P), P
    Q = _lower(a) + _lower(-b)
    return mpmath.log1p(-Q), 1 - Q


def node(lo, hi, f, sigma):
    """addends of log p, dlog p/df, d2log p/df2 at one f."""
    a = -mpmath.inf if lo == -INF else (mpf(lo) - f) / sigma
    b = mpmath.inf if hi == INF else (mpf(hi) - f) / sigma
    lp, P = prob_terms(a, b)
    pa, pb = _phi(a), _phi(b)
    t1 = [pa / (sigma * P), -pb / (sigma * P)]
    d1 = t1[0] + t1[1]
    apa = mpf(0) if mpmath.isinf(a) else a * pa
    bpb = mpf(0) if mpmath.isinf(b) else b * pb
    return [lp], t1, [apa / (sigma * sigma * P), -bpb / (sigma * sigma * P), -d1 * d1]


def _acc(pairs):
    r = sum(w * t for w, ts in pairs for t in ts)
    s = sum(w * abs(t) for w, ts in pairs for t in ts)
    return r, s


def row(lo, hi, sigma, m, v):
    """One row of var_exp: (R [3], S [3]) for ve, dm, dv as float64 (R rounded to nearest)."""
    with mp.workdps(WORK_DPS):
        x, w = gh20()
        sg, mm, sv = mpf(float(sigma)), mpf(float(m)), mpmath.sqrt(2 * mpf(float(v)))
        nodes = [(wi, node(lo, hi, mm + sv * xi, sg)) for xi, wi in zip(x, w)]
        out = [_acc([(wi, n[0]) for wi, n in nodes]), _acc([(wi, n[1]) for wi, n in nodes]),
               _acc([(wi / 2, n[2]) for wi, n in nodes])]
        return np.array([float(r) for r, _ in out]), np.array([float(s) for _, s in out])


def cuts(label, edges):
    ext = [-INF] + [float(e) for e in edges] + [INF]
    k = int(label)
    return ext[k - 1], ext[k]


def var_exp(y, m, v, bin_edges, sigma):
    """y [N] labels, m, v [N] -> R, S [N, 3]."""
    out = [row(*cuts(yy, bin_edges), sigma, mm, vv) for yy, mm, vv in zip(np.reshape(y, -1), np.reshape(m, -1), np.reshape(v, -1))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def class_probs(m, v, bin_edges, sigma):
    """[P_1 .. P_K] (mpf) of one row under q(f) = N(m, v)."""
    s = mpmath.sqrt(mpf(float(sigma)) ** 2 + mpf(float(v)))
    ext = [-INF] + [float(e) for e in bin_edges] + [INF]
    z = [(-mpmath.inf if e == -INF else mpmath.inf if e == INF else (mpf(e) - mpf(float(m))) / s) for e in ext]
    return [prob_terms(z[k], z[k + 1]) for k in range(len(ext) - 1)]


def predictive_row(m, v, bin_edges, sigma):
    """(R_mean, S_mean, R_var, S_var): mean = sum k P_k (S the same sum), var = sum k^2 P_k - mean^2 (S = sum k^2 P_k + mean^2)."""
    with mp.workdps(WORK_DPS):
        P = [p for _, p in class_probs(m, v, bin_edges, sigma)]
        mean = sum((k + 1) * p for k, p in enumerate(P))
        m2 = sum((k + 1) ** 2 * p for k, p in enumerate(P))
        return float(mean), float(mean), float(m2 - mean * mean), float(m2 + mean * mean)


def log_prob(label, m, v, bin_edges, sigma):
    """closed-form log P_y(m, v), float64."""
    with mp.workdps(WORK_DPS):
        return float(class_probs(m, v, bin_edges, sigma)[int(label) - 1][0])
