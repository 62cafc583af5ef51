"""High-precision restatement (mpmath, 50 digits) of the variational expectations of all nine likelihood families, written
node by node from the formulas: the reference's eight families with their clips, `safe_exp` / `safe_square` bounds and quirks
Q1 / Q2 (as `oracle/likelihoods_oracle.py` documents them) and the Student-t of DESIGN 9.  Independent of the float64 code:
it imports neither the oracle nor `lik_student`.  Only `oracle/make_lik_grid.py` and `tests/test_likgrid_cpu.py` import it;
the GPU tests read the committed `tests/golden/likgrid_*.npz` instead.

The Gauss-Hermite nodes x_i and normalised weights w_i = fl(w_i / sqrt(pi)) are the float64 tables the kernels carry
(`gh_tables.h`), taken as exact numbers, and so are the float64 inputs y, m, v and the float64 constants of the reference
(LIM_VAL, sqrt(DBL_MAX), fl(sqrt(pi)), fl(pi)).  Everything else -- f = m + sqrt(2 v) x_i, exp, log, the special functions,
the sums -- is carried with 50 digits and no overflow, so the result is the value of the reference's RULE, not of the integral.

For every output element a family returns two numbers:
  R  the value, sum over nodes of weight * (sum of the addends the formula writes);
  S  the condition scale, sum over nodes of weight * (sum of the absolute values of those addends), S >= |R|.
A product whose outer factor multiplies a sum is distributed over it ((a + b) c counts |a c| + |b c|); for the two-fold
quirk-Q1 weights of Gamma / Beta the weight is w_i w_j / pi.  Output layout of a row: [ve, dm_0 .. dm_{J-1}, dv_0 .. dv_{J-1}]."""
import itertools

import mpmath
import numpy as np

mp = mpmath.mp
mp.dps = 50
mpf = mpmath.mpf

LIM_VAL = mpf(float(np.log(np.finfo(np.float64).max)))        # GPy safe_exp bound, the float64 number
SQRT_MAX = mpf(float(np.sqrt(np.finfo(np.float64).max)))      # GPy safe_square bound
SQRT_PI = mpf(float(np.sqrt(np.pi)))
PI64 = mpf(float(np.pi))
LO, HI = mpf(1e-9), mpf(1e9)                                   # the float64 numbers 1e-9, 1e9
PLO, PHI = mpf(1e-9), mpf(1.0 - 1e-9)                          # probability clip (1 - 1e-9 rounded to float64)
DIM_F = dict(Gaussian=1, Bernoulli=1, HetGaussian=2, Poisson=1, Exponential=1, Gamma=2, Beta=2, Student=2)


def dim_f(name, K=None, **_):
    return K - 1 if name == "Categorical" else DIM_F[name]


def gh(T):
    x, w = np.polynomial.hermite.hermgauss(T)
    wn = w / np.sqrt(np.pi)
    return [mpf(float(a)) for a in x], [mpf(float(a)) for a in wn]


def safe_exp(f):
    return mpmath.exp(min(f, LIM_VAL))


def safe_square(f):
    return min(f, SQRT_MAX) ** 2


def clip(x, lo, hi):
    return min(max(x, lo), hi)


class Acc:
    """R and S of one output element: add(weight, addends)."""
    __slots__ = ("r", "s")

    def __init__(self):
        self.r = mpf(0)
        self.s = mpf(0)

    def add(self, w, *terms):
        for t in terms:
            self.r += w * t
            self.s += w * abs(t)

    def scaled(self, c):
        o = Acc()
        o.r, o.s = self.r * c, self.s * abs(c)
        return o


def _f(m, v, x):
    return m + mpmath.sqrt(2 * v) * x


# ---------------------------------------------------------------------------------------------- closed forms
def gaussian(y, m, v, sigma=0.5):
    y, m, v, s2 = mpf(y), mpf(m[0]), mpf(v[0]), mpf(float(sigma)) ** 2
    ve, dm, dv = Acc(), Acc(), Acc()
    ve.add(1, -mpmath.log(2 * mpmath.pi) / 2, -mpmath.log(s2) / 2, -y * y / (2 * s2), -m * m / (2 * s2), -v / (2 * s2),
           2 * m * y / (2 * s2))
    dm.add(1, -m / s2, y / s2)
    dv.add(1, -1 / (2 * s2))
    return [ve, dm, dv]


def hetgaussian(y, m, v):
    y, m1, m2, v1, v2 = mpf(y), mpf(m[0]), mpf(m[1]), mpf(v[0]), mpf(v[1])
    prec = clip(safe_exp(-m2 + v2 / 2), -HI, HI)
    t = [safe_square(y), safe_square(m1), v1, -2 * m1 * y]
    if not -HI <= sum(t) <= HI:                          # an active clip leaves one addend, the bound
        t = [clip(sum(t), -HI, HI)]
    ve, d0, d1, h0, h1 = Acc(), Acc(), Acc(), Acc(), Acc()
    ve.add(1, -mpmath.log(2 * mpmath.pi) / 2, -m2 / 2, *[-prec * a / 2 for a in t])
    d0.add(1, prec * y, -prec * m1)
    d1.add(1, -mpf(1) / 2, *[prec * a / 2 for a in t])
    h0.add(1, -prec / 2)
    h1.add(1, *[-prec * a / 4 for a in t])
    return [ve, d0, d1, h0, h1]


# ---------------------------------------------------------------------------------------------- 1-D rules, T = 20
def _quad1(y, m, v, node):
    x, w = gh(20)
    y, m, v = mpf(y), mpf(m[0]), mpf(v[0])
    ve, dm, dv = Acc(), Acc(), Acc()
    for xi, wi in zip(x, w):
        lp, d1, d2 = node(_f(m, v, xi), y)
        ve.add(wi, *lp)
        dm.add(wi, *d1)
        dv.add(wi / 2, *d2)
    return [ve, dm, dv]


def bernoulli(y, m, v):
    def node(f, y):
        ef = safe_exp(f)
        p = clip(ef / (1 + ef), PLO, PHI)
        q = (1 - p) * (1 + ef)
        return [y * mpmath.log(p), (1 - y) * mpmath.log(1 - p)], [y / q, -p / q], [-p / (1 + ef)]
    return _quad1(y, m, v, node)


def poisson(y, m, v):
    def node(f, y):
        ef = safe_exp(f)
        return [-ef, y * f, -mpmath.loggamma(y + 1)], [y, -ef], [-ef]
    return _quad1(y, m, v, node)


def exponential(y, m, v):
    def node(f, y):
        b = clip(safe_exp(-f), LO, HI)
        return [-mpmath.log(b), -y / b], [mpf(1), -y / b], [-y / b]
    return _quad1(y, m, v, node)


# ---------------------------------------------------------------------------------------------- 2-D rules, T = 10 (quirk Q1)
def _tab2(m, v, T=10):
    x, w = gh(T)
    a = [clip(safe_exp(_f(mpf(m[0]), mpf(v[0]), xi)), LO, HI) for xi in x]
    b = [clip(safe_exp(_f(mpf(m[1]), mpf(v[1]), xi)), LO, HI) for xi in x]
    return a, b, [wi / SQRT_PI for wi in w]


def gamma(y, m, v):
    y = mpf(y)
    A, B, w = _tab2(m, v)
    ly = mpmath.log(y)
    ta = [(a, mpmath.loggamma(a), mpmath.digamma(a), mpmath.zeta(2, a)) for a in A]
    tb = [(b, mpmath.log(b)) for b in B]
    ve, d0, d1, h0, h1 = Acc(), Acc(), Acc(), Acc(), Acc()
    for (a, lga, psa, za), wi in zip(ta, w):
        for (b, lb), wj in zip(tb, w):
            ww = wi * wj
            ve.add(ww, -lga, a * lb, a * ly, -ly, -b * y)
            d0.add(ww, -psa * a, lb * a, ly * a)
            d1.add(ww, a, -b * y)
            h0.add(ww / 2, -psa * a, -a * za * a, lb * a, ly * a)
            h1.add(ww / 2, -y * b)
    return [ve, d0, d1, h0, h1]


def beta(y, m, v):
    y = mpf(y)
    A, B, w = _tab2(m, v)
    ly, l1y = mpmath.log(y), mpmath.log(1 - y)
    ta = [(a, mpmath.loggamma(a), mpmath.digamma(a), mpmath.zeta(2, a)) for a in A]
    tb = [(b, mpmath.loggamma(b), mpmath.digamma(b), mpmath.zeta(2, b)) for b in B]
    ve, d0, d1, h0, h1 = Acc(), Acc(), Acc(), Acc(), Acc()
    for (a, lga, psa, za), wi in zip(ta, w):
        for (b, lgb, psb, zb), wj in zip(tb, w):
            ww = wi * wj
            ab = a + b
            lgab, psab, zab = mpmath.loggamma(ab), mpmath.digamma(ab), mpmath.zeta(2, ab)
            ve.add(ww, a * ly, -ly, b * l1y, -l1y, -lga, -lgb, lgab)       # betaln = lgamma a + lgamma b - lgamma(a + b)
            d0.add(ww, psab * a, -psa * a, ly * a)
            d1.add(ww, psab * b, -psb * b, l1y * b)
            h0.add(ww / 2, psab * a, a * zab * a, -psa * a, -a * za * a, ly * a)
            h1.add(ww / 2, psab * b, b * zab * b, -psb * b, -b * zb * b, l1y * b)
    return [ve, d0, d1, h0, h1]


# ---------------------------------------------------------------------------------------------- Student-t, 20 x 20
def student(y, m, v, deg_free=5.0):
    nu, y = mpf(float(deg_free)), mpf(y)
    x, w = gh(20)
    R = [y - _f(mpf(m[0]), mpf(v[0]), xi) for xi in x]
    F1 = [_f(mpf(m[1]), mpf(v[1]), xi) for xi in x]
    Sx = [safe_exp(-f) for f in F1]
    c = [mpmath.loggamma((nu + 1) / 2), -mpmath.loggamma(nu / 2), -mpmath.log(nu * mpmath.pi) / 2]
    hn = (nu + 1) / 2
    ve, d0, d1, h0, h1 = Acc(), Acc(), Acc(), Acc(), Acc()
    for r, wi in zip(R, w):
        for f1, s, wj in zip(F1, Sx, w):
            ww = wi * wj
            u = r * r * s / nu
            a = 1 / (1 + u)
            ve.add(ww, c[0], c[1], c[2], -f1 / 2, -hn * mpmath.log1p(u))
            d0.add(ww, (nu + 1) * r * s * a / nu)
            d1.add(ww, -mpf(1) / 2, hn * u * a)
            h0.add(ww / 2, (nu + 1) * s * u * a * a / nu, -(nu + 1) * s * a * a / nu)
            h1.add(ww / 2, -hn * u * a * a)
    return [ve, d0, d1, h0, h1]


# ---------------------------------------------------------------------------------------------- Categorical, 10^(K-1) nodes
def categorical_both(y, m, v, K):
    """Labels 1..K, class K the reference class.  Returns (reference outputs, exact-mode outputs): they differ in dm only -- the
    reference's is the constant (onehot_d - 1) integrated against the weights (quirk Q2), the exact mode's is
    E[onehot_d - softmax_d].  A label outside 1..K gives ve = NaN and zero derivatives."""
    D = K - 1
    x, w = gh(10)
    yv = float(y)
    valid = yv == int(yv) and 1 <= int(yv) <= K
    label = int(yv) if valid else 0
    F = [[_f(mpf(m[k]), mpf(v[k]), xi) for xi in x] for k in range(D)]
    E = [[safe_exp(f) for f in F[k]] for k in range(D)]
    # exp(min(f_d + f_j, LIM_VAL)) for d < j, per pair of node indices
    P2 = {(d, j): [[safe_exp(F[d][a] + F[j][b]) for b in range(10)] for a in range(10)] for d in range(D) for j in range(d + 1, D)}
    ve = Acc()
    dm = [Acc() for _ in range(D)]
    dmx = [Acc() for _ in range(D)]
    dv = [Acc() for _ in range(D)]
    one, zero = mpf(1), mpf(0)
    for idx in itertools.product(range(10), repeat=D):
        ww = one
        for i in idx:
            ww *= w[i]
        for d in range(D):
            dm[d].add(ww, one if label == d + 1 else zero, -one if valid else zero)
        if not valid:
            continue
        e = [E[k][idx[k]] for k in range(D)]
        den = 1 + sum(e)
        p = [clip(ek / den, PLO, PHI) for ek in e] + [clip(1 / den, PLO, PHI)]
        ve.add(ww, mpmath.log(p[label - 1] / sum(p)))
        den2 = safe_square(den)
        for d in range(D):
            num = e[d]
            for j in range(D):
                if j != d:
                    num += P2[(d, j)][idx[d]][idx[j]] if d < j else P2[(j, d)][idx[j]][idx[d]]
            dv[d].add(ww / 2, -num / den2)
            dmx[d].add(ww, one if label == d + 1 else zero, -e[d] / den)
    if not valid:
        ve.r = ve.s = mpf("nan")
    return [ve] + dm + dv, [ve] + dmx + dv


def categorical(y, m, v, K, exact=False):
    return categorical_both(y, m, v, K)[1 if exact else 0]


FAMILIES = dict(Gaussian=gaussian, Bernoulli=bernoulli, HetGaussian=hetgaussian, Poisson=poisson, Exponential=exponential,
                Gamma=gamma, Beta=beta, Student=student, Categorical=categorical)


def _to_f64(x):
    if mpmath.isnan(x):
        return np.nan
    try:
        return float(x)
    except OverflowError:
        return np.inf if x > 0 else -np.inf


def _vec(acc):
    return np.array([_to_f64(a.r) for a in acc]), np.array([_to_f64(a.s) for a in acc])


def row_both(name, y, m, v, **kw):
    """One row in both modes: (R, S, R_exact, S_exact), float64 vectors of length 1 + 2 J (R rounded to nearest; S is a scale).
    Exact mode: Gamma / Beta without quirk Q1 (the float64 pi times the reference's value), Categorical without quirk Q2;
    for every other family the two modes are the same numbers."""
    kw = {k: a for k, a in kw.items() if a is not None}
    if name == "Categorical":
        ref, ex = categorical_both(y, m, v, kw["K"])
    else:
        ref = FAMILIES[name](y, m, v, **kw)
        ex = [a.scaled(PI64) for a in ref] if name in ("Gamma", "Beta") else ref
    return _vec(ref) + _vec(ex)


def var_exp(name, y, m, v, exact=False, **kw):
    """y [N], m, v [N, J] -> R, S [N, 1 + 2 J]."""
    y = np.asarray(y, float).reshape(-1)
    J = dim_f(name, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    out = [row_both(name, float(y[n]), [float(a) for a in m[n]], [float(a) for a in v[n]], **kw) for n in range(y.shape[0])]
    k = 2 if exact else 0
    return np.array([o[k] for o in out]).reshape(-1, 1 + 2 * J), np.array([o[k + 1] for o in out]).reshape(-1, 1 + 2 * J)


# ---------------------------------------------------------------------------------------------- predictive moments
# `<likelihood>.predictive(m, v)` node by node: per output element (the mean of every column, then the variance of every column) the value R
# of the reference's rule and its condition scale S = sum over nodes of weight * sum |addends as the formula writes them|; the variance's S
# includes the subtracted square of the mean.  Student is the closed form of DESIGN 9, NaN / +inf where the moment does not exist.
def _sub_square(var, mean_r, square=lambda a: a * a):
    var.add(1, -square(mean_r))
    return var


def predictive_row(name, m, v, T=20, sigma=0.5, deg_free=5.0, K=None):
    """[mean_0 .., var_0 ..] as Acc of one row; T is the Gauss-Hermite order (unused by Gaussian and Student; Categorical always 10)."""
    m, v = [mpf(a) for a in m], [mpf(a) for a in v]
    mean, var = Acc(), Acc()
    if name == "Gaussian":
        mean.add(1, m[0])
        var.add(1, mpf(float(sigma)) ** 2, v[0])
        return [mean, var]
    if name == "Student":
        nu = mpf(float(deg_free))
        if nu > 1:
            mean.add(1, m[0])
        else:
            mean.r = mean.s = mpf("nan")
        if nu > 2:
            var.add(1, v[0], nu / (nu - 2) * mpmath.exp(m[1] + v[1] / 2))
        else:
            var.r = var.s = mpf("inf")
        return [mean, var]
    if name == "Categorical":
        D = K - 1
        x, w = gh(10)
        E = [[safe_exp(_f(m[k], v[k], xi)) for xi in x] for k in range(D)]
        means = [Acc() for _ in range(D)]
        for idx in itertools.product(range(10), repeat=D):
            ww = mpf(1)
            for i in idx:
                ww *= w[i]
            e = [E[k][idx[k]] for k in range(D)]
            den = 1 + sum(e)
            rho = [clip(ek / den, PLO, PHI) for ek in e]
            rs = sum(rho)
            for d in range(D):
                means[d].add(ww, rho[d] / rs)
        return means + [Acc() for _ in range(D)]              # the reference's variance: zeros
    x, w = gh(T)
    if name == "HetGaussian":
        mean.add(1, m[0])
        for xi, wi in zip(x, w):
            var.add(wi, safe_exp(_f(m[1], v[1], xi)), safe_square(_f(m[0], v[0], xi)))
        return [mean, _sub_square(var, m[0])]
    if name in ("Bernoulli", "Poisson", "Exponential"):
        for xi, wi in zip(x, w):
            f = _f(m[0], v[0], xi)
            if name == "Bernoulli":
                ef = safe_exp(f)
                p = clip(ef / (1 + ef), PLO, PHI)
                mu, vr, ms = p, p * (1 - p), p * p
            elif name == "Poisson":
                ef = safe_exp(f)
                mu, vr, ms = ef, ef, ef * ef
            else:
                b = clip(safe_exp(-f), LO, HI)
                mu, vr, ms = b, safe_square(b), safe_square(b)
            mean.add(wi, mu)
            var.add(wi, vr, ms)
        return [mean, _sub_square(var, mean.r)]
    if name in ("Gamma", "Beta"):                            # quirk Q1: the weight is w_i w_j / pi
        A, B, wq = _tab2(m, v, T)
        for a, wi in zip(A, wq):
            for b, wj in zip(B, wq):
                ww = wi * wj
                if name == "Gamma":
                    mu, vr = a / b, a / (b * b)
                else:
                    mu, vr = a / (a + b), a * b / ((a + b) * (a + b) * (a + b + 1))
                mean.add(ww, mu)
                var.add(ww, vr, mu * mu)
        return [mean, _sub_square(var, mean.r, safe_square)]
    raise KeyError(name)


def predictive_row_f64(name, m, v, T=20, **kw):
    """(R, S, real): float64 vectors of one row, and per element whether the rule's value is a real number (False: NaN / inf by the
    contract itself, Student's missing moments) -- a real value that float64 cannot hold comes back as +-inf in R."""
    kw = {k: a for k, a in kw.items() if a is not None}
    acc = predictive_row(name, m, v, T, **kw)
    R, S = _vec(acc)
    return R, S, np.array([bool(mpmath.isfinite(a.r)) for a in acc])


def predictive(name, m, v, T=20, **kw):
    """m, v [N, J] -> R, S [N, 2 Jp] (Jp = K - 1 for Categorical, else 1): the means, then the variances."""
    J = dim_f(name, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    out = [predictive_row_f64(name, [float(a) for a in m[n]], [float(a) for a in v[n]], T, **kw) for n in range(m.shape[0])]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
