"""Loader of tests/golden/predgrid.npz (tools/make_pred_grid.py) and the element-wise criterion of the predictive moments:

    |got - R| <= C * 2^-52 * max(S, 2^-1022)        for every element (the mean of every column, then the variance of every column),

R = the 50-digit value of the reference's rule, S = its condition scale (tests/lik_ref_mp.py `predictive_row`; the variance's S includes the
subtracted square of the mean).  Rows marked `nf` overflowed in float64 after the reference's own clips: only the class (finite, +inf, -inf,
NaN) of the float64 oracle is asserted there; so it is in the rows marked `ovf` (Categorical: 1 + sum_k exp(f_k) overflows at a node and
float64 goes on with 0 -> clip, every output finite).  An element whose R is NaN / inf by the contract itself (Student's missing moments) is
compared by class as well.  Needs NumPy only.

C_ORACLE_PRED[(family, class)] = (mean, variance): the largest |oracle - R| / (2^-52 max(S, 2^-1022)) of `oracle.likelihoods_oracle.predictive`
(oracle/lik_student.py for Student) over the whole grid, both rule orders, no element left out, rounded up to a power of two.  The
kernels get C = max(16, 4 C_ORACLE_PRED), the rule of DESIGN 9a.  Measured 2026-10-20 against R, never against a kernel (CPU: NumPy; the
raw figures are in DESIGN 9o)."""
import json
import os

import numpy as np

import likgrid as lg

GRID = os.path.join(lg.GOLDEN, "predgrid.npz")
BULK, EDGE = lg.BULK, lg.EDGE
FAMILIES = ("Gaussian", "HetGaussian", "Bernoulli", "Poisson", "Exponential", "Gamma", "Beta", "Student", "Categorical")

# (family, class) -> (C_mean, C_variance), measured 2026-10-20 (worst of both rule orders beside each entry: bulk mean variance | edge).  The
# edge figures are the rounding of f = m + sqrt(2 v) x_i amplified by |f| in exp(f) at |f| up to 700 (Poisson, Exponential, Gamma, Student's
# exp(m_1 + v_1 / 2)), as in DESIGN 9a -- not folded into S; Categorical's grow with K because the oracle adds its 10^(K-1) nodes in one pass.
C_ORACLE_PRED = {
    ("Gaussian", BULK): (1.0, 1.0), ("Gaussian", EDGE): (1.0, 1.0),                      # measured 0 0 | 0 0: m and sigma^2 + v to the bit
    ("HetGaussian", BULK): (1.0, 4.0), ("HetGaussian", EDGE): (1.0, 128.0),              # 0 2.06 | 0 70.3
    ("Bernoulli", BULK): (2.0, 2.0), ("Bernoulli", EDGE): (8.0, 8.0),                    # 1.35 1.39 | 4.77 4.80
    ("Poisson", BULK): (4.0, 16.0), ("Poisson", EDGE): (128.0, 128.0),                   # 2.97 9.12 | 99.3 115
    ("Exponential", BULK): (4.0, 8.0), ("Exponential", EDGE): (64.0, 128.0),             # 2.20 5.99 | 55.5 114
    ("Gamma", BULK): (4.0, 16.0), ("Gamma", EDGE): (64.0, 256.0),                        # 2.77 8.55 | 60.5 133
    ("Beta", BULK): (2.0, 2.0), ("Beta", EDGE): (8.0, 32.0),                             # 1.92 1.74 | 6.69 19.7
    ("Student", BULK): (1.0, 2.0), ("Student", EDGE): (1.0, 256.0),                      # 0 1.88 | 0 251
    ("Categorical_K3", BULK): (8.0, 1.0), ("Categorical_K3", EDGE): (8.0, 1.0),          # 4.75 0 | 5.85 0  (the variance is the reference's zeros)
    ("Categorical_K4", BULK): (32.0, 1.0), ("Categorical_K4", EDGE): (64.0, 1.0),        # 17.7 0 | 45.6 0
    ("Categorical_K5", BULK): (64.0, 1.0), ("Categorical_K5", EDGE): (512.0, 1.0),       # 58.2 0 | 268 0
    ("Categorical_K6", BULK): (512.0, 1.0), ("Categorical_K6", EDGE): (4096.0, 1.0),     # 331 0 | 2422 0
}
# kernel elements beyond C that are inherent to the formulation: {tag: [(T, row, column), ...]} -- none
KERNEL_EXCEPTIONS = {}
# Elements of marked rows where the kernel's class is not the oracle's: {tag: {(T, row, column): class the kernel returns}} (0 finite, 1 +inf,
# 2 -inf, 3 NaN; DESIGN 9o lists the reason).  All of one kind: the variance a1 + a2 - mean^2 where a2 (or a1) or mean^2 overflows.  The oracle
# rounds mean^2 on its own, to +inf, and gets inf - inf = NaN; the compiler contracts the kernel's expression into fma(-mean, mean, a1 + a2),
# inside which the product is exact and finite: an infinity comes out.  Measured on an MI355X 2026-10-20: every element of the grid at which the
# oracle has NaN, and no other.  Never a bulk row; at most 1 % of a family's elements (asserted by tests/test_predgrid_gpu.py).
KERNEL_CLASS_EXCEPTIONS = {
    # m = -30 .. 30 at v = 1e4 and m >= 355 (group `clips`): ef^2 overflows at the outer nodes, a2 = +inf; R = +inf as well.  Kernel +inf.
    "poisson": {(T, r, 1): 1 for T in (10, 20) for r in range(649, 810, 10)},
    # group `safe_square`, m_0 = +-2e154, where m_0^2 = 4e308 overflows.  Rows 946-948 (m_0 > 0: sq = 1.8e308 times the weights' sum): the rule's
    # value is -2.2e308, R = -inf; the kernel has -inf at T = 20 and +inf at T = 10, whose weights sum above 1 so that sq overflows first.
    # Rows 955-957 (m_0 < 0, no clip: every node's square overflows): R is a rounding residue of 1e292, the kernel has +inf.
    "hetgaussian": dict([((T, r, 1), 1) for T in (10, 20) for r in (955, 956, 957)] + [((10, r, 1), 1) for r in (946, 947, 948)] +
                        [((20, r, 1), 2) for r in (946, 947, 948)]),
}


def family_key(g):
    """The key of a grid's constants: the family, Categorical per K (its oracle sums 10^(K-1) nodes in one pass: the figure grows with K)."""
    return "Categorical_K%d" % g.kw0["K"] if g.name == "Categorical" else g.name


def c_oracle(family):
    return {c: C_ORACLE_PRED[(family, c)] for c in (BULK, EDGE)}


def c_kernel(family):
    return {c: tuple(max(16.0, 4.0 * a) for a in C_ORACLE_PRED[(family, c)]) for c in (BULK, EDGE)}


class PredGrid:
    """The rows of one family tag (file tag of the likgrid it was taken from)."""

    def __init__(self, npz, spec, tag):
        self.tag = tag
        self.name, self.kw0, self.param_name, self.groups, self.Ts = spec[tag]
        for k in ("m", "v", "param", "cls", "group", "ovf"):
            setattr(self, k, npz["%s__%s" % (tag, k)])
        self.R = {T: npz["%s__R%d" % (tag, T)] for T in self.Ts}
        self.S = {T: npz["%s__S%d" % (tag, T)] for T in self.Ts}
        self.nf = {T: npz["%s__nf%d" % (tag, T)] for T in self.Ts}
        self.ovf = self.ovf.astype(bool)
        self.n, self.J = self.m.shape
        self.Jp = self.R[self.Ts[0]].shape[1] // 2

    def kw(self, p):
        kw = {k: a for k, a in self.kw0.items() if a is not None}
        if self.param_name:
            kw[self.param_name] = float(p)
        return kw

    def col_kind(self):
        """0 = mean, 1 = variance for each of the 2 Jp columns."""
        return np.array([0] * self.Jp + [1] * self.Jp)

    def evaluate(self, fn, T, rows=None):
        """fn(name, m, v, T, **kw) -> (mean, var) on the rows (all by default), packed [n, 2 Jp] in their order."""
        rows = np.arange(self.n) if rows is None else np.asarray(rows)
        out = np.zeros((len(rows), 2 * self.Jp))
        p = self.param[rows] if self.param_name else np.zeros(len(rows))
        for u in np.unique(p):
            sel = np.where(p == u)[0]
            mean, var = fn(self.name, self.m[rows[sel]], self.v[rows[sel]], T, **self.kw(u))
            out[sel] = np.hstack([np.reshape(mean, (len(sel), -1)), np.reshape(var, (len(sel), -1))])
        return out


def load():
    npz = np.load(GRID)
    spec = json.loads(str(npz["spec"]))
    return {tag: PredGrid(npz, spec, tag) for tag in sorted(spec)}


def oracle_fn(name, m, v, T, **kw):
    from oracle import likelihoods_oracle as lo
    with np.errstate(all="ignore"):
        return lo.predictive(name, m, v, **kw) if T == 0 else lo.predictive(name, m, v, gh_T=T, **kw)


def ratios(got, R, S, nf, ovf=None):
    """|got - R| / (2^-52 max(S, 2^-1022)) per element; NaN (class only) in a marked row (`nf`, or `ovf`: an intermediate overflowed while the
    outputs stayed finite) and where R itself is not finite."""
    got = np.asarray(got, float)
    with np.errstate(all="ignore"):
        d = np.abs(got - R)
        r = np.where(d == 0.0, 0.0, d / (lg.EPS * np.maximum(S, lg.TINY)))
    r = np.where(np.isnan(r), np.inf, r)
    byclass = np.any(nf != 0, axis=1, keepdims=True) | ~np.isfinite(R)
    if ovf is not None:
        byclass = byclass | np.asarray(ovf, bool)[:, None]
    return np.where(byclass, np.nan, r)


def worst(r, kind, cls):
    """{class: [mean, variance]}: the largest ratio."""
    return {c: [float(np.nanmax(r[cls == c][:, kind == k], initial=0.0)) for k in (0, 1)] for c in (BULK, EDGE)}


def assert_rows(g, T, got, C, what, exceptions=(), class_exceptions=None):
    """Every compared element within C[class][kind] 2^-52 max(S, 2^-1022); every other element in the class of the oracle (marked rows) or
    of R (the contract's own NaN / inf).  Prints the worst figures first and returns them."""
    R, S, nf = g.R[T], g.S[T], g.nf[T]
    r = ratios(got, R, S, nf, g.ovf)
    for rc in exceptions:
        r[rc] = np.nan
    kind = g.col_kind()
    w = worst(r, kind, g.cls)
    print("[predgrid] %-40s T = %2d  worst |got - R| / (2^-52 S): bulk mean/var %s | edge %s" %
          (what, T, " ".join("%.3g" % a for a in w[BULK]), " ".join("%.3g" % a for a in w[EDGE])))
    bound = np.array([[C[c][k] for k in kind] for c in g.cls])
    bad = np.argwhere(np.nan_to_num(r, nan=0.0) > bound)
    assert bad.size == 0, (what, T, "%d elements beyond C" % len(bad),
                           [(int(i), int(j), "cls %d" % g.cls[i], float(r[i, j]), float(bound[i, j])) for i, j in bad[:8]])
    marked = np.any(nf != 0, axis=1) | g.ovf            # (an `ovf` row: nf = 0 throughout, every element finite)
    want = np.where(marked[:, None], nf, lg.classes(R))
    byclass = marked[:, None] | ~np.isfinite(R)
    for (r_, c_), cl in (class_exceptions or {}).items():
        assert marked[r_] and want[r_, c_] == 3, (what, T, r_, c_, "a class exception is for an element of a marked row where the oracle has NaN")
        want[r_, c_] = cl
    diff = np.argwhere((lg.classes(got) != want) & byclass)
    assert diff.size == 0, (what, T, "non-finite class differs: (row, column, kernel's class, wanted, class of R)",
                            [(int(i), int(j), int(lg.classes(got)[i, j]), int(want[i, j]), int(lg.classes(R)[i, j])) for i, j in diff])
    return w
