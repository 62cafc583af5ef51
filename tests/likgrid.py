"""Loader of tests/golden/likgrid_*.npz / lik_scales.npz and the element-wise criterion of the likelihood rows:

    |got - R| <= C * 2^-52 * S        for every output element,

R = the 50-digit value of the reference's rule, S = its condition scale (sum over nodes of weight times the absolute values
of the addends; tests/lik_ref_mp.py), both from the fixture -- never an array maximum.  Needs NumPy only.

Constants.  C_ORACLE[(family, mode)][class] = (ve, dm, dv): the largest |oracle - R| / (2^-52 S) of the float64 NumPy oracle
(oracle/lik_student.py for Student) over the committed grids, per output kind and row class, rounded up to the next power of
two -- what plain float64 with libm / SciPy special functions achieves on the reference's formulas.  The two classes are kept
apart (the amplification of the rounding of f = m + sqrt(2 v) x_i by |f| in exp(f), and of the rounding of p by 1 / (1 - p) in
log(1 - p), is NOT folded into S): "bulk" = m in [-3, 3], v in [1e-3, 4]; "edge" = every designed row.  The kernels get
C_KERNEL = max(16, 4 * C_ORACLE): wave-shuffle summation order and special-function series with a stated error of 1-2 ulp.
Measured 2026-10-16 (CPU: NumPy / SciPy; the raw figures are in DESIGN 9a)."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -52
TINY = 2.0 ** -1022               # smallest normal float64
SIZE_BOUND = 1013033              # bytes: the largest fixture committed before the grids (ref_c4_mix_M160.npz)
NONFINITE_SHARE = 0.02
BULK, EDGE = 0, 1

# (family, mode) -> {class: (C_ve, C_dm, C_dv)}: powers of two at or above the measured figure (measured 2026-10-16).  The large
# edge figures are properties of the reference's formulas in float64, not of summation: log(1 - p) and 1 / (1 - p) with p rounded
# next to 1 (Bernoulli, Categorical: 1 / 2^-52 / 1e-9 ~ 2^27), psi(a + b) - psi(b) with a = 1e-9 next to digamma's zero (Beta dm),
# -log(exp(-f)) at |f| ~ 1e-6 (Exponential ve), y - f at a residual of 1e-6 (Student), |f| eps in exp(f) at |f| ~ 700 (Poisson).
C_ORACLE = {
    ("Bernoulli", "reference"): {BULK: (4, 8, 2), EDGE: (2.0 ** 27, 2.0 ** 27, 128)},
    ("Beta", "reference"): {BULK: (1, 2, 1), EDGE: (8, 2.0 ** 27, 8)},
    ("Beta", "exact"): {BULK: (1, 2, 1), EDGE: (8, 2.0 ** 27, 8)},
    ("Categorical", "reference"): {BULK: (8, 1, 8), EDGE: (2.0 ** 28, 1, 256)},
    ("Categorical", "exact"): {BULK: (8, 8, 8), EDGE: (2.0 ** 28, 64, 256)},
    ("Exponential", "reference"): {BULK: (4, 2, 2), EDGE: (131072, 8, 64)},
    ("Gamma", "reference"): {BULK: (4, 4, 4), EDGE: (16, 16, 16)},
    ("Gamma", "exact"): {BULK: (4, 4, 4), EDGE: (16, 16, 16)},
    ("Gaussian", "reference"): {BULK: (2, 1, 1), EDGE: (1, 1, 1)},
    ("HetGaussian", "reference"): {BULK: (4, 2, 2), EDGE: (8, 256, 256)},
    ("Poisson", "reference"): {BULK: (4, 4, 4), EDGE: (128, 128, 128)},
    ("Student", "reference"): {BULK: (8, 8, 8), EDGE: (16, 4096, 16384)},
}
# Kernel elements beyond C_KERNEL that are inherent to the formulation: {(file tag, mode): [(row, column), ...]}; at most 1 % of a
# family's elements, never a bulk row (DESIGN 9a lists each with its measured excess and the reason).
#   beta row 337, dm_1 (a = 1e-9 .. 1.1e-9, b = 1.4616321449683623, digamma's zero; y = 1e-12): every addend psi(.) b vanishes, S = 4.6e-10,
#   while a + b is rounded BEFORE psi: 2^-53 (a + b) psi'(b) b / pi = 7.1e8 in units of 2^-52 S from that rounding alone (the oracle's
#   1.2e8 on this row is the luck of this a + b); the recurrence adds ~1.5e-16 absolute.  Measured 2.11e9 (2026-10-16).
KERNEL_EXCEPTIONS = {("beta", "reference"): [(337, 2)], ("beta", "exact"): [(337, 2)]}


def c_oracle(family, mode="reference"):
    return C_ORACLE[(family, mode)]


def c_kernel(family, mode="reference"):
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE[(family, mode)].items()}


def c_kernel_vs_float64(family, mode="reference"):
    """Bound of the distance between a kernel result and ANOTHER float64 evaluation (the oracle's, or the reference's own output
    in a lik_*.npz fixture) instead of R: each sits within its own constant of the true value, so the two constants add."""
    k, o = c_kernel(family, mode), c_oracle(family, mode)
    return {c: tuple(a + b for a, b in zip(k[c], o[c])) for c in k}


def fixture_classes(n):
    """Row classes of the reference's own fixtures lik_*.npz (oracle/make_golden.py): rows 0-4 are its clip rows, the rest is drawn
    from the bulk ranges."""
    return np.where(np.arange(n) < 5, EDGE, BULK)


def grid_files():
    fs = sorted(glob.glob(os.path.join(GOLDEN, "likgrid_*.npz")))
    assert fs, "no likgrid fixtures"
    return fs


def tag_of(path):
    return os.path.basename(path)[len("likgrid_"):-len(".npz")]


class LikGrid:
    """One grid file.  kw(param) = keyword arguments of var_exp for the rows that share a per-row parameter value."""

    def __init__(self, path):
        g = np.load(path)
        self.tag = tag_of(path)
        self.name, self.kw0, self.param_name, self.groups = json.loads(str(g["spec"]))
        for k in ("y", "m", "v", "param", "R", "S", "cls", "group", "nonfinite"):
            setattr(self, k, g[k])
        self.has_exact = "R_exact" in g.files
        self.R_exact = g["R_exact"] if self.has_exact else self.R
        self.S_exact = g["S_exact"] if self.has_exact else self.S
        self.nonfinite_exact = g["nonfinite_exact"] if self.has_exact else self.nonfinite
        self.n, self.J = self.m.shape

    def kw(self, param):
        kw = dict(self.kw0)
        if self.param_name:
            kw[self.param_name] = float(param)
        return kw

    def param_groups(self, rows=None):
        """[(kw, row indices)]: the rows (all, or the given ones, order kept) split by their per-row parameter."""
        rows = np.arange(self.n) if rows is None else np.asarray(rows)
        if not self.param_name:
            return [(dict(self.kw0), rows)]
        p = self.param[rows]
        return [(self.kw(u), rows[p == u]) for u in np.unique(p)]

    def evaluate(self, fn, rows=None, **extra):
        """fn(name, y, m, v, **kw) -> (ve, dm, dv) on the rows, packed as [n, 1 + 2 J] in the order of `rows`."""
        rows = np.arange(self.n) if rows is None else np.asarray(rows)
        out = np.empty((len(rows), 1 + 2 * self.J))
        pos = {int(r): i for i, r in enumerate(rows)} if len(set(rows.tolist())) == len(rows) else None
        for kw, idx in self.param_groups(rows):
            ve, dm, dv = fn(self.name, self.y[idx], self.m[idx], self.v[idx], **kw, **extra)
            packed = pack(ve, dm, dv, len(idx))
            where = [pos[int(r)] for r in idx] if pos is not None else np.where(np.isin(rows, idx))[0]
            out[where] = packed
        return out

    def col_kind(self):
        """0 / 1 / 2 = ve / dm / dv for each of the 1 + 2 J columns."""
        return np.array([0] + [1] * self.J + [2] * self.J)


def pack(ve, dm, dv, n):
    return np.concatenate([np.reshape(ve, (n, 1)), np.reshape(dm, (n, -1)), np.reshape(dv, (n, -1))], 1)


def classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN."""
    a = np.asarray(a)
    return (np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3).astype(np.uint8)


def ratios(got, R, S, nonfinite):
    """|got - R| / (2^-52 max(S, 2^-1022)) per element: below the smallest normal number float64 is spaced 2^-1074 = 2^-52 * 2^-1022
    absolutely, so C there counts subnormal ulps (a property of the format, the only floor there is).  0 where got == R exactly
    (S may be 0), inf where a finite value was due and got is not finite.  A row the float64 oracle leaves with ANY non-finite
    element overflowed after the reference's own clips: all its elements are NaN here (only their class is asserted)."""
    got, R, S = np.asarray(got, float), np.asarray(R, float), np.asarray(S, float)
    with np.errstate(all="ignore"):
        d = np.abs(got - R)
        r = np.where(d == 0.0, 0.0, d / (EPS * np.maximum(S, TINY)))
    r = np.where(np.isnan(r), np.inf, r)
    return np.where(np.any(nonfinite != 0, axis=1, keepdims=True), np.nan, r)


def worst(r, kind, cls):
    """Largest ratio per (class, output kind): {cls: [ve, dm, dv]}."""
    out = {}
    for c in (BULK, EDGE):
        rows = r[cls == c]
        out[c] = [float(np.nanmax(rows[:, kind == k], initial=0.0)) if rows.size else 0.0 for k in range(3)]
    return out


def assert_rows(got, R, S, nonfinite, kind, cls, C, what, exceptions=()):
    """Every element of a finite row within C[class][kind] * 2^-52 * S; every element of a marked row in the class (finite, +inf,
    -inf, NaN) the float64 oracle gave.  Prints the worst figure per class and output before asserting; returns them."""
    r = ratios(got, R, S, nonfinite)
    for rc in exceptions:
        r[rc] = np.nan
    w = worst(r, kind, cls)
    print("[likgrid] %-44s worst |got - R| / (2^-52 S): bulk ve/dm/dv %s | edge %s" %
          (what, " ".join("%.3g" % a for a in w[BULK]), " ".join("%.3g" % a for a in w[EDGE])))
    bound = np.array([[C[c][k] for k in kind] for c in cls])
    bad = np.argwhere(np.nan_to_num(r, nan=0.0) > bound)
    assert bad.size == 0, (what, "%d elements beyond C" % len(bad),
                           [(int(i), int(j), "cls %d" % cls[i], float(r[i, j]), float(bound[i, j])) for i, j in bad[:8]])
    marked = np.any(nonfinite != 0, axis=1)
    assert np.array_equal(classes(got)[marked], nonfinite[marked]), \
        (what, "non-finite class differs", np.argwhere((classes(got) != nonfinite) & marked[:, None])[:8].tolist())
    return w


def reference_fixtures():
    """The reference's own per-likelihood fixtures lik_<family>.npz (not their side file of scales)."""
    fs = sorted(p for p in glob.glob(os.path.join(GOLDEN, "lik_*.npz")) if os.path.basename(p) != "lik_scales.npz")
    assert fs, "no lik_*.npz fixtures"
    return fs


def fixture_want_and_scale(path):
    """(name, kw, y, m, v, want [n, 1 + 2 J], S, column kinds, row classes) of one lik_<family>.npz and its scales."""
    g = np.load(path)
    name, kw = json.loads(str(g["spec"]))
    want = np.concatenate([g["var_exp"], g["var_exp_dm"], g["var_exp_dv"]], 1)
    J = g["m"].shape[1]
    S = load_scales()[os.path.basename(path)[:-4] + "__S"]
    return name, kw, g["y"], g["m"], g["v"], want, S, np.array([0] + [1] * J + [2] * J), fixture_classes(want.shape[0])


def large_random_cases():
    """The seeded rows of tests/test_gpu_blocks.py::test_var_exp_large_random_vs_oracle: [(name, kw, y, m, v)], n = 3000 each,
    m in [-2, 2], v in [e^-5, e].  Their scales are lik_scales.npz["random__<name>__S"] (float32: a scale needs no more)."""
    rng = np.random.RandomState(5)
    n = 3000
    dims = dict(Bernoulli=1, Poisson=1, Gamma=2, Beta=2, Categorical=3, HetGaussian=2)
    out = []
    for name, kw, y in (("Bernoulli", {}, (rng.rand(n) < 0.4).astype(float)), ("Poisson", {}, rng.poisson(4.0, n).astype(float)),
                        ("Gamma", {}, rng.gamma(2.0, 1.0, n) + 1e-3), ("Beta", {}, np.clip(rng.beta(2, 3, n), 1e-4, 1 - 1e-4)),
                        ("Categorical", {"K": 4}, rng.randint(1, 5, n).astype(float)), ("HetGaussian", {}, rng.randn(n))):
        J = dims[name]
        m, v = rng.uniform(-2, 2, (n, J)), np.exp(rng.uniform(-5, 1, (n, J)))
        out.append((name, kw, y, m, v))
    return out


def load_scales():
    return np.load(os.path.join(GOLDEN, "lik_scales.npz"))
