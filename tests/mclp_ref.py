"""float64 NumPy / SciPy restatement of the Monte-Carlo log predictive density (`hmogp_log_predictive`: `log_predictive_kernel<LIK>` and
`dirichlet_log_predictive_kernel<K>` of csrc/lik_blocks.hip), the loader / criterion of its grid tests/golden/mclpgrid.npz
(tools/make_mclp_grid.py; 50-digit values from tests/mclp_ref_mp.py), the statistics that hold its generator to the normal law, and a
NumPy emulation of the kernel's own (max, sum-exp) update.

  normal_pair(seed, n, s, pair)   `normal_pair` of lik_device.h on uint64 arrays: h = splitmix64(splitmix64(seed ^ n MUL) ^ (s << 8) ^ pair),
                                  h2 = splitmix64(h), u1 = ((h >> 11) + 1) / 2^53, u2 = (h2 >> 11) / 2^53, r = sqrt(-2 log u1),
                                  z0 = r cos(2 pi u2), z1 = r sin(2 pi u2).
                                  The source divides u1 by the literal 9007199254740993.0, which IS 2^53 as a double
                                  (9007199254740993.0 == 2.0**53: 2^53 + 1 is not representable and rounds to even), so u1 lies in (0, 1],
                                  not in the (0, 1) its comment states.  u1 = 1 gives r = 0, z = 0: harmless, and restated as it is.
  estimate(name, y, m, v, S, seed)   f[n, s, j] = m[n, j] + sqrt(v[n, j]) z, z of pair j >> 1 and member j & 1; log p per sample in the
                                  Monte-Carlo forms of `lik_logpdf_sample` (Gaussian ignores sigma, quirk Q6; HetGaussian in its sample
                                  form; Gamma and Beta refused); then -log S + logsumexp_s, samples with log p = -inf contributing nothing and
                                  a row of only such samples giving -inf (the rule of DESIGN 9j for nodes).

Criterion: |got - R| <= C 2^-52 Sc per row, R the 50-digit estimate and
  Sc = 1 + |log S| + sum_s wbar_s (A_s + sum_j |dl_s/df_j| (|m_j| + 4 sqrt(v_j) |z_sj|))
(wbar the normalised exp(l_s), A_s the sum of the absolute addends of log p at sample s).  The derivative term is folded in because the draw
is computed inside the kernel: a few ulps of libm in log / cos / sin reach l through dl/df.

C_ORACLE[family][class]: the largest figure of THIS file against the grid, per family and row class, rounded up to the next power of two
(measured on the CPU, NumPy / SciPy; `python tools/make_mclp_grid.py --measure` prints the raw figures, tests/test_mclp_ref_cpu.py
re-measures them).  The kernels get C_KERNEL = max(16, 4 C_ORACLE)."""
import json
import os
import sys

import numpy as np
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import binom_ref as br             # noqa: E402
import likgrid as lg               # noqa: E402
import logpred_ref as lr           # noqa: E402
import sampler_ref as sr           # noqa: E402
import zip_ref as zr               # noqa: E402

EPS = lg.EPS
BULK, EDGE = lg.BULK, lg.EDGE
GRID = os.path.join(lg.GOLDEN, "mclpgrid.npz")
U64 = np.uint64
_ROWMUL = U64(0xD1342543DE82EF95)
SAMPLE_COUNTS = (1, 2, 63, 64, 65, 100, 128, 1000)
SEEDS = (0, 1, 2 ** 32, 2 ** 63 + 5)
FAMILIES = ("Gaussian", "Bernoulli", "HetGaussian", "Poisson", "Exponential", "Student", "Ordinal", "NegBinomial", "Weibull", "Binomial",
            "BetaBinomial", "ZIPoisson", "Categorical", "Dirichlet")
MC_REFUSED = lr.MC_REFUSED

GENERATOR_CORRUPTIONS = ("pair_ignored", "s_unshifted", "u2_from_h", "z1_is_z0", "row_ignored", "no_two_pi")
COMBINE_CORRUPTIONS = ("no_log_S", "S_round_64", "idle_lanes", "drop_partial_stride", "no_rescale", "stride_N_minus_1")

# family -> {class: C}, measured 2026-10-20 on the CPU (the raw figure beside each constant).  Figures above 1 are properties of the formulas
# in float64 that Sc does not fold in, named on their lines.
C_ORACLE = {
    "Gaussian": {BULK: 1, EDGE: 1},             # raw 0.468 | 0.257
    "Bernoulli": {BULK: 1, EDGE: 1},            # raw 0.758 | 0.111
    "HetGaussian": {BULK: 1, EDGE: 1},          # raw 0.417 | 0.481
    "Poisson": {BULK: 1, EDGE: 1},              # raw 0.528 | 0.216
    "Exponential": {BULK: 1, EDGE: 1},          # raw 0.669 | 0.618
    "Student": {BULK: 256, EDGE: 128},          # raw 143 | 64.9        (nu = 300: oracle/lik_student.logc subtracts two lgammas of ~600,
                                                #  as in logpred_ref.C_ORACLE; the blocks nu = 0.5 and nu = 5 stay below 1)
    "Ordinal": {BULK: 2, EDGE: 1},              # raw 1.21 | 0.147
    "NegBinomial": {BULK: 1, EDGE: 1},          # raw 0.45 | 0.31
    "Weibull": {BULK: 1, EDGE: 1},              # raw 0.566 | 0.572
    "Binomial": {BULK: 1, EDGE: 1},             # raw 0.51 | 0.0415
    "BetaBinomial": {BULK: 1, EDGE: 1},         # raw 0.437 | 0.325
    "ZIPoisson": {BULK: 1, EDGE: 1},            # raw 0.596 | 0.285
    "Categorical": {BULK: 1, EDGE: 1},          # raw 0.667 | 0.618
    "Dirichlet": {BULK: 1, EDGE: 1},            # raw 0.621 | 0.467
}
# {(tag, call, row): cause} of the grid rows the kernels may miss; expected to stay empty
KERNEL_EXCEPTIONS = {}


def c_oracle(family):
    return {c: float(a) for c, a in C_ORACLE[family].items()}


def c_kernel(family):
    return {c: max(16.0, 4.0 * a) for c, a in C_ORACLE[family].items()}


def c_sum(family):
    """Bound between a kernel result and this file's float64 value: each within its own constant of R."""
    k, o = c_kernel(family), c_oracle(family)
    return {c: k[c] + o[c] for c in k}


# ------------------------------------------------------------------------------------------------------------ shapes
def dim_f(name, **kw):
    if name in ("Binomial", "BetaBinomial"):
        return br.DIM_F[name]
    if name == "ZIPoisson":
        return 2
    return lr.dim_f(name, **kw)


def dim_y(name, **kw):
    return 2 if name in ("Binomial", "BetaBinomial") else lr.dim_y(name, **kw)


def _yrows(name, y, **kw):
    dy = dim_y(name, **kw)
    y = np.asarray(y, float)
    return y.reshape(-1) if dy == 1 else y.reshape(-1, dy)


# ------------------------------------------------------------------------------------------------------------ the generator
def _u64(x):
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        x = x.astype(U64)          # (indices and seeds are never negative)
    elif x.dtype != U64:
        x = np.array([int(t) & (2 ** 64 - 1) for t in np.ravel(x)], dtype=U64).reshape(x.shape)
    return x


def normal_pair(seed, n, s, pair, corrupt=None):
    """(z0, z1) of lik_device.h's normal_pair at (seed, row n, sample s, pair), broadcast; every argument an integer or an array of them."""
    assert corrupt is None or corrupt in GENERATOR_CORRUPTIONS
    seed, n, s, pair = np.broadcast_arrays(_u64(seed), _u64(n), _u64(s), _u64(pair))
    with np.errstate(over="ignore"):
        if corrupt == "row_ignored":
            n = n * U64(0)
        if corrupt == "pair_ignored":
            pair = pair * U64(0)
        ss = s if corrupt == "s_unshifted" else s << U64(8)
        h = sr.splitmix64(sr.splitmix64(seed ^ n * _ROWMUL) ^ ss ^ pair)
        h2 = h if corrupt == "u2_from_h" else sr.splitmix64(h)
    u1 = ((h >> U64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)     # (0, 1]: the literal is 2^53
    u2 = (h2 >> U64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)            # [0, 1)
    r = np.sqrt(-2.0 * np.log(u1))
    a = u2 if corrupt == "no_two_pi" else 2.0 * np.pi * u2
    z0 = r * np.cos(a)
    z1 = z0.copy() if corrupt == "z1_is_z0" else r * np.sin(a)
    return z0, z1


def draws(seed, rows, S, J, corrupt=None):
    """z [N, S, J] of the rows `rows` (their indices n in the call): z of function j = member j & 1 of pair j >> 1."""
    rows = np.asarray(rows).reshape(-1, 1, 1)
    s = np.arange(S).reshape(1, -1, 1)
    npair = (J + 1) // 2
    z0, z1 = normal_pair(int(seed), rows, s, np.arange(npair).reshape(1, 1, -1), corrupt)
    z = np.empty((rows.shape[0], S, 2 * npair))
    z[..., 0::2], z[..., 1::2] = z0, z1
    return z[..., :J]


# ------------------------------------------------------------------------------------------------------------ log p at a sample
def _weibull_terms(y, F):
    """Weibull with a real-valued second column (the stride corruption reads a log time where the indicator belongs)."""
    ly, dl = np.log(y[:, 0:1]), y[:, 1:2]
    k = np.clip(lr._safe_exp(F[..., 1]), 1e-3, 1e3)
    z = np.minimum(k * (ly - F[..., 0]), 680.0)
    t = [dl * np.log(k), -dl * ly, dl * z, -np.exp(z)]
    return t[0] + t[1] + t[2] + t[3], sum(np.abs(a) for a in t)


def logpdf_terms(name, y, F, **kw):
    """y the rows, F [N, S, J] -> (log p [N, S], A [N, S] or None where no scale is stated in float64)."""
    with np.errstate(all="ignore"):
        if name in MC_REFUSED:
            raise ValueError("the Monte-Carlo log predictive is not defined for %s" % name)
        if name == "Gaussian":                                   # sigma ignored (quirk Q6)
            d = y[:, None] - F[..., 0]
            t = [np.full(d.shape, -0.5 * np.log(2.0 * np.pi)), -0.5 * d * d]
            return t[0] + t[1], np.abs(t[0]) + np.abs(t[1])
        if name == "HetGaussian":
            f0, f1 = F[..., 0], F[..., 1]
            d = np.minimum(y[:, None] - f0, lr.SQRT_DBL_MAX)             # safe_square clips from above alone
            t = [np.full(f0.shape, -0.5 * np.log(2.0 * np.pi)), -0.5 * f1, -0.5 * (d * d / lr._safe_exp(f1))]
            return (t[0] + t[1]) + t[2], sum(np.abs(a) for a in t)
        if name in ("Binomial", "BetaBinomial"):
            return br.logpdf(name, y, F), None
        if name == "ZIPoisson":
            return zr.logpdf(y, F), None
        if name == "Weibull" and not np.isin(y[:, 1], (0.0, 1.0)).all():
            return _weibull_terms(y, F)
        return lr._logpdf_terms(name, y, F, **kw)


def _lse(l, S_div):
    """-log S_div + logsumexp over axis 1; -inf samples contribute nothing, all -inf -> -inf, a NaN sample -> NaN."""
    with np.errstate(all="ignore"):
        mx = np.max(l, 1, keepdims=True)
        none = np.isneginf(mx)
        e = np.exp(l - np.where(none, 0.0, mx))
        return np.where(none[:, 0], -np.inf, -np.log(float(S_div)) + (mx[:, 0] + np.log(e.sum(1))))


def _stride_corrupt(name, y):
    """The [2][N] image of y read with stride N - 1: row n takes its second value from position (N - 1) + n of the image."""
    assert name == "Weibull", "stated for the Weibull image (log time, indicator)"
    N = y.shape[0]
    img = np.concatenate([np.log(y[:, 0]), y[:, 1]])
    out = y.copy()
    out[:, 1] = img[(N - 1) + np.arange(N)]
    return out


def estimate(name, y, m, v, S, seed, rows=None, corrupt=None, return_parts=False, **kw):
    """The restated estimator, [N].  rows: the rows' indices in the call (default 0 .. N-1).  corrupt: one of GENERATOR_CORRUPTIONS or
    COMBINE_CORRUPTIONS.  return_parts: (estimate, l [N, S], A [N, S], z [N, S, J], F)."""
    assert corrupt is None or corrupt in GENERATOR_CORRUPTIONS + COMBINE_CORRUPTIONS
    J = dim_f(name, **kw)
    y = _yrows(name, y, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    N, S = y.shape[0], int(S)
    rows = np.arange(N) if rows is None else np.asarray(rows)
    if corrupt == "stride_N_minus_1":
        y = _stride_corrupt(name, y)
    S_draw = 64 * ((S + 63) // 64) if corrupt == "idle_lanes" else (64 * (S // 64) if corrupt == "drop_partial_stride" else S)
    z = draws(seed, rows, S_draw, J, corrupt if corrupt in GENERATOR_CORRUPTIONS else None)
    F = m[:, None, :] + np.sqrt(v)[:, None, :] * z
    l, A = logpdf_terms(name, y, F, **kw)
    if corrupt == "no_log_S":
        out = _lse(l, 1)
    elif corrupt == "S_round_64":
        out = _lse(l, 64 * ((S + 63) // 64))
    elif corrupt == "no_rescale":
        out = np.array([kernel_combine(r, S, fixed=True, rescale=False) for r in l])
    elif S_draw == 0:
        out = np.full(N, -np.inf)
    else:
        out = _lse(l, S)
    return (out, l, A, z, F) if return_parts else out


def scale(name, y, m, v, S, seed, rows=None, **kw):
    """Sc [N] in float64 (a scale needs no more): the derivative by a central difference with step 1e-6 max(1, |f|)."""
    out, l, A, z, F = estimate(name, y, m, v, S, seed, rows=rows, return_parts=True, **kw)
    assert A is not None, "no float64 scale is stated for %s" % name
    J = F.shape[2]
    yy = _yrows(name, y, **kw)
    m, v = np.asarray(m, float).reshape(-1, J), np.asarray(v, float).reshape(-1, J)
    with np.errstate(all="ignore"):
        D = np.zeros_like(l)
        for j in range(J):
            h = 1e-6 * np.maximum(1.0, np.abs(F[..., j]))
            Fp, Fm = F.copy(), F.copy()
            Fp[..., j] += h
            Fm[..., j] -= h
            dl = (logpdf_terms(name, yy, Fp, **kw)[0] - logpdf_terms(name, yy, Fm, **kw)[0]) / (2.0 * h)
            D += np.abs(dl) * (np.abs(m[:, None, j]) + 4.0 * np.sqrt(v[:, None, j]) * np.abs(z[..., j]))
        mx = np.max(l, 1, keepdims=True)
        w = np.exp(l - np.where(np.isfinite(mx), mx, 0.0))
        w = w / w.sum(1, keepdims=True)
        return 1.0 + abs(np.log(float(S))) + np.nansum(np.where(w > 0.0, w * (A + D), 0.0), 1)


# ------------------------------------------------------------------------------------------------------------ the kernel's own update
def kernel_combine(l, S, fixed, rescale=True):
    """The kernels' combination of the S values l[s] in the kernels' order: sample s in lane s & 63, the per-lane (max, sum-exp) update, the
    five-step butterfly with its -inf guards, -log S + mx + log se.  fixed=False: the update before DESIGN 9q's fix (a first sample with
    l = -inf computes exp(-inf - -inf) = exp(NaN), and the butterfly's `mx == -inf ? 0` guard swallows the NaN of a lane that saw only NaN
    samples); fixed=True: a sample with l = -inf leaves (mx, se) untouched, and the butterfly keeps the sum of a lane whose maximum is the
    new maximum as it is (an empty lane's 0, a NaN lane's NaN) instead of replacing it by 0."""
    l = np.asarray(l, float)
    mx, se = np.full(64, -np.inf), np.zeros(64)
    with np.errstate(all="ignore"):
        for lane in range(64):
            for s in range(lane, int(S), 64):
                x = l[s]
                if fixed and x == -np.inf:
                    continue
                if x > mx[lane]:
                    se[lane] = (se[lane] * np.exp(mx[lane] - x) if rescale else se[lane]) + 1.0
                    mx[lane] = x
                else:
                    se[lane] += np.exp(x - mx[lane])
        o = 32
        while o > 0:
            idx = np.arange(64) ^ o
            omx, ose = mx[idx], se[idx]
            nm = np.fmax(mx, omx)
            if fixed:
                se = np.where(mx == nm, se, se * np.exp(mx - nm)) + np.where(omx == nm, ose, ose * np.exp(omx - nm))
            else:
                se = np.where(mx == -np.inf, 0.0, se * np.exp(mx - nm)) + np.where(omx == -np.inf, 0.0, ose * np.exp(omx - nm))
            mx = nm
            o >>= 1
        return -np.log(float(S)) + mx[0] + np.log(se[0])


# ------------------------------------------------------------------------------------------------------------ the generator's law
N_DRAWS = 200000
P_MIN = 1e-6
MAX_STATISTICS = 1000
N_STATISTICS = [0]


def _count(p, counted):
    if counted:
        N_STATISTICS[0] += 1
        assert N_STATISTICS[0] <= MAX_STATISTICS, "more than %d statistics: the family-wise level no longer holds" % MAX_STATISTICS
    return float(p)


def _pit(z, counted, bins=64):
    u = stats.norm.cdf(np.asarray(z, float))
    if not np.all(np.isfinite(u)):
        return {"chi2": _count(0.0, counted), "ks": _count(0.0, counted)}
    cnt = np.bincount(np.minimum((u * bins).astype(np.int64), bins - 1), minlength=bins)
    return {"chi2": _count(stats.chisquare(cnt).pvalue, counted), "ks": _count(stats.kstest(u, "uniform").pvalue, counted)}


def _lag(a, b, counted):
    """|r| sqrt(N) of the correlation of a with b against the normal law.  Perfect dependence (no spread left) is p = 0."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    if a.std() < 1e-9 or b.std() < 1e-9:
        return _count(0.0, counted)
    r = np.corrcoef(a, b)[0, 1]
    return _count(2.0 * stats.norm.sf(abs(r) * np.sqrt(a.size)), counted)


def generator_statistics(seed, pair, corrupt=None, D=N_DRAWS, pair_of=None):
    """{statistic: p} of one (seed, pair).  `pair_of(seed, n, s, pair) -> (z0, z1)` replaces the restatement (the device's draws)."""
    counted = corrupt is None
    gen = pair_of or (lambda sd, n, s, p: normal_pair(sd, n, s, p, corrupt))
    n, zero = np.arange(D), np.zeros(D, dtype=np.int64)
    out = {}
    a0, a1 = gen(seed, n, zero, pair)                         # across rows at sample 0
    for k, z in (("rows z0", a0), ("rows z1", a1)):
        for t, p in _pit(z, counted).items():
            out["%s %s" % (k, t)] = p
    out["z0 ~ z1"] = _lag(a0, a1, counted)
    out["z0^2 ~ z1^2"] = _lag(a0 * a0, a1 * a1, counted)
    out["row n ~ n+1"] = _lag(a0[:-1], a0[1:], counted)
    out["sample 0 ~ 1"] = _lag(a0, gen(seed, n, zero + 1, pair)[0], counted)
    out["sample 0 ~ 64"] = _lag(a0, gen(seed, n, zero + 64, pair)[0], counted)
    b0 = gen(seed, n, zero, pair + 1)[0]
    out["pair p ~ p+1"] = _lag(a0, b0, counted)
    out["(s, p+1) ~ (s+1, p)"] = _lag(b0, gen(seed, n, zero + 1, pair)[0], counted)
    out["seed ~ seed+1"] = _lag(a0, gen(seed + 1, n, zero, pair)[0], counted)
    c0, c1 = gen(seed, zero + 3, n, pair)                     # within one row over the samples
    for k, z in (("samples z0", c0), ("samples z1", c1)):
        for t, p in _pit(z, counted).items():
            out["%s %s" % (k, t)] = p
    out["sample s ~ s+1"] = _lag(c0[:-1], c0[1:], counted)
    out["sample s ~ s+64"] = _lag(c0[:-64], c0[64:], counted)
    return out


# ------------------------------------------------------------------------------------------------------------ the grid
class Call:
    """One call of the grid: rows n = 0 .. N-1 of one family under one (S, seed)."""

    def __init__(self, b, i, S, seed, rows):
        self.block, self.index, self.S, self.seed, self.rows = b, i, int(S), int(seed), rows
        for k in ("y", "m", "v", "cls", "R", "Sc"):
            setattr(self, k, getattr(b, k)[rows])
        self.n = len(rows)

    def y_arg(self):
        return self.y[:, 0] if self.y.shape[1] == 1 else self.y


class Block:
    """One block of mclpgrid.npz: the calls of one family under one set of keyword arguments."""

    def __init__(self, g, tag, name, kw, calls):
        self.tag, self.name, self.kw = tag, name, kw
        for k in ("y", "m", "v", "cls", "R", "Sc", "call"):
            setattr(self, k, g["%s__%s" % (tag, k)])
        self.calls = [Call(self, i, S, int(seed), np.flatnonzero(self.call == i)) for i, (S, seed) in enumerate(calls)]


def load_grid(path=GRID):
    g = np.load(path)
    return [Block(g, tag, name, kw, calls) for tag, name, kw, calls in json.loads(str(g["spec"]))]


def ratios(got, c):
    """|got - R| / (2^-52 Sc) per row of a call; rows whose R is -inf (or NaN) must be equal and give 0, else +inf."""
    got = np.asarray(got, float)
    with np.errstate(all="ignore"):
        r = np.abs(got - c.R) / (EPS * c.Sc)
    nf = ~np.isfinite(c.R)
    same = (got == c.R) | (np.isnan(got) & np.isnan(c.R))
    r[nf] = np.where(same[nf], 0.0, np.inf)
    r[~nf & ~np.isfinite(got)] = np.inf
    return r


def assert_call(got, c, C, what, exceptions=()):
    """The criterion on one call; prints and returns the worst figure per class.  exceptions: rows of the call left out."""
    r = ratios(got, c)
    keep = np.ones(c.n, bool)
    keep[list(exceptions)] = False
    worst = {}
    for cls in (BULK, EDGE):
        sel = keep & (c.cls == cls)
        worst[cls] = float(r[sel].max()) if sel.any() else 0.0
        bad = np.flatnonzero(sel & ~(r <= C[cls]))
        assert bad.size == 0, "%s: rows %s of call %d (S = %d, seed = %d) miss C = %g: ratios %s, got %s, R %s" % (
            what, bad.tolist(), c.index, c.S, c.seed, C[cls], r[bad].tolist(), np.asarray(got)[bad].tolist(), c.R[bad].tolist())
    return worst
