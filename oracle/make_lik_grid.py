#!/usr/bin/env python
"""Write tests/golden/likgrid_<family>.npz and tests/golden/lik_scales.npz: designed grids of likelihood rows with their
high-precision values R and condition scales S (tests/lik_ref_mp.py, mpmath) -- the only place besides
tests/test_likgrid_cpu.py that needs mpmath.

    python oracle/make_lik_grid.py [--out DIR] [--jobs N] [--only TAG ...]

Every file: spec (JSON: family, fixed keyword arguments, name of the per-row parameter, group names), y [N], m, v [N, J],
param [N] (sigma / deg_free per row, NaN where the family has none), R, S [N, 1 + 2 J] in the layout
[ve, dm_0.., dv_0..], R_exact / S_exact / nonfinite_exact (the engine's quirks = "exact" mode: Gamma, Beta, Categorical), cls [N]
(0 = bulk, 1 = edge), group [N] (index into the group names), nonfinite [N, 1 + 2 J] (0 finite; 1 / 2 / 3: the float64
oracle returns +inf / -inf / NaN there -- overflow after the reference's own clips; only the class is asserted of these).
Fixed seeds and a per-row evaluation: the arrays regenerate bit for bit, whatever the number of jobs.

Classes.  bulk: m in [-3, 3], v log-uniform in [1e-3, 4], y drawn as oracle/make_golden.py draws it -- the common case.
edge: everything designed -- f = m + sqrt(2 v) x_i on both sides of the probability clip (|f| ~ 20.72), of the [1e-9, 1e9]
clip of exp(f), of safe_exp (709.78), of safe_square; a = exp(f) at digamma's zero (1.4616), at 10 and 12 (the recurrence /
series hand-over of the device's digamma / trigamma), at 1e-9 and 1e9; v from exactly 0 to 1e4; y at its edges; Categorical
rows by path (fast / clipped / den > 1e150 / overflow / one dimension dominating); Student nu on both sides of 64."""
import argparse
import glob
import itertools
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden")
V_EDGE = [0.0, 1e-300, 1e-12, 1e-6, 1e-3, 0.1, 1.0, 4.0, 25.0, 1e4]
LN = np.log
# means that put f (v small) or some node (v large) on each side of every switch of the 1-D and 2-D families
M_EDGE = [-750.0, -709.8, -709.782712893384, -700.0, -30.0, -20.75, float(LN(1e-9)), -20.7, -12.0, -3.0, 0.0,
          float(LN(1.4616321449683623)), 1.0, float(LN(5.0)), float(LN(6.0)), float(np.nextafter(LN(10.0), 0)), float(LN(10.0)) + 1e-9,
          float(LN(12.0)) - 1e-9, float(np.nextafter(LN(12.0), 9)), 12.0, 20.7, float(LN(1e9)), 20.75, 30.0, 700.0, 709.782712893384, 709.8,
          750.0]


def bulk_y(rng, name, n, K=None):
    if name in ("Gaussian", "HetGaussian", "Student"):
        return rng.randn(n) * 1.5
    if name == "Bernoulli":
        return (rng.rand(n) < 0.5).astype(float)
    if name == "Poisson":
        return rng.poisson(3.0, size=n).astype(float)
    if name in ("Gamma", "Exponential"):
        return rng.gamma(2.0, 1.0, size=n) + 1e-3
    if name == "Beta":
        return np.clip(rng.beta(2.0, 3.0, size=n), 1e-4, 1 - 1e-4)
    return rng.randint(1, K + 1, size=n).astype(float)


class Grid:
    def __init__(self, name, J, groups):
        self.name, self.J, self.groups = name, J, list(groups)
        self.rows = []                                  # (y, m tuple, v tuple, param, cls, group)

    def add(self, group, y, m, v, param=np.nan, cls=1):
        m, v = np.broadcast_to(np.asarray(m, float), (self.J,)), np.broadcast_to(np.asarray(v, float), (self.J,))
        self.rows.append((float(y), tuple(map(float, m)), tuple(map(float, v)), float(param), cls, self.groups.index(group)))

    def bulk(self, rng, n, param=None, K=None):
        y = bulk_y(rng, self.name, n, K)
        m = rng.uniform(-3, 3, size=(n, self.J))
        v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), size=(n, self.J)))
        for i in range(n):
            self.add("bulk", y[i], m[i], v[i], np.nan if param is None else param[i % len(param)], cls=0)


def design(tag):
    """The rows of one grid file and its spec."""
    rng = np.random.RandomState(abs(hash_tag(tag)) % (2 ** 31))
    pick = lambda seq: seq[rng.randint(len(seq))]
    if tag in ("bernoulli", "poisson", "exponential", "gaussian"):
        name = tag.capitalize()
        g = Grid(name, 1, ["bulk", "clips", "y_edge"])
        ys = dict(bernoulli=[0.0, 1.0], poisson=[0.0, 1.0, 3.0, 1e6], exponential=[1e-12, 1.0, 1e6],
                  gaussian=[0.0, 1.5, 1e8, -1e8])[tag]
        par = [0.5, 1.0] if tag == "gaussian" else None
        g.bulk(rng, 600, par)
        k = 0
        for mm, vv in itertools.product(M_EDGE, V_EDGE):
            for rep in range(2):
                g.add("clips", ys[k % len(ys)], mm, vv, par[k % 2] if par else np.nan)
                k += 1
        for yy in ys:                                   # every edge y at ordinary moments
            for _ in range(12):
                g.add("y_edge", yy, rng.uniform(-3, 3), np.exp(rng.uniform(np.log(1e-3), np.log(4.0))), pick(par) if par else np.nan)
        return g, [name, {}, "sigma" if par else None]
    if tag == "hetgaussian":
        g = Grid("HetGaussian", 2, ["bulk", "clips", "safe_square", "y_edge"])
        g.bulk(rng, 600)
        m2s = [-750.0, -709.8, -30.0, -20.75, -20.7, -3.0, 0.0, 3.0, 20.7, 20.75, 30.0, 709.8, 750.0]
        for m2, v2 in itertools.product(m2s, V_EDGE):
            for yy in (0.3, 1e8, -1e8):
                if m2 > 700.0 and yy != 0.3:
                    continue                             # exp(-f) subnormal there: not multiplied by 1e8 (its few bits say nothing)
                g.add("clips", yy, [pick([0.0, -2.5] if m2 > 700.0 else [0.0, -2.5, 1e4, 1e8, -1e8]), m2], [pick(V_EDGE), v2])
        for yy, m1 in ((2e154, 0.0), (1.0, 2e154), (-2e154, 1.0), (1.3407807929942596e154, 0.5), (3.0, -2e154)):
            for m2 in (-3.0, 0.0, 30.0):
                g.add("safe_square", yy, [m1, m2], [1.0, 0.1])
        for yy in (1e8, -1e8, 0.0):
            for _ in range(12):
                g.add("y_edge", yy, rng.uniform(-3, 3, 2), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), 2)))
        return g, ["HetGaussian", {}, None]
    if tag in ("gamma", "beta"):
        name = tag.capitalize()
        g = Grid(name, 2, ["bulk", "clips", "handover", "y_edge"])
        ys = [1e-12, 0.7, 1e6, 2.5] if tag == "gamma" else [1e-12, 0.3, 1 - 1e-12, 0.8]
        g.bulk(rng, 600 if tag == "gamma" else 300)
        k = 0
        for mm, vv in itertools.product(M_EDGE, V_EDGE):   # one function on the designed point, the other anywhere on the list
            for dim in (0, 1):
                m, v = [pick(M_EDGE), pick(M_EDGE)], [pick(V_EDGE), pick(V_EDGE)]
                m[dim], v[dim] = mm, vv
                if tag == "beta" and (k % 4):              # a wave-per-row family with three special functions per node: a quarter
                    k += 1
                    continue
                g.add("clips", ys[k % 4], m, v)
                k += 1
        # a, b and a + b on both sides of 10 and 12, at digamma's zero, at the clip bounds: both functions pinned (v tiny)
        pts = [1e-9, 1.4616321449683623, 5.0 - 1e-9, 5.0, 6.0 - 1e-9, 6.0, 10.0 - 1e-9, 10.0, 10.0 + 1e-9, 12.0 - 1e-9, 12.0, 12.0 + 1e-9, 1e9]
        for a, b in itertools.product(pts, pts):
            if tag == "gamma" and rng.rand() < 0.5:
                continue
            g.add("handover", pick(ys), [LN(a), LN(b)], [pick([0.0, 1e-300, 1e-12]), pick([0.0, 1e-12, 1e-6])])
        for yy in ys:
            for _ in range(10):
                g.add("y_edge", yy, rng.uniform(-3, 3, 2), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), 2)))
        return g, [name, {}, None]
    if tag == "student":
        g = Grid("Student", 2, ["bulk", "residual", "clips", "overflow"])
        nus = [0.1, 1.0, 2.0, 5.0, 63.9, 64.0, 64.1, 1e3, 1e8]
        g.bulk(rng, 450, nus)
        for nu in nus:                                   # residuals from 0 to 1e6 scale units, narrow and wide q(f0)
            for res in (0.0, 1e-3, 1.0, 10.0, 1e3, 1e6):
                for m1 in (-2.0, 0.0, 3.0):
                    sc = float(np.exp(0.5 * m1))
                    g.add("residual", 0.25 + res * sc, [0.25, m1], [pick(V_EDGE[:8]), pick(V_EDGE[:8])], nu)
        for nu in nus:
            for m1 in (-709.8, -700.0, -30.0, 30.0, 700.0, 709.8, 750.0):
                for v1 in (0.0, 1e-6, 1.0, 25.0, 1e4):
                    if m1 < -600 or (m1 < 100 and v1 == 1e4) or (m1 > 705.0 and nu > 100.0):
                        continue                         # exp(-f1) r^2 overflows (the overflow group below, by hand), or exp(-f1) is
                                                         # subnormal and multiplied by (nu + 1) / 2: its few bits say nothing
                    g.add("clips", pick([0.0, 1.0, -3.0]), [pick([0.0, 0.5]), m1], [pick(V_EDGE), v1], nu)
        for k, nu in enumerate(nus):                     # u = r^2 s / nu overflows -> inf * 0 in the derivatives
            g.add("overflow", 1e6, [0.0, -750.0], [pick([0.0, 1.0]), 0.0], nu)
        for nu in (1.0, 5.0, 1e3):
            g.add("overflow", 0.5, [0.5, -750.0], [0.0, 0.0], nu)     # r = 0 exactly: u = 0, finite
        return g, ["Student", {}, "deg_free"]
    if tag.startswith("categorical_K"):
        K = int(tag[-1])
        D = K - 1
        nb, ne, nov = {3: (400, 30, 3), 4: (200, 12, 1), 5: (60, 4, 0), 6: (2, 0, 0)}[K]
        g = Grid("Categorical", D, ["bulk", "fast_wide", "clipped", "den_gt_1e150", "near_safe_exp", "dominant", "v_edge",
                                    "safe_exp", "overflow", "bad_label"])
        g.bulk(rng, nb, K=K)
        lab = lambda: rng.randint(1, K + 1)
        ordinary = lambda: (rng.uniform(-3, 3, D), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), D)))
        for _ in range(ne):
            for grp, mm, vv in (("fast_wide", pick([8.0, -8.0, 12.0]), 1.0),      # all nodes inside the admission bound, far from 0
                                ("clipped", pick([20.6, 20.8, -20.6, -20.8, 21.5, -25.0]), pick([0.0, 1e-6, 0.1, 1.0])),
                                ("den_gt_1e150", pick([345.0, 346.0, 350.0, 500.0]), pick([0.0, 0.1, 1.0, 25.0])),
                                ("near_safe_exp", pick([700.0, 705.0]), pick([0.0, 1e-6])),
                                ("dominant", pick([30.0, 60.0, 200.0]), pick([0.1, 1.0, 4.0]))):
                m, v = ordinary()
                if grp == "near_safe_exp":               # every f_j + f_d stays below 709.78: finite in float64
                    m, v = -np.abs(m), np.minimum(v, 0.1)
                d = rng.randint(D)
                m[d], v[d] = mm, vv
                g.add(grp, lab(), m, v)
            m, v = ordinary()
            for d in range(D):
                v[d] = V_EDGE[(rng.randint(10) + 3 * d) % 10]                       # different per latent function
            g.add("v_edge", lab(), m, v)
        if K == 6:                                       # 10^5 nodes a row: one designed row per path that costs the most
            m, v = ordinary()
            m[1], v[1] = 20.8, 1.0
            g.add("clipped", 2, m, v)
            m, v = ordinary()
            m[4], v[4] = 350.0, 0.1
            g.add("den_gt_1e150", 6, m, v)
        for k in range(nov):
            m, v = ordinary()                            # one function beyond safe_exp: e_d + e^{f_j + f_d} overflows in float64
            d = rng.randint(D)
            m[d], v[d] = pick([709.8, 750.0]), pick([0.0, 1.0, 25.0])
            g.add("safe_exp", lab(), m, v)
            m, v = ordinary()                            # two functions beyond safe_exp: den = inf in float64
            m[0], m[D - 1] = 750.0, pick([720.0, 750.0])
            v[0], v[D - 1] = 0.0, pick([0.0, 1e-6])
            g.add("overflow", lab(), m, v)
        if K in (3, 4):
            m, v = ordinary()
            g.add("bad_label", pick([0.0, K + 1.0, 1.5]), m, v)
        return g, ["Categorical", {"K": K}, None]
    raise ValueError(tag)


def hash_tag(tag):
    h = 7
    for c in tag:
        h = (h * 131 + ord(c)) % 1000003
    return h


TAGS = ["gaussian", "bernoulli", "hetgaussian", "poisson", "exponential", "gamma", "beta", "student", "categorical_K3",
        "categorical_K4", "categorical_K5", "categorical_K6"]


def _kw(spec, param):
    kw = dict(spec[1])
    if spec[2]:
        kw[spec[2]] = param
    return kw


def _eval(job):
    import lik_ref_mp
    name, y, m, v, kw = job
    return lik_ref_mp.row_both(name, y, list(m), list(v), **kw)


def oracle_rows(spec, y, m, v, param, exact=False):
    """The float64 oracle on the grid, [N, 1 + 2 J], grouped by the per-row parameter."""
    from oracle import likelihoods_oracle as lo
    out = np.empty((y.shape[0], 1 + 2 * m.shape[1]))
    keys = param if spec[2] else np.zeros_like(param)
    for p in np.unique(keys):
        idx = np.where(keys == p)[0]
        kw = _kw(spec, float(p))
        with np.errstate(all="ignore"):
            ve, dm, dv = lo.var_exp_all(spec[0], y[idx, None], m[idx], v[idx], exact=exact, **kw)
        out[idx] = np.concatenate([np.reshape(ve, (-1, 1)), np.reshape(dm, (len(idx), -1)), np.reshape(dv, (len(idx), -1))], 1)
    return out


def classes(a):
    return (np.isposinf(a) * 1 + np.isneginf(a) * 2 + np.isnan(a) * 3).astype(np.uint8)


def make_grid(tag, out, pool):
    g, spec = design(tag)
    jobs = [(g.name, r[0], r[1], r[2], _kw(spec, r[3])) for r in g.rows]
    res = pool.map(_eval, jobs, chunksize=max(1, min(16, len(jobs) // 64)))
    arr = lambda k: np.array([r[k] for r in res])
    y, m, v = (np.array([r[k] for r in g.rows]) for k in (0, 1, 2))
    param = np.array([r[3] for r in g.rows])
    nonfinite = classes(oracle_rows(spec, y, m, v, param))
    extra = {}
    if g.name in ("Gamma", "Beta", "Categorical"):
        extra = dict(R_exact=arr(2), S_exact=arr(3), nonfinite_exact=classes(oracle_rows(spec, y, m, v, param, exact=True)))
    np.savez_compressed(os.path.join(out, "likgrid_%s.npz" % tag), spec=json.dumps(spec + [g.groups]), y=y, m=m, v=v, param=param,
                        R=arr(0), S=arr(1), cls=np.array([r[4] for r in g.rows], np.uint8),
                        group=np.array([r[5] for r in g.rows], np.uint8), nonfinite=nonfinite, **extra)
    print("likgrid", tag, len(jobs), "rows,", int(np.sum(nonfinite.any(1))), "with a non-finite element", flush=True)


def make_scales(out, pool):
    """R and S of every element of the reference's own fixtures lik_*.npz (which stay as the reference wrote them), and S of
    the seeded random rows of the GPU suite's large-array comparison."""
    d = {}
    for path in sorted(glob.glob(os.path.join(GOLDEN, "lik_*.npz"))):
        if os.path.basename(path) == "lik_scales.npz":
            continue
        f = np.load(path)
        name, kw = json.loads(str(f["spec"]))
        jobs = [(name, float(f["y"][n, 0]), tuple(map(float, f["m"][n])), tuple(map(float, f["v"][n])), kw) for n in range(f["y"].shape[0])]
        res = pool.map(_eval, jobs, chunksize=2)
        key = os.path.basename(path)[:-4]
        d[key + "__R"] = np.array([r[0] for r in res])
        d[key + "__S"] = np.array([r[1] for r in res])
        print("scales", key, flush=True)
    import likgrid
    for name, kw, y, m, v in likgrid.large_random_cases():      # the seeded rows of test_var_exp_large_random_vs_oracle: S only
        res = pool.map(_eval, [(name, float(y[n]), tuple(map(float, m[n])), tuple(map(float, v[n])), kw) for n in range(y.shape[0])],
                       chunksize=8)
        d["random__%s__S" % name] = np.array([r[1] for r in res]).astype(np.float32)
        print("scales random", name, flush=True)
    np.savez_compressed(os.path.join(out, "lik_scales.npz"), **d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    with multiprocessing.Pool(a.jobs) as pool:
        for tag in TAGS:
            if a.only is None or tag in a.only:
                make_grid(tag, a.out, pool)
        if a.only is None or "scales" in a.only:
            make_scales(a.out, pool)


if __name__ == "__main__":
    main()
