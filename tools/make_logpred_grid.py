#!/usr/bin/env python
"""Writes tests/golden/lpgrid.npz: rows of every likelihood family with the 50-digit values R = (lpd, ess) and condition scales S of the
deterministic log predictive density (tests/logpred_ref_mp.py) -- the yardstick of tests/test_logpred_cpu.py and
tests/test_logpred_gpu.py.  Fixed seeds, one row at a time: the arrays regenerate bit for bit.

Per block `tag` (a family under one set of keyword arguments; `spec` = JSON list of [tag, family, kwargs]):
  tag__y [n, dim_y], tag__m, tag__v [n, dim_f], tag__cls [n] (0 bulk / 1 edge), tag__R [n, 2] = lpd, ess, tag__S [n]

bulk = m in [-3, 3], v log-uniform in [1e-3, 4], y drawn from the model at a draw of q(f) (logpred_ref.bulk_rows);
edge = the designed rows: v = 0 and 1e-300, f at the links' clips (+-700, the 1e-9 / 1e9 clips), y at the edge of the support, censored and
observed Weibull rows, an end bin and a narrow middle bin of Ordinal, nu = 2.5 and 300 of Student, rows whose ess is next to 1 (a likelihood
much narrower than q(f)), and one Gamma row with y = 0 whose every node has p = 0 (lpd = -inf, ess = NaN).

usage: python tools/make_logpred_grid.py [out.npz] [--measure]     (--measure: no file; prints logpred_ref's figures against the grid)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logpred_ref as lr       # noqa: E402
import logpred_ref_mp as lmp   # noqa: E402

BULK, EDGE = 0, 1
A = lambda *a: np.array(a, float)   # noqa: E731


def _edges1(ys, extra=()):
    """Edge rows of a one-function family: every y against v = 0, v = 1e-300, a wide q(f), and f at +-700."""
    rows = []
    for y in ys:
        rows += [(y, A(0.7), A(0.0)), (y, A(-1.3), A(1e-300)), (y, A(0.4), A(4.0)), (y, A(700.0), A(0.5)), (y, A(-700.0), A(0.5)),
                 (y, A(25.0), A(0.1)), (y, A(-25.0), A(0.1))]
    return rows + list(extra)


def _edges2(ys, extra=()):
    rows = []
    for y in ys:
        rows += [(y, A(0.7, -0.4), A(0.0, 0.0)), (y, A(-1.3, 0.2), A(1e-300, 1e-300)), (y, A(0.3, 0.5), A(0.0, 0.6)),
                 (y, A(0.3, 0.5), A(0.6, 0.0)), (y, A(0.5, 0.2), A(4.0, 4.0)), (y, A(25.0, 25.0), A(0.1, 0.1)),
                 (y, A(-25.0, -25.0), A(0.1, 0.1)), (y, A(0.2, 700.0), A(0.3, 0.5)), (y, A(0.2, -700.0), A(0.3, 0.5))]
    return rows + list(extra)


# (tag, family, kwargs, bulk rows, seed, edge rows)
BLOCKS = [
    ("gaussian", "Gaussian", {"sigma": 0.5}, 48, 101, _edges1([0.3, -40.0])),
    ("bernoulli", "Bernoulli", {}, 48, 102, _edges1([0.0, 1.0])),
    ("hetgaussian", "HetGaussian", {}, 48, 103, _edges2([0.3], [(0.3, A(0.1, -0.5), A(100.0, 0.0)), (5.0, A(0.0, -6.0), A(0.01, 3.0))])),
    ("categorical3", "Categorical", {"K": 3}, 32, 104, _edges2([1.0, 3.0])),
    ("categorical5", "Categorical", {"K": 5}, 0, 105, [(5.0, A(0.3, -0.2, 0.1, 0.5), A(0.5, 1.0, 0.2, 2.0)), (2.0, A(-1.0, 2.0, 0.0, 1.0), A(0.1, 0.3, 0.0, 1e-300)),
                                                        (1.0, A(700.0, 0.0, -700.0, 1.0), A(0.2, 0.2, 0.2, 0.2))]),
    ("poisson", "Poisson", {}, 48, 106, _edges1([0.0, 7.0], [(150.0, A(5.0), A(4.0)), (1e6, A(10.0), A(1.0))])),
    ("exponential", "Exponential", {}, 48, 107, _edges1([1e-300, 2.5, 1e300], [(1e-4, A(5.0), A(4.0))])),
    ("gamma", "Gamma", {}, 48, 108, _edges2([1e-300, 1.7], [(0.0, A(3.0, 0.2), A(0.01, 0.5)), (40.0, A(4.0, 0.0), A(3.0, 0.01))])),
    ("beta", "Beta", {}, 48, 109, _edges2([1e-12, 0.3, 1.0 - 1e-12], [(0.5, A(6.0, 6.0), A(3.0, 3.0))])),
    ("student_nu4", "Student", {"deg_free": 4.0}, 48, 110, _edges2([0.3], [(0.7 + 1e-6, A(0.7, -3.0), A(0.0, 0.2)), (50.0, A(0.2, -0.4), A(0.3, 0.5)), (-50.0, A(0.2, 3.0), A(4.0, 0.0))])),
    ("student_nu2.5", "Student", {"deg_free": 2.5}, 8, 111, _edges2([0.3])),
    ("student_nu300", "Student", {"deg_free": 300.0}, 8, 112, _edges2([0.3])),
    ("ordinal4", "Ordinal", {"K": 4, "sigma": 1.0}, 48, 113, [(y, m, v) for y in (1.0, 2.0, 4.0) for m, v in
                                                              ((A(0.7), A(0.0)), (A(-1.3), A(1e-300)), (A(0.4), A(4.0)), (A(20.0), A(0.5)), (A(-20.0), A(0.5)))]),
    ("ordinal_narrow", "Ordinal", {"bin_edges": [-1.0, 0.0, 1e-3, 1.0], "sigma": 0.7}, 0, 114,
     [(3.0, A(0.0), A(0.0)), (3.0, A(0.3), A(0.5)), (3.0, A(-6.0), A(2.0)), (1.0, A(0.2), A(1.0)), (5.0, A(0.2), A(1.0)), (3.0, A(12.0), A(0.1))]),
    ("dirichlet3", "Dirichlet", {"K": 3}, 24, 115, [((0.2, 0.3, 0.5), A(0.5, -0.2, 0.1), A(0.0, 0.0, 0.0)), ((0.2, 0.3, 0.5), A(0.5, -0.2, 0.1), A(1e-300, 0.5, 0.0)),
                                                    ((1e-9, 0.5, 0.5 - 1e-9), A(1.0, 1.0, 1.0), A(0.5, 0.5, 0.5)), ((0.2, 0.3, 0.5), A(25.0, -25.0, 0.0), A(0.1, 0.1, 0.1)),
                                                    ((0.2, 0.3, 0.5), A(6.0, 6.0, 6.0), A(3.0, 3.0, 3.0))]),
    ("dirichlet4", "Dirichlet", {"K": 4}, 0, 116, [((0.1, 0.2, 0.3, 0.4), A(0.5, -0.2, 0.1, 1.0), A(0.3, 1.0, 0.05, 2.0)),
                                                   ((0.4, 0.3, 0.2, 0.1), A(-1.0, 2.0, 0.0, 0.3), A(0.0, 0.2, 1e-300, 0.7)),
                                                   ((0.25, 0.25, 0.25, 0.25), A(3.0, 3.0, -2.0, 0.0), A(2.0, 0.1, 0.1, 4.0))]),
    ("negbinomial", "NegBinomial", {}, 48, 117, _edges2([0.0, 3.0, 1000.0], [(150.0, A(5.0, 6.0), A(4.0, 0.1))])),
    ("weibull", "Weibull", {}, 48, 118, _edges2([(2.5, 1.0), (2.5, 0.0), (1e-300, 1.0), (1e10, 0.0)], [((150.0, 1.0), A(0.0, 1.5), A(4.0, 0.1)), ((1.0, 1.0), A(0.3, 10.0), A(0.2, 0.0)),
                                                                                                     ((1.0, 0.0), A(0.3, -10.0), A(0.2, 0.0))])),
]


def rows_of(block):
    """The rows of one block, without their values: (y [n, dim_y], m, v [n, J], cls [n])."""
    tag, name, kw, nb, seed, edge = block
    J, dy = lr.dim_f(name, **kw), lr.dim_y(name, **kw)
    if nb:
        y, m, v = lr.bulk_rows(name, nb, seed, **kw)
        y = np.asarray(y, float).reshape(nb, dy)
    else:
        y, m, v = np.zeros((0, dy)), np.zeros((0, J)), np.zeros((0, J))
    ye = np.array([np.ravel(r[0]) for r in edge], float).reshape(len(edge), dy)
    me = np.array([r[1] for r in edge], float).reshape(len(edge), J)
    ve = np.array([r[2] for r in edge], float).reshape(len(edge), J)
    cls = np.concatenate([np.zeros(nb, np.uint8), np.ones(len(edge), np.uint8)])
    return np.concatenate([y, ye]), np.concatenate([m, me]), np.concatenate([v, ve]), cls


def value_of(block, y, m, v):
    """(R [2], S) of one row of the block at 50 digits."""
    name, kw = block[1], block[2]
    yy = float(y[0]) if len(y) == 1 else tuple(float(t) for t in y)
    return lmp.row(name, yy, m, v, **kw)


def build(blocks=BLOCKS):
    d = {"spec": json.dumps([[b[0], b[1], b[2]] for b in blocks])}
    for b in blocks:
        y, m, v, cls = rows_of(b)
        R, S = np.zeros((len(cls), 2)), np.zeros(len(cls))
        for i in range(len(cls)):
            R[i], S[i] = value_of(b, y[i], m[i], v[i])
        for k, a in (("y", y), ("m", m), ("v", v), ("cls", cls), ("R", R), ("S", S)):
            d["%s__%s" % (b[0], k)] = a
    return d


def measure(path=lr.GRID):
    """logpred_ref against the grid: the raw figures behind logpred_ref.C_ORACLE, per family (the maximum over its blocks)."""
    worst = {}
    for b in lr.load_grid(path):
        y = b.y[:, 0] if b.y.shape[1] == 1 else b.y
        a, e = lr.lpd(b.name, y, b.m, b.v, **b.kw)
        big = {c: (np.inf, np.inf) for c in (BULK, EDGE)}
        w = lr.assert_block(a, e, b, big, b.tag)
        cur = worst.setdefault(b.name, {BULK: [0.0, 0.0], EDGE: [0.0, 0.0]})
        for c in (BULK, EDGE):
            cur[c] = [max(cur[c][0], w[c][0]), max(cur[c][1], w[c][1])]
    up = lambda x: 2.0 ** np.ceil(np.log2(max(x, 1.0)))   # noqa: E731
    for name, w in worst.items():
        print('    "%s": {BULK: (%g, %g), EDGE: (%g, %g)},      # raw %.3g %.3g | %.3g %.3g' %
              (name, up(w[0][0]), up(w[0][1]), up(w[1][0]), up(w[1][1]), w[0][0], w[0][1], w[1][0], w[1][1]))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--measure" in sys.argv:
        measure(args[0] if args else lr.GRID)
        sys.exit(0)
    out = args[0] if args else lr.GRID
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows in %d blocks, %d bytes" % (out, sum(len(g[b[0] + "__cls"]) for b in BLOCKS), len(BLOCKS), os.path.getsize(out)))
