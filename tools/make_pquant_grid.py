#!/usr/bin/env python
"""Writes tests/golden/pqgrid.npz: rows of the six families of DESIGN 9k with the 50-digit values R = (cdf, sf) and scales S = (S_cdf,
S_sf) of the predictive cdf and survival function (tests/pquant_ref_mp.py) -- the yardstick of tests/test_pquant_cpu.py and
tests/test_pquant_gpu.py.  Fixed seeds, one row at a time: the arrays regenerate bit for bit.

Per block `tag` (a family under one set of keyword arguments; `spec` = JSON list of [tag, family, kwargs]):
  tag__y [n] (values; Ordinal labels; Weibull times), tag__m, tag__v [n, dim_f], tag__cls [n] (0 bulk / 1 edge), tag__R [n, 2], tag__S [n, 2]

bulk = m in [-3, 3], v log-uniform in [1e-3, 4], y drawn from the model at a draw of q(f) (pquant_ref.bulk_rows);
edge = the designed rows: tails whose cdf or sf is below 1e-100 (and still a normal number), v = 0 and 1e-300, y at and below the edge of
the support, f at the links' clips, the end categories and a narrow middle bin of Ordinal, Weibull rows with z at its clip.

usage: python tools/make_pquant_grid.py [out.npz] [--measure]     (--measure: no file; prints pquant_ref's figures against the grid)"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pquant_ref as pq        # noqa: E402
import pquant_ref_mp as pmp    # noqa: E402

BULK, EDGE = 0, 1
A = lambda *a: np.array(a, float)   # noqa: E731

Q1 = [(A(0.7), A(0.0)), (A(-1.3), A(1e-300)), (A(0.4), A(4.0)), (A(2.0), A(0.25))]
Q2 = [(A(0.7, -0.4), A(0.0, 0.0)), (A(-1.3, 0.2), A(1e-300, 1e-300)), (A(0.3, 0.5), A(0.0, 0.6)), (A(0.3, 0.5), A(0.6, 0.0)),
      (A(0.5, 0.2), A(4.0, 4.0))]


def _cross(ys, qs, extra=()):
    return [(y, m, v) for y in ys for m, v in qs] + list(extra)


# (tag, family, kwargs, bulk rows, seed, edge rows)
BLOCKS = [
    ("gaussian", "Gaussian", {"sigma": 0.5}, 40, 201,
     _cross([0.3, -40.0], Q1, [(-12.0, A(0.5), A(0.0)), (13.0, A(0.5), A(0.0)), (-60.0, A(0.7), A(4.0)), (61.0, A(0.7), A(4.0)),
                               (0.7, A(0.7), A(0.0))])),
    ("gaussian_dflt", "Gaussian", {"sigma": None}, 0, 202, _cross([0.3], Q1)),
    ("hetgaussian", "HetGaussian", {}, 40, 203,
     _cross([0.3, 25.0], Q2, [(-200.0, A(0.3, 0.5), A(0.6, 0.3)), (200.0, A(0.3, 0.5), A(0.6, 0.3)), (0.3, A(0.2, 700.0), A(0.3, 0.5)),
                              (0.3, A(0.2, -700.0), A(0.3, 0.5)), (-30.0, A(0.1, 0.0), A(0.0, 0.0)), (0.1, A(0.1, -0.5), A(100.0, 0.0))])),
    ("bernoulli", "Bernoulli", {}, 40, 204,
     _cross([-1.0, -0.0, 0.0, 0.5, 1.0, 2.0], Q1[:3], [(0.0, A(40.0), A(0.1)), (0.0, A(-40.0), A(0.1)), (0.5, A(700.0), A(0.5)),
                                                        (0.5, A(-700.0), A(0.5))])),
    ("exponential", "Exponential", {}, 40, 205,
     _cross([0.0, -1.0, 1e-300, 2.5, 1e300], Q1[:3], [(300.0, A(0.0), A(0.0)), (1e-200, A(0.0), A(0.0)), (400.0, A(0.3), A(0.05)),
                                                      (1e-150, A(0.3), A(2.0)), (2.5, A(700.0), A(0.5)), (2.5, A(-700.0), A(0.5)),
                                                      (1e-4, A(5.0), A(4.0))])),
    ("ordinal4", "Ordinal", {"K": 4, "sigma": 1.0}, 40, 206,
     _cross([1.0, 2.0, 4.0], Q1[:3] + [(A(20.0), A(0.5)), (A(-20.0), A(0.5))], [(1.0, A(25.0), A(0.0)), (3.0, A(-24.0), A(0.0))])),
    ("ordinal_narrow", "Ordinal", {"bin_edges": [-1.0, 0.0, 1e-3, 1.0], "sigma": 0.7}, 0, 207,
     [(3.0, A(0.05), A(0.0)), (3.0, A(0.3), A(0.5)), (2.0, A(-6.0), A(2.0)), (1.0, A(0.2), A(1.0)), (5.0, A(0.2), A(1.0)), (4.0, A(12.0), A(0.1))]),
    ("weibull", "Weibull", {}, 40, 208,
     _cross([0.0, -1.0, 1e-300, 2.5, 1e10], Q2, [(300.0, A(0.0, 0.0), A(0.0, 0.0)), (1e-200, A(0.0, 0.0), A(0.0, 0.0)),
                                                 (300.0, A(0.0, 0.0), A(0.1, 0.1)), (1e-120, A(0.2, 0.3), A(0.5, 0.2)),
                                                 (1e300, A(0.0, 3.0), A(0.0, 0.0)), (1e300, A(0.0, 3.0), A(0.2, 0.2)),
                                                 (1.0, A(0.3, 10.0), A(0.2, 0.0)), (1.0, A(0.3, -10.0), A(0.2, 0.0)),
                                                 (150.0, A(0.0, 1.5), A(4.0, 0.1))])),
]


def rows_of(block):
    """The rows of one block, without their values: (y [n], m, v [n, J], cls [n])."""
    tag, name, kw, nb, seed, edge = block
    J = pq.dim_f(name, **kw)
    if nb:
        y, m, v = pq.bulk_rows(name, nb, seed, **kw)
    else:
        y, m, v = np.zeros(0), np.zeros((0, J)), np.zeros((0, J))
    ye = np.array([r[0] for r in edge], float)
    me = np.array([r[1] for r in edge], float).reshape(len(edge), J)
    ve = np.array([r[2] for r in edge], float).reshape(len(edge), J)
    cls = np.concatenate([np.zeros(nb, np.uint8), np.ones(len(edge), np.uint8)])
    return np.concatenate([y, ye]), np.concatenate([m, me]), np.concatenate([v, ve]), cls


def value_of(block, y, m, v):
    """(R [2], S [2]) of one row of the block at 50 digits."""
    return pmp.row(block[1], float(y), m, v, **block[2])


def build(blocks=BLOCKS):
    d = {"spec": json.dumps([[b[0], b[1], b[2]] for b in blocks])}
    for b in blocks:
        y, m, v, cls = rows_of(b)
        R, S = np.zeros((len(cls), 2)), np.zeros((len(cls), 2))
        for i in range(len(cls)):
            R[i], S[i] = value_of(b, y[i], m[i], v[i])
        for k, a in (("y", y), ("m", m), ("v", v), ("cls", cls), ("R", R), ("S", S)):
            d["%s__%s" % (b[0], k)] = a
    return d


def measure(path=pq.GRID):
    """pquant_ref against the grid: the raw figures behind pquant_ref.C_ORACLE, per family (the maximum over its blocks)."""
    worst = {}
    for b in pq.load_grid(path):
        c, s = pq.cdf_sf(b.name, b.y, b.m, b.v, **b.kw)
        big = {k: (np.inf, np.inf) for k in (BULK, EDGE)}
        w = pq.assert_block(c, s, b, big, b.tag)
        cur = worst.setdefault(b.name, {BULK: [0.0, 0.0], EDGE: [0.0, 0.0]})
        for k in (BULK, EDGE):
            cur[k] = [max(cur[k][0], w[k][0]), max(cur[k][1], w[k][1])]
    up = lambda x: 2.0 ** np.ceil(np.log2(max(x, 1.0)))   # noqa: E731
    for name, w in worst.items():
        print('    "%s": {BULK: (%g, %g), EDGE: (%g, %g)},      # raw %.3g %.3g | %.3g %.3g' %
              (name, up(w[0][0]), up(w[0][1]), up(w[1][0]), up(w[1][1]), w[0][0], w[0][1], w[1][0], w[1][1]))


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--measure" in sys.argv:
        measure(args[0] if args else pq.GRID)
        sys.exit(0)
    out = args[0] if args else pq.GRID
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows in %d blocks, %d bytes" % (out, sum(len(g[b[0] + "__cls"]) for b in BLOCKS), len(BLOCKS), os.path.getsize(out)))
