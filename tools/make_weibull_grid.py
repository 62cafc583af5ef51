#!/usr/bin/env python
"""Writes tests/golden/wbgrid.npz: the designed rows of the right-censored Weibull likelihood with their high-precision
values R and condition scales S from tests/weibull_ref_mp.py -- the yardstick of tests/test_weibull_cpu.py and
tests/test_weibull_gpu.py.  Fixed seed, one row at a time: the arrays regenerate bit for bit.

  y [n, 2] = (time, event indicator), m, v [n, 2], cls (0 bulk / 1 edge), R, S [n, 5] = ve, dm_0, dm_1, dv_0, dv_1

bulk = m in [-1.5, 1.5]^2, v log-uniform in [1e-3, 0.5]^2, y drawn from the row's own Weibull (scale exp(m0), shape exp(m1)), the
indicator alternating between 1 and 0, and only rows in which no node of the rule reaches the clip of z (a drawn row that does is
drawn again: about one in a hundred);
edge = every designed row, each with delta = 0 and delta = 1: the clip of z at some and at all nodes, the shape k at both clips
(f1 = +-10, +-750), y = 1e-300 and 1e300, v = 0 in either dimension and in both, |m0| = 700, z at and next to 0.

usage: python tools/make_weibull_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import weibull_ref as wr      # noqa: E402  (only to tell whether a drawn row reaches the clip)
import weibull_ref_mp as wmp  # noqa: E402

BULK, EDGE = 0, 1
N_BULK = 256


def _bulk_rows(rng):
    rows = []
    while len(rows) < N_BULK:
        m = rng.uniform(-1.5, 1.5, 2)
        v = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), 2))
        y = float(np.exp(m[0]) * (-np.log(1.0 - rng.rand())) ** np.exp(-m[1]))
        delta = float(1 - len(rows) % 2)
        if y > 0.0 and wr.clipped_nodes(np.array([[y, delta]]), m, v)[0] == 0:
            rows.append((y, delta, m, v, BULK))
    return rows


def _edge_rows():
    rows = []
    A = lambda *a: np.array(a, float)
    for delta in (1.0, 0.0):
        # the clip of z at some nodes (the large k_j and small f0_i), and at every node
        rows.append((50.0, delta, A(0.0, 1.0), A(0.3, 0.3), EDGE))
        rows.append((8.0, delta, A(0.5, 1.4), A(0.5, 0.5), EDGE))
        rows.append((1e10, delta, A(0.0, 5.0), A(0.01, 0.01), EDGE))
        rows.append((3.0, delta, A(-2.0, 8.0), A(0.0, 0.0), EDGE))
        # the shape at both clips, at and beyond safe_exp's clip, with and without a variance
        for m1 in (10.0, -10.0, 750.0, -750.0):
            for v1 in (0.0, 0.1):
                rows.append((1.5, delta, A(0.25, m1), A(0.2, v1), EDGE))
                rows.append((0.999, delta, A(0.0, m1), A(1e-6, v1), EDGE))
        # the smallest and the largest time, against moderate and extreme scales
        for y in (1e-300, 1e300):
            for m0 in (0.0, 700.0, -700.0):
                rows.append((y, delta, A(m0, 0.3), A(0.1, 0.05), EDGE))
            rows.append((y, delta, A(np.log(y), -0.5), A(0.2, 0.2), EDGE))          # ... and z of order one there
        # v = 0 in either dimension, and in both
        for v in (A(0.0, 0.3), A(0.3, 0.0), A(0.0, 0.0)):
            rows.append((2.5, delta, A(0.7, 0.4), v, EDGE))
            rows.append((0.01, delta, A(-1.0, -1.2), v, EDGE))
        # |m0| = 700 with a time of its own size
        for m0 in (700.0, -700.0):
            rows.append((float(np.exp(m0 * 0.99)), delta, A(m0, 0.0), A(0.5, 0.1), EDGE))
            rows.append((1.0, delta, A(m0, -3.0), A(1.0, 0.0), EDGE))
        # z at 0 (y = 1, m0 = 0, v0 = 0: exactly) and next to it
        rows.append((1.0, delta, A(0.0, 0.5), A(0.0, 0.2), EDGE))
        rows.append((1.0 + 1e-9, delta, A(0.0, 0.5), A(0.0, 0.2), EDGE))
        rows.append((float(np.exp(1.0)), delta, A(1.0, 2.0), A(1e-12, 0.0), EDGE))
        rows.append((1.0, delta, A(1e-9, 6.0), A(0.0, 0.01), EDGE))
    return rows


def build():
    rng = np.random.RandomState(20261019)
    rows = _bulk_rows(rng) + _edge_rows()
    n = len(rows)
    d = dict(y=np.zeros((n, 2)), m=np.zeros((n, 2)), v=np.zeros((n, 2)), cls=np.zeros(n, np.uint8), R=np.zeros((n, 5)), S=np.zeros((n, 5)))
    for i, (y, delta, m, v, cls) in enumerate(rows):
        d["y"][i], d["m"][i], d["v"][i], d["cls"][i] = (y, delta), m, v, cls
        d["R"][i], d["S"][i] = wmp.row(y, delta, d["m"][i], d["v"][i])
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "wbgrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows (%d bulk), %d bytes" % (out, len(g["y"]), int((g["cls"] == 0).sum()), os.path.getsize(out)))
