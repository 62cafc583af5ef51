#!/usr/bin/env python
"""Writes tests/golden/zipgrid.npz: the designed rows of the zero-inflated Poisson likelihood with their high-precision values
R and condition scales S from tests/zip_ref_mp.py -- the yardstick of tests/test_zip_cpu.py and tests/test_zip_gpu.py.  Fixed seed, one
row at a time: the arrays regenerate bit for bit.

  y [n], m, v [n, 2], cls (0 bulk / 1 edge / 2 clip), R, S [n, 5] = ve, dm_0, dm_1, dv_0, dv_1, lpd [n] (the 20 x 20 log predictive density)

bulk = m in [-3, 3]^2, v log-uniform in [1e-3, 4] (the ranges of DESIGN 9a), y drawn from the model at the row's own mean parameters;
edge = every designed row: y in {0, 1, 32, 1000, 1e6} against f0 in {+-750, 709.78, 400, 355, 37, -37} (lambda^2 past overflow while rho is
already 0; lambda at both ends), f1 in {+-20.7, +-21, +-750} (both sides of pi's clip), u = log(1 - pi) - lambda - log pi at 0, +-1e-9, -40 and
at its upper end 20.72 (the clip keeps it below: +40 does not exist), lambda in {1e-12, 1e-6} (g tiny beside pi), v exactly 0 and 1e4;
clip = the designed rows at which some node of f1 reaches 19 in absolute value, where pi sits at (or within 6e-9 of) a clip: log(1 - pi) and
1 / (1 - pi) at the upper clip set a constant of 2^27 there, as they do for Bernoulli -- a class of their own, as in DESIGN 9l,
so that the figure does not set the constant of the other designed rows.

usage: python tools/make_zip_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zip_ref_mp as zmp  # noqa: E402

BULK, EDGE, CLIP = 0, 1, 2
N_BULK = 100
YS = (0.0, 1.0, 32.0, 1000.0, 1e6)
F0S = (750.0, -750.0, 709.78, 400.0, 355.0, 37.0, -37.0)
F1_CLIP = (20.7, -20.7, 21.0, -21.0, 750.0, -750.0)
V4 = (0.0, 1e-12, 0.3, 1e4)
CLIP_AT = 19.0    # pi within 6e-9 of an end: 1 - pi carries 2^-53 / 6e-9 of itself from the rounding of pi
X_MAX = float(np.polynomial.hermite.hermgauss(20)[0].max())


def _bulk_rows(rng):
    rows = []
    for _ in range(N_BULK):
        m = rng.uniform(-3.0, 3.0, 2)
        v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), 2))
        zero = rng.rand() < 1.0 / (1.0 + np.exp(-m[1]))
        rows.append((0.0 if zero else float(rng.poisson(np.exp(m[0]))), m, v))
    return rows


def _edge_rows():
    A = lambda *a: np.array(a, float)
    rows = []
    n = 0
    for y in YS:                                             # every y against every f0; f1 moderate, all four v in turn
        for f0 in F0S:
            rows.append((y, A(f0, (-2.0, 0.0, 1.5)[n % 3]), A(V4[n % 4], V4[(n // 4) % 4])))
            n += 1
    for f1 in F1_CLIP:                                       # pi at and next to both clips
        for k, y in enumerate((0.0, 1.0, 32.0)):
            rows.append((y, A(0.5, f1), A(0.1, (0.0, 1e-3, 0.0)[k])))
    for f0 in (750.0, -750.0):                               # both functions at their ends
        for f1 in (750.0, -750.0):
            rows.append((0.0, A(f0, f1), A(0.0, 0.0)))
    for du in (0.0, 1e-9, -1e-9):                            # u = -f1 - lambda inside the clip: lambda = 1, f1 = -1 - u
        for v0 in (0.0, 1e-12):
            rows.append((0.0, A(0.0, -1.0 - du), A(v0, 0.0)))
    rows.append((0.0, A(np.log(40.0), 0.0), A(0.0, 0.0)))    # u = -40 (lambda = 40)
    rows.append((0.0, A(np.log(20.0), 20.0), A(0.0, 0.0)))   # u = -40 (lambda = 20, f1 = 20)
    rows.append((0.0, A(-37.0, -750.0), A(0.0, 0.0)))        # u at its upper end, log((1 - 1e-9) / 1e-9) = 20.72
    for lam in (1e-12, 1e-6):                                # g = pi (1 - pi) lambda, tiny beside pi
        for f1 in (-2.0, 1.0, 2.0):                          # (not f1 = 0: there rho - pi = -lambda / 4, the zero crossing of d2/df1^2)
            for vv in (0.0, 1e-3):
                rows.append((0.0, A(np.log(lam), f1), A(vv, vv)))
    for y in (0.0, 3.0, 1e6):                                # v exactly 0 and 1e4 in both dimensions
        rows.append((y, A(1.0, -0.5), A(0.0, 0.0)))
        rows.append((y, A(1.0, -0.5), A(1e4, 1e4)))
    for y in (1000.0, 1e6):                                  # large counts at their own rate
        for f1 in (-2.0, 2.0):
            rows.append((y, A(np.log(y), f1), A(0.3, 0.3)))
            rows.append((y, A(np.log(y), f1), A(0.0, 0.0)))
    return rows


def row_class(m, v):
    """EDGE, or CLIP where some node of f1 reaches CLIP_AT in absolute value."""
    return CLIP if abs(m[1]) + X_MAX * np.sqrt(2.0 * v[1]) >= CLIP_AT else EDGE


def build():
    rng = np.random.RandomState(20261020)
    rows = [r + (BULK,) for r in _bulk_rows(rng)] + [r + (row_class(r[1], r[2]),) for r in _edge_rows()]
    n = len(rows)
    d = dict(y=np.zeros(n), m=np.zeros((n, 2)), v=np.zeros((n, 2)), cls=np.zeros(n, np.uint8), R=np.zeros((n, 5)), S=np.zeros((n, 5)),
             lpd=np.zeros(n))
    for i, (y, m, v, cls) in enumerate(rows):
        d["y"][i], d["m"][i], d["v"][i], d["cls"][i] = y, m, v, cls
        d["R"][i], d["S"][i] = zmp.row(d["y"][i], d["m"][i], d["v"][i])
        d["lpd"][i] = zmp.lpd_row(d["y"][i], d["m"][i], d["v"][i])
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "zipgrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows (%d bulk, %d edge, %d clip), %d bytes" % (out, len(g["y"]), int((g["cls"] == 0).sum()), int((g["cls"] == 1).sum()),
                                                                 int((g["cls"] == 2).sum()), os.path.getsize(out)))
