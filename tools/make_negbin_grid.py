#!/usr/bin/env python
"""Writes tests/golden/nbgrid.npz: the designed rows of the Negative Binomial likelihood with their high-precision values R
and condition scales S from tests/negbin_ref_mp.py -- the yardstick of tests/test_negbin_cpu.py and tests/test_negbin_gpu.py.
Fixed seed, one row at a time: the arrays regenerate bit for bit.

  y [n], m, v [n, 2], cls (0 bulk / 1 edge), R, S [n, 5] = ve, dm_0, dm_1, dv_0, dv_1

bulk = m in [-3, 3], v log-uniform in [1e-3, 4] (the ranges of DESIGN 9a), y drawn from the model at the row's own mean parameters;
edge = every designed row: y in {0, 1, 32, 33, 1000, 1e6} (both sides of the switch between the sums and the series), the size r on
both sides of 16 and at both clip ends (f1 = +-21, +-750), r / y in {1e-6, 1, 1e6, 1e9} (where the plain differences of lgamma, psi, psi'
cancel), f0 = +-750, z = f0 - log r at 0 and at +-40 (where the sigmoid saturates), v exactly 0 and 1e4.

usage: python tools/make_negbin_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import negbin_ref_mp as nmp  # noqa: E402

BULK, EDGE = 0, 1
N_BULK = 96
YS = (0.0, 1.0, 32.0, 33.0, 1000.0, 1e6)
RATIOS = (1e-6, 1.0, 1e6, 1e9)
V4 = (0.0, 1e-12, 0.3, 1e4)


def _bulk_rows(rng):
    rows = []
    for _ in range(N_BULK):
        m = rng.uniform(-3.0, 3.0, 2)
        v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), 2))
        r = np.exp(m[1])
        rows.append((float(rng.poisson(np.exp(m[0]) * rng.gamma(r) / r)), m, v, BULK))
    return rows


def _edge_rows():
    rows = []
    # every y against the size on both sides of 16 and at / beyond both clip ends; all four v in turn
    n = 0
    for y in YS:
        for m1 in (np.log(15.9), np.log(16.1), 21.0, -21.0, 750.0, -750.0, 0.0):
            rows.append((y, np.array([np.log(max(y, 0.5)), m1]), np.array([V4[n % 4], V4[(n // 4) % 4]]), EDGE))
            n += 1
    # r / y where the plain differences cancel (and where they do not), at a vanishing and at a small variance
    for y in (1.0, 33.0, 50.0, 1000.0):
        for ratio in RATIOS:
            r = ratio * y
            if r > 1e9:
                continue
            for v1 in (0.0, 1e-3):
                rows.append((y, np.array([np.log(y) + 0.25, np.log(r)]), np.array([0.1, v1]), EDGE))
    rows.append((50.0, np.array([3.0, np.log(1e9)]), np.array([0.0, 0.0]), EDGE))      # the example of the issue: r = 1e9, y = 50
    # f0 at +-750 (beyond safe_exp's clip / a vanishing mean)
    for y in (0.0, 7.0, 1000.0):
        for m0 in (750.0, -750.0):
            rows.append((y, np.array([m0, 2.0]), np.array([0.0 if y < 1000.0 else 1.0, 0.5]), EDGE))
    # z = f0 - log r at 0 (and next to it) and at +-40
    for m1 in (0.0, 10.0, 20.0):
        for dz, v0 in ((0.0, 0.0), (1e-9, 0.0), (0.0, 1e-12), (40.0, 1e-3), (-40.0, 1e-3)):
            rows.append((5.0 if dz <= 0.0 else 40.0, np.array([m1 + dz, m1]), np.array([v0, 0.0]), EDGE))
    # v exactly 0 and 1e4 in both dimensions
    for y in (3.0, 1e6):
        rows.append((y, np.array([1.0, 1.0]), np.array([0.0, 0.0]), EDGE))
        rows.append((y, np.array([1.0, 1.0]), np.array([1e4, 1e4]), EDGE))
    return rows


def build():
    rng = np.random.RandomState(20261019)
    rows = _bulk_rows(rng) + _edge_rows()
    n = len(rows)
    d = dict(y=np.zeros(n), m=np.zeros((n, 2)), v=np.zeros((n, 2)), cls=np.zeros(n, np.uint8), R=np.zeros((n, 5)), S=np.zeros((n, 5)))
    for i, (y, m, v, cls) in enumerate(rows):
        d["y"][i], d["m"][i], d["v"][i], d["cls"][i] = y, m, v, cls
        d["R"][i], d["S"][i] = nmp.row(d["y"][i], d["m"][i], d["v"][i])
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "nbgrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows (%d bulk), %d bytes" % (out, len(g["y"]), int((g["cls"] == 0).sum()), os.path.getsize(out)))
