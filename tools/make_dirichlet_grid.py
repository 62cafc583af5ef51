#!/usr/bin/env python
"""Writes tests/golden/dirgrid.npz: the designed rows of the Dirichlet likelihood with their high-precision values R and
condition scales S from tests/dirichlet_ref_mp.py -- the yardstick of tests/test_dirichlet_cpu.py and tests/test_dirichlet_gpu.py.
Fixed seed, one row at a time: the arrays regenerate bit for bit.

  K [n], y, m, v [n, 4] (NaN beyond K), cls (0 bulk / 1 edge), R, S [n, 9] = ve, dm_0 .. dm_{K-1}, dv_0 .. dv_{K-1} (NaN beyond 1 + 2 K)

bulk = m in [-3, 3], v in [1e-3, 4] (the ranges of DESIGN 9a), y drawn from Dirichlet(c 1), c in {0.05, 1, 20} (parts floored at
1e-300 and renormalised: c = 0.05 underflows); edge = every designed row: m on both sides of the clips of alpha (log 1e9 = 20.72) and
of safe_exp (709.78), v from exactly 0 to 1e4, one alpha 1e18 times the others, all alpha at 1e-9, alpha at digamma's zero, parts of y
from 1e-300 to 1e-6.  K = 4 has few rows: the high-precision rule has 10^4 nodes there.

usage: python tools/make_dirichlet_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dirichlet_ref_mp as dmp  # noqa: E402

MAXK = 4
BULK, EDGE = 0, 1
PSI_ZERO = 1.4616321449683623          # digamma's positive zero
N_BULK = {2: 60, 3: 24, 4: 2}


def _simplex(rng, K, c):
    y = np.maximum(rng.dirichlet(np.full(K, c)), 1e-300)
    return y / y.sum()


def _with_small(K, tiny):
    """A composition whose first part is `tiny`, the rest equal."""
    y = np.full(K, (1.0 - tiny) / (K - 1))
    y[0] = tiny
    return y


def _bulk_rows(rng):
    rows = []
    for K in (2, 3, 4):
        for rep in range(N_BULK[K]):
            c = (0.05, 1.0, 20.0)[rep % 3]
            rows.append((_simplex(rng, K, c), rng.uniform(-3.0, 3.0, K), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), K)), BULK))
    return rows


def _edge_rows(rng):
    rows = []
    for K in (2, 3):
        mid = np.full(K, 1.0 / K)
        # m on both sides of the clips of alpha and of safe_exp, every v from 0 to 1e4
        for j, m0 in enumerate((20.7, 20.75, -20.7, -20.75, 30.0, -30.0, 750.0, -750.0, 0.0)):
            for v0 in (0.0, 1e-12, 1.0, 1e4) if K == 2 else ((0.0, 1e-12, 1.0, 1e4)[j % 4],):     # (K = 3: one v per m, all four in turn)
                m = np.full(K, 0.3)
                m[0] = m0
                v = np.full(K, 0.5)
                v[0] = v0
                rows.append((_simplex(rng, K, 1.0), m, v, EDGE))
        # one alpha 1e18 times the others; all alpha at the lower / upper clip
        for v0 in (0.0, 1.0):
            m = np.full(K, -30.0)
            m[K - 1] = 30.0
            rows.append((_simplex(rng, K, 1.0), m, np.full(K, v0), EDGE))
            rows.append((mid, np.full(K, -30.0), np.full(K, v0), EDGE))
            rows.append((mid, np.full(K, 30.0), np.full(K, v0), EDGE))
        # alpha at digamma's zero (v = 0: every node is m), and next to it
        for v0 in (0.0, 1e-12, 1e-3):
            rows.append((_simplex(rng, K, 1.0), np.full(K, np.log(PSI_ZERO)), np.full(K, v0), EDGE))
            m = np.full(K, -25.0)
            m[0] = np.log(PSI_ZERO)
            rows.append((_simplex(rng, K, 1.0), m, np.full(K, v0), EDGE))
        # a part of y next to the boundary
        for tiny in (1e-300, 1e-100, 1e-30, 1e-12, 1e-6):
            rows.append((_with_small(K, tiny), rng.uniform(-3.0, 3.0, K), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), K)), EDGE))
            rows.append((_with_small(K, tiny), np.full(K, 25.0), np.full(K, 1.0), EDGE))
    K = 4
    rows.append((_with_small(K, 1e-300), np.array([750.0, -750.0, 20.7, -20.7]), np.array([0.0, 1e4, 1.0, 1e-12]), EDGE))
    rows.append((_simplex(rng, K, 1.0), np.array([30.0, -30.0, -30.0, -30.0]), np.full(K, 1.0), EDGE))
    rows.append((_simplex(rng, K, 1.0), np.array([np.log(PSI_ZERO), -25.0, -25.0, -25.0]), np.full(K, 1e-3), EDGE))
    return rows


def build():
    rng = np.random.RandomState(20261017)
    rows = _bulk_rows(rng) + _edge_rows(rng)
    n = len(rows)
    d = dict(K=np.zeros(n, np.int64), y=np.full((n, MAXK), np.nan), m=np.full((n, MAXK), np.nan), v=np.full((n, MAXK), np.nan),
             cls=np.zeros(n, np.uint8), R=np.full((n, 1 + 2 * MAXK), np.nan), S=np.full((n, 1 + 2 * MAXK), np.nan))
    for i, (y, m, v, cls) in enumerate(rows):
        K = len(y)
        d["K"][i], d["cls"][i] = K, cls
        d["y"][i, :K], d["m"][i, :K], d["v"][i, :K] = y, m, v
        d["R"][i, :1 + 2 * K], d["S"][i, :1 + 2 * K] = dmp.row(d["y"][i, :K], d["m"][i, :K], d["v"][i, :K])
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dirgrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows (%d bulk; K = 2 / 3 / 4: %s), %d bytes" %
          (out, len(g["K"]), int((g["cls"] == 0).sum()), " / ".join(str(int((g["K"] == k).sum())) for k in (2, 3, 4)), os.path.getsize(out)))
