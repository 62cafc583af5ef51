#!/usr/bin/env python
"""Writes tests/golden/bngrid.npz: the designed rows of the Binomial and Beta-Binomial likelihoods with their high-precision
values R and condition scales S from tests/binom_ref_mp.py -- the yardstick of tests/test_binom_cpu.py and tests/test_binom_gpu.py.
Fixed seed, one row at a time: the arrays regenerate bit for bit.

  per family (prefix b_ = Binomial, J = 1; bb_ = BetaBinomial, J = 2):
  y [n, 2] = (k, n), m, v [n, J], cls (0 bulk / 1 edge / 2 clip), R, S [n, 1 + 2 J] = ve, dm_*, dv_*

bulk = m in [-1.5, 1.5] per dimension, v log-uniform in [1e-3, 0.5], n log-uniform in [1, 2000], k from the row's own law at the mean
parameters; edge = every designed row: k = 0 and k = n, n = 1, n = 32 and n = 33 with a + b on both sides of 16 (the three regimes of
nb_gamma_diffs), n = 1e9 with k in {0, 1, 5e8, n}, p at both clips (|m| = 25, v = 0), |m| = 750, a or b at 1e-9 and at 1e9, v = 0 and
1e-300 in either dimension and in both; clip = the Binomial's designed rows with |m| >= 25, where p sits at one of its clips at every node
(log(1 - p) at p = 1e-9 carries the rounding of 1 - p: a class of their own keeps that figure out of the other edge rows' constant).

usage: python tools/make_binom_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binom_ref_mp as bmp  # noqa: E402

BULK, EDGE, CLIP = 0, 1, 2
N_BULK = {"Binomial": 96, "BetaBinomial": 64}
PREFIX = {"Binomial": "b_", "BetaBinomial": "bb_"}
DIM_F = {"Binomial": 1, "BetaBinomial": 2}
COUNTS = ((0, 1), (1, 1), (0, 7), (7, 7), (3, 7), (0, 32), (32, 32), (12, 32), (0, 33), (33, 33), (12, 33), (700, 2000),
          (0, 1e9), (1, 1e9), (5e8, 1e9), (1e9, 1e9))
# Binomial: (m, v) -- a plain row, p at both clips, |m| = 750, v = 0 and 1e-300
B_MV = ((0.3, 0.1), (25.0, 0.0), (-25.0, 0.0), (750.0, 0.2), (-750.0, 0.2), (0.0, 0.0), (0.5, 1e-300), (-1.0, 0.5))
L79, L81 = float(np.log(7.9)), float(np.log(8.1))      # a = b = 7.9: s = 15.8;  8.1: s = 16.2
# Beta-Binomial: (m0, m1, v0, v1) -- s on both sides of 16, a / b beyond both clip ends (exp(+-21) is outside [1e-9, 1e9]), |m| = 750,
# v = 0 and 1e-300 in either dimension and in both
BB_MV = ((L79, L79, 0.0, 0.0), (L81, L81, 0.0, 0.0), (L79, L81, 1e-3, 1e-300), (0.4, -0.3, 0.1, 0.2),
         (-21.0, 0.5, 0.0, 0.1), (21.0, 0.5, 0.1, 0.0), (0.5, -21.0, 1e-300, 0.0), (0.5, 21.0, 0.0, 1e-300),
         (21.0, 21.0, 1e-300, 1e-300), (-21.0, -21.0, 0.0, 0.0), (750.0, -750.0, 0.2, 0.2), (-750.0, 750.0, 0.0, 0.3),
         (21.0, -21.0, 0.05, 0.05))


def _bulk_rows(rng, family):
    J = DIM_F[family]
    rows = []
    for _ in range(N_BULK[family]):
        m = rng.uniform(-1.5, 1.5, J)
        v = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), J))
        n = int(min(max(np.floor(np.exp(rng.uniform(0.0, np.log(2001.0)))), 1), 2000))
        p = 1.0 / (1.0 + np.exp(-m[0])) if family == "Binomial" else rng.beta(np.exp(m[0]), np.exp(m[1]))
        rows.append(((float(rng.binomial(n, p)), float(n)), m, v, BULK))
    return rows


def _edge_rows(family):
    if family == "Binomial":
        return [((float(k), float(n)), np.array([m]), np.array([v]), CLIP if abs(m) >= 25.0 else EDGE) for k, n in COUNTS for m, v in B_MV]
    return [((float(k), float(n)), np.array(q[:2]), np.array(q[2:]), EDGE) for k, n in COUNTS for q in BB_MV]


def rows():
    """{family: [((k, n), m, v, cls)]}: the inputs alone (cheap; both families drawn from one generator, Binomial first)."""
    rng = np.random.RandomState(20261019)
    return {family: _bulk_rows(rng, family) + _edge_rows(family) for family in ("Binomial", "BetaBinomial")}


def build(every=None):
    """The arrays of the fixture.  every = {family: e}: R and S of every e-th row of that family only (the others stay zero) -- what the
    regeneration test recomputes, since a Beta-Binomial row costs 0.17 s at 50 digits."""
    every = every or {}
    d = {}
    for family, rr in rows().items():
        n, J, pre = len(rr), DIM_F[family], PREFIX[family]
        g = dict(y=np.zeros((n, 2)), m=np.zeros((n, J)), v=np.zeros((n, J)), cls=np.zeros(n, np.uint8), R=np.zeros((n, 1 + 2 * J)),
                 S=np.zeros((n, 1 + 2 * J)))
        for i, (y, m, v, cls) in enumerate(rr):
            g["y"][i], g["m"][i], g["v"][i], g["cls"][i] = y, m, v, cls
            if i % every.get(family, 1) == 0:
                g["R"][i], g["S"][i] = bmp.row(family, g["y"][i], g["m"][i], g["v"][i])
        d.update({pre + k: a for k, a in g.items()})
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "bngrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d + %d rows, %d bytes" % (out, len(g["b_cls"]), len(g["bb_cls"]), os.path.getsize(out)))
