#!/usr/bin/env python
"""Writes tests/golden/ordgrid.npz: the designed rows of the Ordinal likelihood with their high-precision values R and
condition scales S from tests/ordinal_ref_mp.py -- the yardstick of tests/test_ordinal_cpu.py and tests/test_ordinal_gpu.py.
Fixed seed, one row at a time: the arrays regenerate bit for bit.

  var_exp rows    y (label), K, edges [n, 10] (NaN beyond K - 1), sigma, m, v, cls (0 bulk / 1 edge), R, S [n, 3] = ve, dm, dv
  predictive rows p_K, p_edges, p_sigma, p_m, p_v, p_R, p_S [n, 2] = mean, variance; p_y, p_logp = closed-form log P_y(m, v)

bulk = m in [-3, 3], v in [1e-3, 4], bin widths (b_k - b_{k-1}) / sigma in [0.25, 4], every label of K in {2, 3, 5, 11};
edge = every designed row: cut points up to 1e3 sigma away on either side (P far below DBL_MIN), v from 0 and 1e-12 to 1e4, bins of
1e-6 .. 1e-2 sigma, sigma in {1e-3, 1e3}, first / last / middle class, f exactly on a cut point (v = 0).

usage: python tools/make_ordinal_grid.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ordinal_ref_mp as omp  # noqa: E402

MAXE = 10
BULK, EDGE = 0, 1


def _bulk_rows(rng):
    rows = []
    for K in (2, 3, 5, 11):
        for label in range(1, K + 1):
            for rep in range(7):
                sigma = (0.5, 1.0, 2.0)[rng.randint(3)]
                widths = np.exp(rng.uniform(np.log(0.25), np.log(4.0), K - 2)) * sigma
                e = np.concatenate([[0.0], np.cumsum(widths)])
                e = e - 0.5 * e[-1] + rng.uniform(-1.0, 1.0)
                rows.append((label, e, sigma, rng.uniform(-3.0, 3.0), float(np.exp(rng.uniform(np.log(1e-3), np.log(4.0)))), BULK))
    return rows


def _edge_rows(rng):
    rows = []
    # cut points far away on either side, first / last / middle class
    for sigma in (1e-3, 1.0, 1e3):
        for dist in (5.0, 30.0, 100.0, 1e3):
            for v in (1e-12, 1e-3, 1.0, 1e4):
                for label, side in ((1, -1.0), (1, 1.0), (3, -1.0), (3, 1.0), (2, -1.0), (2, 1.0)):
                    e = np.array([-0.7, 0.9]) * sigma                      # K = 3; m sits dist sigma below / above the cuts
                    rows.append((label, e, sigma, side * dist * sigma, v * sigma * sigma if v < 1e4 else v, EDGE))
    # narrow middle bins, near and far from m
    for sigma in (1e-3, 1.0, 1e3):
        for width in (1e-6, 1e-4, 1e-2):
            for off in (0.0, 0.5, 3.0, 30.0, -30.0, 1e3):
                for v in (1e-3, 1.0):
                    e = np.array([-2.0, 0.25, 0.25 + width, 2.5]) * sigma    # K = 5, the narrow bin is class 3
                    rows.append((3, e, sigma, (0.25 + off) * sigma, v * sigma * sigma, EDGE))
    # f exactly on a cut point (v = 0: every node is m), and a tiny variance around it
    for sigma in (1e-3, 1.0, 1e3):
        e = np.array([-1.5, -0.5, 0.5, 1.5]) * sigma
        for label in (1, 2, 3, 5):
            for k in range(4):
                for v in (0.0, 1e-12):
                    rows.append((label, e, sigma, float(e[k]), v, EDGE))
    # K = 11 and K = 2 at the extremes of v
    for v in (1e-12, 1e4):
        for label in (1, 6, 11):
            rows.append((label, np.arange(1, 11) - 5.5, 1.0, rng.uniform(-3, 3), v, EDGE))
        for label in (1, 2):
            rows.append((label, np.array([0.0]), 1.0, rng.uniform(-3, 3), v, EDGE))
    return rows


def _pred_rows(rng):
    rows = []
    for K in (2, 3, 5, 11):
        for rep in range(10):
            sigma = (0.3, 1.0, 4.0)[rng.randint(3)]
            e = np.sort(rng.uniform(-3.0, 3.0, K - 1)) * sigma
            e += np.arange(K - 1) * 1e-3 * sigma
            rows.append((e, sigma, rng.uniform(-3.0, 3.0) * sigma, float(np.exp(rng.uniform(np.log(1e-3), np.log(4.0)))) * sigma ** 2))
    for sigma in (1e-3, 1.0, 1e3):                 # one class takes all the mass; huge and tiny v
        e = np.array([-1.0, 0.0, 2.0]) * sigma
        for mm, v in ((-50.0, 1e-6), (60.0, 1e-6), (0.5, 1e-12), (0.5, 1e8), (-1.0, 0.0), (1e3, 1.0)):
            rows.append((e, sigma, mm * sigma, v * sigma * sigma))
    return rows


def build():
    rng = np.random.RandomState(20261016)
    rows = _bulk_rows(rng) + _edge_rows(rng)
    n = len(rows)
    d = dict(y=np.zeros(n), K=np.zeros(n, np.int64), edges=np.full((n, MAXE), np.nan), sigma=np.zeros(n), m=np.zeros(n),
             v=np.zeros(n), cls=np.zeros(n, np.uint8), R=np.zeros((n, 3)), S=np.zeros((n, 3)))
    for i, (label, e, sigma, m, v, cls) in enumerate(rows):
        d["y"][i], d["K"][i], d["sigma"][i], d["m"][i], d["v"][i], d["cls"][i] = label, len(e) + 1, sigma, m, v, cls
        d["edges"][i, :len(e)] = e
        d["R"][i], d["S"][i] = omp.row(*omp.cuts(label, d["edges"][i, :len(e)]), d["sigma"][i], d["m"][i], d["v"][i])
    prow = _pred_rows(rng)
    n = len(prow)
    d.update(p_K=np.zeros(n, np.int64), p_edges=np.full((n, MAXE), np.nan), p_sigma=np.zeros(n), p_m=np.zeros(n), p_v=np.zeros(n),
             p_R=np.zeros((n, 2)), p_S=np.zeros((n, 2)), p_y=np.zeros(n), p_logp=np.zeros(n))
    for i, (e, sigma, m, v) in enumerate(prow):
        d["p_K"][i], d["p_sigma"][i], d["p_m"][i], d["p_v"][i] = len(e) + 1, sigma, m, v
        d["p_edges"][i, :len(e)] = e
        ee = d["p_edges"][i, :len(e)]
        rm, sm, rv, sv = omp.predictive_row(d["p_m"][i], d["p_v"][i], ee, d["p_sigma"][i])
        d["p_R"][i], d["p_S"][i] = (rm, rv), (sm, sv)
        d["p_y"][i] = 1 + rng.randint(len(e) + 1)
        d["p_logp"][i] = omp.log_prob(d["p_y"][i], d["p_m"][i], d["p_v"][i], ee, d["p_sigma"][i])
    return d


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "ordgrid.npz")
    g = build()
    np.savez_compressed(out, **g)
    print("%s: %d var_exp rows (%d bulk), %d predictive rows, %d bytes" %
          (out, len(g["y"]), int((g["cls"] == 0).sum()), len(g["p_m"]), os.path.getsize(out)))
