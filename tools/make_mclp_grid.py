#!/usr/bin/env python
"""Writes tests/golden/mclpgrid.npz: calls of `hmogp_log_predictive` (the Monte-Carlo log predictive density) for every family it
accepts, with the 50-digit estimate R and the condition scale Sc of every row (tests/mclp_ref_mp.py) -- the yardstick of
tests/test_mclp_ref_cpu.py and tests/test_mclp_gpu.py.  Fixed seeds, one row at a time: the arrays regenerate bit for bit.

Per block `tag` (a family under one set of keyword arguments; `spec` = JSON list of [tag, family, kwargs, [[S, seed], ..]]):
  tag__y [n, dim_y], tag__m, tag__v [n, dim_f], tag__cls [n] (0 bulk / 1 edge), tag__call [n] (index into the block's calls; a row's index
  n in its call is its position among the rows of that call), tag__R [n], tag__Sc [n]

Every block has one call per S in (1, 2, 63, 64, 65, 100, 128, 1000), the seeds (0, 1, 2^32, 2^63 + 5) in rotation, a row count that is no
multiple of the 4 rows per block of the kernels, and distinct auxiliary values per row (trial counts, cut points, indicators, shares).
bulk = m in [-3, 3], v log-uniform in [1e-3, 4], y drawn from the model at a draw of q(f);
edge (in the S = 65 call) = v = 0 in one dimension in turn and v > 0 in one dimension in turn (each member of each pair alone), m = +-25
(the links' clips) and +-700 (|f| next to LIM_VAL; Ordinal, which has no exponential link: +-20);
Exponential with y = 1e300: (m, v) = (19, 4) at S = 64 and S = 1000 -- samples with log p = -inf beside finite ones -- and (30, 0) at S = 1
and S = 65 -- every sample -inf, R = -inf.

The generator asserts on the reference: the mixed rows hold both kinds of sample, no sample has |l| / DBL_MAX within 1e-9 of 1 (where
float64 and 50 digits could disagree about -inf), the all--inf rows are exactly -inf, and the whole grid stays within 3e5 sample evaluations.

usage: python tools/make_mclp_grid.py [out.npz] [--measure]     (--measure: no file; prints mclp_ref's figures against the grid)"""
import json
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import binom_ref as br         # noqa: E402
import mclp_ref as mr          # noqa: E402
import mclp_ref_mp as mmp      # noqa: E402
import logpred_ref as lr       # noqa: E402
import zip_ref as zr           # noqa: E402

BULK, EDGE = 0, 1
MAX_EVALUATIONS = 300000
BULK_ROWS = {1: 11, 2: 7, 63: 5, 64: 6, 65: 5, 100: 3, 128: 2, 1000: 2}     # per S; every count is 4k + 1, 4k + 2 or 4k + 3

# (tag, family, kwargs, seed of the bulk rows)
BLOCKS = [
    ("gaussian", "Gaussian", {"sigma": 0.5}, 201), ("bernoulli", "Bernoulli", {}, 202), ("hetgaussian", "HetGaussian", {}, 203),
    ("poisson", "Poisson", {}, 204), ("exponential", "Exponential", {}, 205),
    ("student_nu0.5", "Student", {"deg_free": 0.5}, 206), ("student_nu5", "Student", {"deg_free": 5.0}, 207),
    ("student_nu300", "Student", {"deg_free": 300.0}, 208),
    ("ordinal2", "Ordinal", {"K": 2, "sigma": 1.0}, 209), ("ordinal5", "Ordinal", {"K": 5, "sigma": 1.0}, 210),
    ("ordinal11", "Ordinal", {"K": 11, "sigma": 1.0}, 211),
    ("negbinomial", "NegBinomial", {}, 212), ("weibull", "Weibull", {}, 213), ("binomial", "Binomial", {}, 214),
    ("betabinomial", "BetaBinomial", {}, 215), ("zipoisson", "ZIPoisson", {}, 216),
    ("categorical2", "Categorical", {"K": 2}, 217), ("categorical3", "Categorical", {"K": 3}, 218),
    ("categorical6", "Categorical", {"K": 6}, 219), ("categorical9", "Categorical", {"K": 9}, 220),
    ("dirichlet2", "Dirichlet", {"K": 2}, 221), ("dirichlet3", "Dirichlet", {"K": 3}, 222), ("dirichlet4", "Dirichlet", {"K": 4}, 223),
]


def bulk_rows(name, n, seed, **kw):
    """(y [n, dim_y], m, v [n, J]) of the bulk class."""
    if name in ("Binomial", "BetaBinomial"):
        rng = np.random.RandomState(seed)
        J = br.DIM_F[name]
        m = rng.uniform(-3.0, 3.0, (n, J))
        v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (n, J)))
        trials = np.floor(np.exp(rng.uniform(0.0, np.log(2001.0), n))).clip(1, 2000) + np.arange(n)      # distinct per row
        y = np.stack([br.draw(rng, name, trials, m + np.sqrt(v) * rng.randn(n, J)), trials], 1)
    elif name == "ZIPoisson":
        y, m, v = zr.bulk_rows(np.random.RandomState(seed), n)
    else:
        y, m, v = lr.bulk_rows(name, n, seed, **kw)
    return np.asarray(y, float).reshape(n, mr.dim_y(name, **kw)), m, v


def edge_rows(name, y, m, v, **kw):
    """Edge rows built on the bulk rows (y, m, v) of a call (used in turn)."""
    J = m.shape[1]
    rows = []
    pick = lambda i: (y[i % len(y)].copy(), m[i % len(y)].copy(), v[i % len(y)].copy())   # noqa: E731
    k = 0
    for j in range(J):
        yy, mm, vv = pick(k)
        k += 1
        vv[j] = 0.0                                   # v = 0 in dimension j alone
        rows.append((yy, mm, vv))
        if J > 1:
            yy, mm, vv = pick(k)
            k += 1
            keep = vv[j]
            vv[:] = 0.0
            vv[j] = keep                              # v > 0 in dimension j alone
            rows.append((yy, mm, vv))
    far = 20.0 if name == "Ordinal" else 700.0
    for val, var, dims in ((25.0, 0.1, None), (-25.0, 0.1, None), (far, 0.5, 0), (-far, 0.5, 0), (far, 0.5, J - 1), (-far, 0.5, J - 1)):
        if dims == J - 1 and J == 1:
            continue
        yy, mm, vv = pick(k)
        k += 1
        if dims is None:
            mm[:], vv[:] = val, var
        else:
            mm[dims], vv[dims] = val, var
        rows.append((yy, mm, vv))
    return rows


def rows_of(bi, block):
    """The rows of one block, without their values: (y, m, v, cls, call, calls = [(S, seed), ..])."""
    tag, name, kw, seed = block
    Y, M, V, CLS, CALL, calls = [], [], [], [], [], []
    for ci, S in enumerate(mr.SAMPLE_COUNTS):
        y, m, v = bulk_rows(name, BULK_ROWS[S] + 1, seed + 1000 * ci, **kw)        # (one spare row, to pad a count that is a multiple of 4)
        nb = BULK_ROWS[S]
        rows = [(y[i], m[i], v[i], BULK) for i in range(nb)]
        if S == 65:
            rows += [r + (EDGE,) for r in edge_rows(name, y[:nb], m[:nb], v[:nb], **kw)]
        if name == "Exponential":
            if S in (64, 1000):
                rows.append((np.array([1e300]), np.array([19.0]), np.array([4.0]), EDGE))
            if S in (1, 65):
                rows.append((np.array([1e300]), np.array([30.0]), np.array([0.0]), EDGE))
        if len(rows) % 4 == 0:
            rows.append((y[nb], m[nb], v[nb], BULK))
        assert len(rows) % 4 != 0
        for r in rows:
            Y.append(r[0]), M.append(r[1]), V.append(r[2]), CLS.append(r[3]), CALL.append(ci)
        calls.append((S, mr.SEEDS[(ci + bi) % len(mr.SEEDS)]))
    return np.array(Y, float), np.array(M, float), np.array(V, float), np.array(CLS, np.uint8), np.array(CALL, np.int32), calls


def _value(task):
    name, kw, y, m, v, S, seed, n = task
    yy = float(y[0]) if len(y) == 1 else tuple(float(t) for t in y)
    return mmp.row(name, yy, m, v, S, seed, n, **kw)


def build(blocks=BLOCKS, procs=None):
    d, tasks, where = {}, [], []
    spec = []
    for bi, b in enumerate(blocks):
        tag, name, kw, _ = b
        y, m, v, cls, call, calls = rows_of(bi, b)
        for k, a in (("y", y), ("m", m), ("v", v), ("cls", cls), ("call", call)):
            d["%s__%s" % (tag, k)] = a
        d[tag + "__R"], d[tag + "__Sc"] = np.zeros(len(cls)), np.zeros(len(cls))
        spec.append([tag, name, kw, [[S, seed] for S, seed in calls]])
        for ci, (S, seed) in enumerate(calls):
            for n, i in enumerate(np.flatnonzero(call == ci)):
                tasks.append((name, kw, y[i], m[i], v[i], S, seed, n))
                where.append((tag, i, S))
    evaluations = sum(t[5] for t in tasks)
    assert evaluations <= MAX_EVALUATIONS, evaluations
    order = np.argsort([-t[5] * len(t[3]) for t in tasks])
    with multiprocessing.Pool(procs or min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_value, [tasks[i] for i in order], chunksize=1)
    for i, (R, Sc, n_out, near) in zip(order, res):
        tag, row, S = where[i]
        d[tag + "__R"][row], d[tag + "__Sc"][row] = R, Sc
        assert near > 1e-9, (tag, row, near)                             # no sample next to +-DBL_MAX
        if tag == "exponential" and d[tag + "__y"][row, 0] == 1e300:
            if d[tag + "__v"][row, 0] == 0.0:
                assert n_out == S and R == -np.inf, (tag, row, n_out)     # every sample -inf
            else:
                assert 0 < n_out < S and np.isfinite(R), (tag, row, n_out)   # both kinds of sample
                print("exponential mixed row at S = %d: %d of %d samples have log p = -inf" % (S, n_out, S))
        else:
            assert n_out == 0 and np.isfinite(R), (tag, row, n_out, R)
    d["spec"] = json.dumps(spec)
    return d, evaluations


def measure(path=mr.GRID):
    """mclp_ref against the grid: the raw figures behind mclp_ref.C_ORACLE, per family (the maximum over its blocks)."""
    worst = {}
    for b in mr.load_grid(path):
        cur = worst.setdefault(b.name, {BULK: 0.0, EDGE: 0.0})
        for c in b.calls:
            r = mr.ratios(mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, **b.kw), c)
            for cls in (BULK, EDGE):
                if (c.cls == cls).any():
                    cur[cls] = max(cur[cls], float(r[c.cls == cls].max()))
    up = lambda x: 2.0 ** np.ceil(np.log2(max(x, 1.0)))   # noqa: E731
    for name, w in worst.items():
        print('    "%s": {BULK: %g, EDGE: %g},      # raw %.3g | %.3g' % (name, up(w[BULK]), up(w[EDGE]), w[BULK], w[EDGE]))
    return worst


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--measure" in sys.argv:
        measure(args[0] if args else mr.GRID)
        sys.exit(0)
    out = args[0] if args else mr.GRID
    t0 = time.time()
    g, evaluations = build()
    np.savez_compressed(out, **g)
    print("%s: %d rows in %d blocks, %d sample evaluations, %d bytes, %.0f s" % (
        out, sum(len(g[b[0] + "__cls"]) for b in BLOCKS), len(BLOCKS), evaluations, os.path.getsize(out), time.time() - t0))
