#!/usr/bin/env python
"""Accuracy envelope of the right-censored Weibull likelihood's 20 x 20 Gauss-Hermite rule: the rule against a 300 x 300
one, on the CPU with tests/weibull_ref.py, over rows with m in [-1.5, 1.5]^2, v log-uniform in [1e-3, 0.5]^2 and y drawn from the
row's own Weibull (every second row censored).  exp(k .) under a Gaussian f1 is a hard integrand once the variance of f1 is large:
the table is by that variance.  Prints, per bin of v1, the rows, the share with a node at the clip of z, and the median / worst
|20 x 20 - 300 x 300| / (1 + |300 x 300|) of ve and of the four derivatives together, with the share of rows that agree to 1e-6.
usage: python tools/weibull_envelope.py [rows=2000]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import weibull_ref as wr  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
rng = np.random.RandomState(7)
m = rng.uniform(-1.5, 1.5, (N, 2))
v = np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, 2)))
Y = wr.draw(rng, m[:, 0], m[:, 1], censored=0.0)
Y[:, 1] = np.arange(N) % 2
clipped = wr.clipped_nodes(Y, m, v) > 0
print("%d rows, %d with at least one node at the clip of z" % (N, clipped.sum()))
err_ve, err_d = np.zeros(N), np.zeros(N)
for b in range(0, N, 50):
    s = slice(b, b + 50)
    ve, dm, dv = wr.var_exp(Y[s], m[s], v[s])
    fe, fm, fv = wr.var_exp(Y[s], m[s], v[s], T=300)
    err_ve[s] = np.abs(ve - fe) / (1.0 + np.abs(fe))
    a, f = np.hstack([dm, dv]), np.hstack([fm, fv])
    err_d[s] = np.max(np.abs(a - f) / (1.0 + np.abs(f)), 1)
edges = [1e-3, 0.01, 0.03, 0.1, 0.2, 0.5]
print("%-16s %5s %8s | %10s %10s %8s | %10s %10s %8s" % ("v1", "rows", "clipped", "ve median", "ve worst", "<= 1e-6", "d median", "d worst", "<= 1e-6"))
for lo, hi in zip(edges[:-1], edges[1:]):
    k = (v[:, 1] >= lo) & (v[:, 1] < hi if hi < 0.5 else v[:, 1] <= hi)
    print("[%-5g, %-5g]   %5d %7.1f%% | %10.1e %10.1e %7.1f%% | %10.1e %10.1e %7.1f%%" % (
        lo, hi, k.sum(), 100.0 * clipped[k].mean(), np.median(err_ve[k]), err_ve[k].max(), 100.0 * np.mean(err_ve[k] <= 1e-6),
        np.median(err_d[k]), err_d[k].max(), 100.0 * np.mean(err_d[k] <= 1e-6)))
