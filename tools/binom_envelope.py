#!/usr/bin/env python
"""Accuracy envelope of the Beta-Binomial likelihood's 20 x 20 Gauss-Hermite rule and of the Binomial's 20-node rule: each
against an 80-node-per-dimension rule, on the CPU with tests/binom_ref.py, over rows with m in [-1.5, 1.5] per dimension, n uniform in
1 .. 199 and k drawn from the row's own law, for the variances v = 0.1, 0.5 and 2 in every dimension.  Prints, per family and v, the
median / worst |20 - 80| / (1 + |80|) of ve and of the derivatives together.  A property of the model, not a pass criterion.
usage: python tools/binom_envelope.py [rows=200]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import binom_ref as br  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
print("%-12s %5s %5s | %10s %10s | %10s %10s" % ("family", "v", "rows", "ve median", "ve worst", "d median", "d worst"))
for family in ("Binomial", "BetaBinomial"):
    J = br.DIM_F[family]
    rng = np.random.RandomState(7)
    m = rng.uniform(-1.5, 1.5, (N, J))
    n = rng.randint(1, 200, N)
    Y = np.stack([br.draw(rng, family, n, m), n.astype(float)], 1)
    for vv in (0.1, 0.5, 2.0):
        v = np.full((N, J), vv)
        a, f = br.stack(*br.var_exp(family, Y, m, v)), br.stack(*br.var_exp(family, Y, m, v, T=80))
        e = np.abs(a - f) / (1.0 + np.abs(f))
        print("%-12s %5g %5d | %10.1e %10.1e | %10.1e %10.1e" % (family, vv, N, np.median(e[:, 0]), e[:, 0].max(), np.median(e[:, 1:].max(1)),
                                                            e[:, 1:].max()))
