#!/usr/bin/env python
"""Accuracy envelope of the zero-inflated Poisson likelihood's Gauss-Hermite rule: the contract's rule (20 x 20 on rows with
y = 0, 20 + 20 on rows with y >= 1) against the dense 120 x 120 tensor rule, on the CPU with tests/zip_ref.py, over seeded bulk rows
(m in [-3, 3]^2, y drawn from the model at the row's mean parameters) in three bands of v.  Prints, per band and kind of row, the
median / worst |rule - dense| / (1 + |dense|) of ve and of the four derivatives together.  A property of the model, not a pass criterion.
usage: python tools/zip_envelope.py [rows=300]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import zip_ref as zr  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 300
print("%-14s %-6s %5s | %10s %10s | %10s %10s" % ("v in", "rows", "n", "ve median", "ve worst", "d median", "d worst"))
for lo, hi in ((1e-3, 0.1), (0.1, 1.0), (1.0, 4.0)):
    rng = np.random.RandomState(7)
    m = rng.uniform(-3.0, 3.0, (N, 2))
    v = np.exp(rng.uniform(np.log(lo), np.log(hi), (N, 2)))
    y = zr.draw(rng, m[:, 0], m[:, 1])
    a, f = zr.pack(*zr.var_exp(y, m, v)), zr.pack(*zr.var_exp(y, m, v, T=120, tensor=True))
    assert np.allclose(f[:, 0], zr.dense(y, m, v), rtol=0, atol=0)
    e = np.abs(a - f) / (1.0 + np.abs(f))
    for name, sel in (("y = 0", y == 0.0), ("y >= 1", y > 0.0)):
        print("[%5g, %4g] %-6s %5d | %10.1e %10.1e | %10.1e %10.1e" % (lo, hi, name, sel.sum(), np.median(e[sel, 0]), e[sel, 0].max(),
                                                                     np.median(e[sel, 1:].max(1)), e[sel, 1:].max()))
