#!/usr/bin/env python
"""Stand-alone timing of the Dirichlet quadrature (10^K-node Gauss-Hermite tensor rule, one wave per row) next to Beta's on
the same rows, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/dirichlet_quad_time.py` (counters not mixed in).
Four one-task models with N rows are evaluated `reps` times each, in this order:
  1. Beta              quad_kernel<7, 0>    the yardstick of K = 2: 100 nodes, lgamma / psi / psi' of the sum per node
  2. Dirichlet K = 2   quad_kernel<10, 2>   the same rows, y -> (y, 1 - y), the same q(f): 100 nodes
  3. Dirichlet K = 3   quad_kernel<10, 3>   1000 nodes
  4. Dirichlet K = 4   quad_kernel<10, 4>   10^4 nodes
The script prints the engine's own event timing of the quadrature per evaluation; in the kernel trace the dispatches of quad_kernel
appear in the same order, `reps` per configuration (`--summarise <kernel_trace.csv>` prints their medians).
usage: python tools/dirichlet_quad_time.py [N=200000] [reps=5]   |   python tools/dirichlet_quad_time.py --summarise kernel_trace.csv [reps=5]"""
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("Beta", "Dirichlet K = 2", "Dirichlet K = 3", "Dirichlet K = 4")


def summarise(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "quad_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    n = len(NAMES)
    assert us and len(us) % (n * reps) == 0, "expected a multiple of %d quad_kernel dispatches, found %d" % (n * reps, len(us))
    c = len(us) // (n * reps)                                  # dispatches per evaluation (row pools)
    ev = np.array(us).reshape(n, reps, c).sum(2)               # per configuration and evaluation
    med = [float(np.median(ev[i])) for i in range(n)]
    for i, name in enumerate(NAMES):
        print("%-16s %-20s median %10.1f us over %d evaluations of %d dispatch(es)   (all: %s)" %
              (name, re.search(r"quad_kernel<[^>]*>", rows[i * reps * c]["Kernel_Name"]).group(0), med[i], reps, c, " ".join("%.1f" % u for u in ev[i])))
    print("ratio to Beta: K = 2 %.2f, K = 3 %.2f, K = 4 %.2f" % (med[1] / med[0], med[2] / med[0], med[3] / med[0]))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import Engine  # noqa: E402
from hetmogp_amd.synthetic import make_case  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
prm2, X, Yb = make_case([("Beta", {})], [N], M=128, Q=1, P=1, seed=3)
for name in NAMES:
    if name == "Beta":
        specs, prm, Y = [("Beta", {})], prm2, Yb
    elif name.endswith("2"):                                   # Beta's rows, parameters and q(f)
        specs, prm, Y = [("Dirichlet", {"K": 2})], prm2, [np.hstack([Yb[0], 1.0 - Yb[0]])]
    else:
        specs = [("Dirichlet", {"K": int(name[-1])})]
        prm, _, Y = make_case(specs, [N], M=128, Q=1, P=1, seed=3)      # (the same X: the generator draws it first)
    e = Engine(specs, 1, 128, 1)
    e.set_data(X, Y)
    for r in range(reps):
        out = e.elbo_grad(**prm)
        ms, _ = e.timings()
        print("%-16s N = %d, M = 128: quadrature %.3f ms, total %.3f ms (engine events)" % (name, N, ms["quadrature"], ms["total"]))
    assert np.isfinite(out["elbo"])
    e.close()
