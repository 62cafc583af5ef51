#!/usr/bin/env python
"""Stand-alone timing of the Ordinal quadrature (20-node Gauss-Hermite, one lane per row) next to Bernoulli's on the
same rows, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/ordinal_quad_time.py` (counters not mixed in).
Three one-task models with N rows and the same inputs are evaluated `reps` times each, in this order:
  1. Bernoulli                   quad_kernel<1, 0>   the nearest existing 1-D family: 20 nodes, one exp + two log per node
  2. Ordinal, end bins only      quad_kernel<9, 0>   labels 1 and K: one erfcx (or two erfc) per node
  3. Ordinal, middle bins only   quad_kernel<9, 0>   labels 2 .. K-1: two erfcx per node
The script prints the engine's own event timing of the quadrature per evaluation; in the kernel trace the dispatches of
quad_kernel appear in the same order, `reps` per configuration (`--summarise <kernel_trace.csv>` prints their medians).
usage: python tools/ordinal_quad_time.py [N=200000] [reps=5]   |   python tools/ordinal_quad_time.py --summarise kernel_trace.csv [reps=5]"""
import csv
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NAMES = ("Bernoulli", "Ordinal end bins", "Ordinal middle bins")


def summarise(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "quad_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    assert us and len(us) % (3 * reps) == 0, "expected a multiple of %d quad_kernel dispatches, found %d" % (3 * reps, len(us))
    c = len(us) // (3 * reps)                                  # dispatches per evaluation (row pools)
    ev = np.array(us).reshape(3, reps, c).sum(2)               # per configuration and evaluation
    med = [float(np.median(ev[i])) for i in range(3)]
    for i, name in enumerate(NAMES):
        print("%-20s %-18s median %8.1f us over %d evaluations of %d dispatch(es)   (all: %s)" %
              (name, re.search(r"quad_kernel<[^>]*>", rows[i * reps * c]["Kernel_Name"]).group(0), med[i], reps, c, " ".join("%.1f" % u for u in ev[i])))
    print("ratio to Bernoulli: end bins %.2f, middle bins %.2f" % (med[1] / med[0], med[2] / med[0]))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import Engine  # noqa: E402
from hetmogp_amd.synthetic import make_case  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
K = 5
rng = np.random.RandomState(0)
prm, X, Y = make_case([("Bernoulli", {})], [N], M=128, Q=1, P=1, seed=3)
labels = {"Bernoulli": Y[0], "Ordinal end bins": np.where(rng.rand(N, 1) < 0.5, 1.0, float(K)),
          "Ordinal middle bins": rng.randint(2, K, (N, 1)).astype(float)}
for name in NAMES:
    specs = [("Bernoulli", {})] if name == "Bernoulli" else [("Ordinal", {"K": K})]
    e = Engine(specs, 1, 128, 1)
    e.set_data(X, [labels[name]])
    for r in range(reps):
        out = e.elbo_grad(**prm)
        ms, _ = e.timings()
        print("%-20s N = %d, M = 128: quadrature %.3f ms, total %.3f ms (engine events)" % (name, N, ms["quadrature"], ms["total"]))
    assert np.isfinite(out["elbo"])
    e.close()
