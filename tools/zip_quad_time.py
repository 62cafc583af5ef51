#!/usr/bin/env python
"""Stand-alone timing of the zero-inflated Poisson quadrature of DESIGN 9n (one wave per row: 400 nodes on a row with y = 0, 40 on a row
with y >= 1) next to the Negative Binomial's (400 nodes on every row) in the same run, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/zip_quad_time.py`: the kernel table then lists, `reps` dispatches each and in this order,
  * var_exp_kernel<15, 0>   over N rows that are all zero,
  * var_exp_kernel<15, 0>   over N rows that are all positive,
  * var_exp_kernel<15, 0>   over N counts drawn from the model at the rows' mean parameters,
  * var_exp_kernel<11, 0>   the Negative Binomial's building block over N counts drawn from its model.
`--summarise <kernel_trace.csv | results.db>` prints the medians of the four groups of dispatches and their ratios to the last.
usage: python tools/zip_quad_time.py [N=200000] [reps=5]   |   python tools/zip_quad_time.py --summarise <trace> [reps=5]"""
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GROUPS = ("ZIPoisson, every y = 0", "ZIPoisson, every y >= 1", "ZIPoisson, y from the model", "NegBinomial, y from the model")


def dispatches(path):
    """[(kernel name, start ns, end ns)] of the var_exp kernels in start order, from a kernel trace as CSV or as the profiler's SQLite
    database (its `kernels` view), whichever this rocprofv3 writes."""
    if path.endswith(".db"):
        import sqlite3
        rows = sqlite3.connect(path).execute("select name, start, end from kernels where name like '%var_exp_kernel%'").fetchall()
    else:
        rows = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(open(path))
                if "var_exp_kernel" in r["Kernel_Name"]]
    return sorted(rows, key=lambda r: r[1])


def summarise(path, reps):
    rows = dispatches(path)
    us = np.array([(e - s) / 1e3 for _, s, e in rows])
    assert len(us) == 4 * reps, "expected %d dispatches, found %d" % (4 * reps, len(us))
    med = [float(np.median(us[i * reps:(i + 1) * reps])) for i in range(4)]
    for i, name in enumerate(GROUPS):
        print("%-30s %-40s median %9.1f us   %.2f of the Negative Binomial's   (all: %s)" % (
            name, rows[i * reps][0][:40], med[i], med[i] / med[3], " ".join("%.1f" % u for u in us[i * reps:(i + 1) * reps])))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import var_exp  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
m = rng.uniform(-3.0, 3.0, (N, 2))
v = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, 2)))
lam = np.exp(m[:, 0])
y_model = np.where(rng.rand(N) < 1.0 / (1.0 + np.exp(-m[:, 1])), 0.0, rng.poisson(lam)).astype(float)
y_pos = 1.0 + rng.poisson(lam)
r = np.exp(m[:, 1])
y_nb = rng.poisson(lam * rng.gamma(r) / r).astype(float)
for group, name, yy in zip(GROUPS, ("ZIPoisson", "ZIPoisson", "ZIPoisson", "NegBinomial"), (np.zeros(N), y_pos, y_model, y_nb)):
    for _ in range(reps):
        t0 = time.perf_counter()
        ve, _, _ = var_exp(name, yy, m, v)
        print("var_exp %s, N = %d: %.2f ms wall (incl. host <-> device copies)" % (group, N, 1e3 * (time.perf_counter() - t0)))
    assert np.all(np.isfinite(ve))
    print("%s: share of rows with y = 0: %.2f" % (group, np.mean(yy == 0.0)))
