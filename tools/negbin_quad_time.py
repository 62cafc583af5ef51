#!/usr/bin/env python
"""Stand-alone timing of the Negative Binomial quadrature (20 x 20 Gauss-Hermite, one wave per row) next to Student's in the
same run, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/negbin_quad_time.py`: the kernel table then lists
  * var_exp_kernel<11, 0>   the building block (hmogp_var_exp) over N rows of counts drawn from the model,
  * var_exp_kernel<8, 0>    Student's building block over the same number of rows (the yardstick: same rule, same lane mapping), and
  * quad_kernel<11, 0>      the rule inside one ELBO + gradient evaluation of a one-task Negative Binomial model with N rows.
A second Negative Binomial pass has every y > 32 (the series instead of the sums in the per-row table): its dispatches are the LAST `reps`
of var_exp_kernel<11, 0> in the trace.
`--summarise <kernel_trace.csv>` prints the medians of the four groups of dispatches and their ratios to Student's.
usage: python tools/negbin_quad_time.py [N=200000] [reps=5]   |   python tools/negbin_quad_time.py --summarise kernel_trace.csv [reps=5]"""
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def summarise(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "var_exp_kernel" in r["Kernel_Name"] or "quad_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows])
    assert len(us) == 4 * reps, "expected %d dispatches, found %d" % (4 * reps, len(us))
    names = ("NegBinomial var_exp, y from the model", "Student var_exp", "NegBinomial var_exp, every y > 32", "NegBinomial quad_kernel")
    med = [float(np.median(us[i * reps:(i + 1) * reps])) for i in range(4)]
    for i, name in enumerate(names):
        print("%-40s %-60s median %8.1f us   (all: %s)" % (name, rows[i * reps]["Kernel_Name"][:60], med[i],
                                                        " ".join("%.1f" % u for u in us[i * reps:(i + 1) * reps])))
    print("ratio to Student's var_exp_kernel: %.2f (y from the model), %.2f (every y > 32)" % (med[0] / med[1], med[2] / med[1]))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import Engine, var_exp  # noqa: E402
from hetmogp_amd.synthetic import make_case  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
m = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N)], 1)
v = 10.0 ** rng.uniform(-4.0, 0.0, (N, 2))
r = np.exp(m[:, 1])
y = rng.poisson(np.exp(m[:, 0]) * rng.gamma(r) / r).astype(float)
ys = rng.randn(N)
ms = np.stack([ys + rng.randn(N), rng.uniform(-2.0, 1.0, N)], 1)
for name, yy, mm, kw in (("NegBinomial", y, m, {}), ("Student", ys, ms, {"deg_free": 5.0}), ("NegBinomial", y + 33.0, m, {})):
    for _ in range(reps):
        t0 = time.perf_counter()
        ve, _, _ = var_exp(name, yy, mm, v, **kw)
        note = ", %d %% of the rows with y <= 32" % round(100.0 * np.mean(yy <= 32.0)) if name == "NegBinomial" else ""
        print("var_exp %s, N = %d%s: %.2f ms wall (incl. host <-> device copies)" % (name, N, note, 1e3 * (time.perf_counter() - t0)))
    assert np.all(np.isfinite(ve))

specs = [("NegBinomial", {})]
prm, X, Y = make_case(specs, [N], M=128, Q=1, P=1, seed=3)
e = Engine(specs, 1, 128, 1)
e.set_data(X, Y)
for _ in range(reps):
    out = e.elbo_grad(**prm)
    tm, _ = e.timings()
    print("ELBO + gradient, one NegBinomial task, N = %d, M = 128: quadrature %.3f ms, total %.3f ms (engine events)" %
          (N, tm["quadrature"], tm["total"]))
assert np.isfinite(out["elbo"])
e.close()
