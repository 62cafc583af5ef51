#!/usr/bin/env python
"""Stand-alone timing of the right-censored Weibull quadrature (20 x 20 Gauss-Hermite, one wave per row) next to Student's and
the Negative Binomial's in the same run, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/weibull_quad_time.py`:
the kernel table then lists
  * var_exp_kernel<12, 0>   the building block (hmogp_var_exp) over N rows (y, delta) drawn from the model, 30 % censored,
  * var_exp_kernel<8, 0>    Student's building block over the same number of rows (same rule, same lane mapping),
  * var_exp_kernel<11, 0>   the Negative Binomial's over the same number of rows, and
  * quad_kernel<12, 0>      the rule inside one ELBO + gradient evaluation of a one-task Weibull model with N rows.
`--summarise <kernel_trace.csv>` prints the medians of the four groups of dispatches and the ratios to Student's and the Negative Binomial's.
usage: python tools/weibull_quad_time.py [N=1048576] [reps=5]   |   python tools/weibull_quad_time.py --summarise kernel_trace.csv [reps=5]"""
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
    names = ("Weibull var_exp", "Student var_exp", "NegBinomial var_exp", "Weibull quad_kernel")
    med = [float(np.median(us[i * reps:(i + 1) * reps])) for i in range(4)]
    for i, name in enumerate(names):
        print("%-24s %-60s median %8.1f us   (all: %s)" % (name, rows[i * reps]["Kernel_Name"][:60], med[i],
                                                        " ".join("%.1f" % u for u in us[i * reps:(i + 1) * reps])))
    print("Weibull var_exp_kernel: %.2f of Student's, %.2f of the Negative Binomial's" % (med[0] / med[1], med[0] / med[2]))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import Engine, var_exp  # noqa: E402
from hetmogp_amd.synthetic import make_case, weibull_censored  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
v = 10.0 ** rng.uniform(-4.0, -0.5, (N, 2))
mw = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N)], 1)
yw = weibull_censored(rng, mw[:, 0], mw[:, 1], 0.3)
ys = rng.randn(N)
ms = np.stack([ys + rng.randn(N), rng.uniform(-2.0, 1.0, N)], 1)
mn = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N)], 1)
r = np.exp(mn[:, 1])
yn = rng.poisson(np.exp(mn[:, 0]) * rng.gamma(r) / r).astype(float)
for name, yy, mm, kw in (("Weibull", yw, mw, {}), ("Student", ys, ms, {"deg_free": 5.0}), ("NegBinomial", yn, mn, {})):
    for _ in range(reps):
        t0 = time.perf_counter()
        ve, _, _ = var_exp(name, yy, mm, v, **kw)
        print("var_exp %s, N = %d: %.2f ms wall (incl. host <-> device copies)" % (name, N, 1e3 * (time.perf_counter() - t0)))
    assert np.all(np.isfinite(ve))

specs = [("Weibull", {})]
prm, X, Y = make_case(specs, [N], M=128, Q=1, P=1, seed=3)
e = Engine(specs, 1, 128, 1)
e.set_data(X, Y)
for _ in range(reps):
    out = e.elbo_grad(**prm)
    tm, _ = e.timings()
    print("ELBO + gradient, one Weibull task, N = %d, M = 128: quadrature %.3f ms, total %.3f ms (engine events)" %
          (N, tm["quadrature"], tm["total"]))
print("ELBO %.6g" % float(np.ravel(out["elbo"])[0]))
e.close()
