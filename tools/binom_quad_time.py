#!/usr/bin/env python
"""Stand-alone timing of the Binomial (20 nodes, one lane per row) and Beta-Binomial (20 x 20, one wave per row) quadratures of DESIGN 9l
next to Bernoulli's and the Negative Binomial's in the same run, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/binom_quad_time.py`: the kernel table then lists
  * var_exp_kernel<13, 0>   Binomial's building block (hmogp_var_exp) over N rows (k, n), n uniform in 1 .. 200,
  * var_exp_kernel<1, 0>    Bernoulli's over the same number of rows (same rule, same lane mapping),
  * var_exp_kernel<14, 0>   the Beta-Binomial's over N rows (k, n), and
  * var_exp_kernel<11, 0>   the Negative Binomial's over the same number of rows (same rule, same lane mapping, the same helper
                            nb_gamma_diffs once per TABLE entry where the Beta-Binomial calls it once per NODE).
`--summarise <kernel_trace.csv>` prints the medians of the four groups of dispatches.
usage: python tools/binom_quad_time.py [N=1048576] [reps=5]   |   python tools/binom_quad_time.py --summarise kernel_trace.csv [reps=5]"""
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NAMES = ("Binomial", "Bernoulli", "BetaBinomial", "NegBinomial")


def summarise(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "var_exp_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = np.array([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows])
    assert len(us) == 4 * reps, "expected %d dispatches, found %d" % (4 * reps, len(us))
    med = [float(np.median(us[i * reps:(i + 1) * reps])) for i in range(4)]
    for i, name in enumerate(NAMES):
        print("%-14s %-50s median %9.1f us   (all: %s)" % (name, rows[i * reps]["Kernel_Name"][:50], med[i],
                                                           " ".join("%.1f" % u for u in us[i * reps:(i + 1) * reps])))
    print("Binomial: %.2f of Bernoulli's;  BetaBinomial: %.2f of the Negative Binomial's" % (med[0] / med[1], med[2] / med[3]))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    sys.exit(0)

from hetmogp_amd.engine import var_exp  # noqa: E402
from hetmogp_amd.synthetic import binomial_counts  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
v = 10.0 ** rng.uniform(-4.0, -0.5, (N, 2))
m = rng.uniform(-1.5, 1.5, (N, 2))
yb = binomial_counts(rng, "Binomial", m[:, :1], 1, 200)
ybb = binomial_counts(rng, "BetaBinomial", m, 1, 200)
yber = (rng.rand(N) < 0.5).astype(float)
mn = np.stack([rng.uniform(-2.0, 3.0, N), rng.uniform(-2.0, 3.0, N)], 1)
r = np.exp(mn[:, 1])
yn = rng.poisson(np.exp(mn[:, 0]) * rng.gamma(r) / r).astype(float)
for name, yy, mm, vv in (("Binomial", yb, m[:, 0], v[:, 0]), ("Bernoulli", yber, m[:, 0], v[:, 0]), ("BetaBinomial", ybb, m, v),
                         ("NegBinomial", yn, mn, v)):
    for _ in range(reps):
        t0 = time.perf_counter()
        ve, _, _ = var_exp(name, yy, mm, vv)
        print("var_exp %s, N = %d: %.2f ms wall (incl. host <-> device copies)" % (name, N, 1e3 * (time.perf_counter() - t0)))
    assert np.all(np.isfinite(ve))
    print("%s: share of rows with n > 32: %.2f" % (name, np.mean(yy[:, 1] > 32) if np.ndim(yy) == 2 else 0.0))
