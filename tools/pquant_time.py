#!/usr/bin/env python
"""Stand-alone timing of the predictive cdf / quantile kernels beside the log-predictive-density kernel of the same family
 as the scale, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/pquant_time.py` (a kernel trace in a run of
its own): per family the kernel table then lists, over the same N rows and `reps` dispatches each,
  * pcdf_lane_kernel<LIK> / pcdf_wave_kernel<T>            cdf and sf (hmogp_predictive_cdf),
  * pquant_lane_kernel<LIK, T> / pquant_wave_kernel<T>     nP = 3 quantiles per row (hmogp_predictive_quantile), and
  * lpd_lane_kernel<LIK> / lpd_wave_kernel<LIK, J>         the log predictive density (hmogp_log_predictive_gh).
It also prints the mean number of evaluations of the rule per quantile, counted by the restatement's copy of the solver on the first
`nsolve` of the same rows: what the solver costs.  The wall times printed here include the host <-> device copies of the building
blocks; the kernel times are the trace's.
`--summarise <kernel_trace.csv>` prints the median per kernel name of the trace such a run leaves.
usage: python tools/pquant_time.py [N=200000] [reps=5] [nsolve=2000] [family ...]   |   python tools/pquant_time.py --summarise kernel_trace.csv"""
import csv
import os
import sys
import time

import numpy as np


def summarise(path):
    us = {}
    for r in csv.DictReader(open(path)):
        if any(k in r["Kernel_Name"] for k in ("pcdf_", "pquant_", "lpd_")):
            us.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for k in sorted(us):
        print("%-90s dispatches %2d  median %9.1f us" % (k[:90], len(us[k]), float(np.median(us[k]))))


if len(sys.argv) > 1 and sys.argv[1] == "--summarise":
    summarise(sys.argv[2])
    sys.exit(0)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pquant_ref as pq  # noqa: E402  (seeded rows, the solver's evaluation count)
from hetmogp_amd.engine import log_predictive_density_rows, predictive_cdf_rows, predictive_quantile_rows  # noqa: E402

PROBS = [0.025, 0.5, 0.975]
args = sys.argv[1:]
N = int(args[0]) if len(args) > 0 else 200000
reps = int(args[1]) if len(args) > 1 else 5
nsolve = int(args[2]) if len(args) > 2 else 2000
families = args[3:] or list(pq.FAMILIES)
for name in families:
    kw = dict(pq.BULK_KW.get(name, {}))
    y2, m, v = pq.lr.bulk_rows(name, N, 1, vhi=0.25, **kw)
    y2 = np.asarray(y2, float)
    y = y2[:, 0] if y2.ndim == 2 else y2
    t_c, t_q, t_l = [], [], []
    for r in range(reps):
        t0 = time.perf_counter()
        c, s = predictive_cdf_rows(name, y, m, v, return_sf=True, **kw)
        t_c.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        q = predictive_quantile_rows(name, m, v, PROBS, **kw)
        t_q.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        a = log_predictive_density_rows(name, y2, m, v, **kw)
        t_l.append(1e3 * (time.perf_counter() - t0))
    assert np.all(np.isfinite(c)) and np.all(np.isfinite(s)) and np.all(np.isfinite(a)) and not np.isnan(q).any()
    nev = pq.quantile(name, m[:nsolve], v[:nsolve], PROBS, count=True, **kw)[1]
    print("%-12s N = %d: cdf %.2f ms, %d quantiles %.2f ms, lpd %.2f ms wall (best of %d); evaluations of the rule per quantile: mean %s, most %d" %
          (name, N, min(t_c), len(PROBS), min(t_q), min(t_l), reps,
           "none (closed form over the support)" if name in pq.DISCRETE else "%.2f" % nev.mean(), nev.max()))
