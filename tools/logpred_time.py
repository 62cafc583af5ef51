#!/usr/bin/env python
"""Stand-alone timing of the deterministic log predictive density beside the Monte-Carlo kernel it complements, meant to run
under `rocprofv3 --kernel-trace --stats -- python tools/logpred_time.py` (a kernel trace in a run of its own): per family the kernel table
then lists, over the same N rows and `reps` dispatches each,
  * lpd_lane_kernel<LIK> / lpd_wave_kernel<LIK, J>      the rule (hmogp_log_predictive_gh), and
  * log_predictive_kernel<LIK> / dirichlet_log_predictive_kernel<K>   the 1000-sample estimate (hmogp_log_predictive); none for Gamma and
    Beta, which it refuses.
The wall times printed here include the host <-> device copies of the building blocks; the kernel times are the trace's.
usage: python tools/logpred_time.py [N=200000] [reps=5] [family ...]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import logpred_ref as lr  # noqa: E402  (seeded rows only)
from hetmogp_amd.engine import log_predictive_density_rows, log_predictive_rows  # noqa: E402

args = sys.argv[1:]
N = int(args[0]) if len(args) > 0 else 200000
reps = int(args[1]) if len(args) > 1 else 5
families = args[2:] or list(lr.FAMILIES)
for name in families:
    kw = dict(lr.BULK_KW.get(name, {}))
    y, m, v = lr.bulk_rows(name, N, 1, vhi=0.25, **kw)
    t_gh, t_mc = [], []
    for r in range(reps):
        t0 = time.perf_counter()
        a = log_predictive_density_rows(name, y, m, v, **kw)
        t_gh.append(1e3 * (time.perf_counter() - t0))
        if name not in lr.MC_REFUSED:
            t0 = time.perf_counter()
            b = log_predictive_rows(name, y, m, v, num_samples=1000, seed=r, **kw)
            t_mc.append(1e3 * (time.perf_counter() - t0))
    assert np.all(np.isfinite(a))
    print("%-12s N = %d: rule %.2f ms wall (best of %d), Monte Carlo (1000 samples) %s" %
          (name, N, min(t_gh), reps, "%.2f ms wall" % min(t_mc) if t_mc else "refused"))
