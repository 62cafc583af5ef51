#!/usr/bin/env python
"""Inducing-input selection at the headline sizes, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/zsel_time.py` (a kernel trace in a run of its own): N = 200 000 and 800 000 pooled rows
(P = 2), M = 256 and 1024 picks, two RBF kernels; one small warm-up selection first.  Prints the host wall time of each call (upload,
allocation and read-back included).  `--summarise <kernel_trace.csv>` cuts the trace at the init kernels and prints, per call, the step
kernel's time per pick in the upper half of the picks, the bytes a pick moves there (8 N (j + 1): the planes read plus the one written; d
and X are 8 N (2 + P) more), the achieved TB/s beside the 6.3 TB/s the HBM sustains, and the share of the one-block kernel.
usage: python tools/zsel_time.py [N,N,..] [M,M,..]   |   python tools/zsel_time.py --summarise kernel_trace.csv [N,N,..] [M,M,..]"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 2
HBM_TBS = 6.3


def sizes(argv):
    Ns = [int(v) for v in argv[0].split(",")] if len(argv) > 0 else [200000, 800000]
    Ms = [int(v) for v in argv[1].split(",")] if len(argv) > 1 else [256, 1024]
    return [(N, M) for N in Ns for M in Ms]


def summarise(path, calls):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    rows = [r for r in rows if "zsel_" in r["Kernel_Name"]]
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    starts = [i for i, r in enumerate(rows) if "zsel_init_kernel" in r["Kernel_Name"]][-len(calls):]
    assert len(starts) == len(calls), "expected %d selections in the trace, found %d" % (len(calls), len(starts))
    for k, (N, M) in enumerate(calls):
        seg = rows[starts[k]:starts[k + 1] if k + 1 < len(calls) else len(rows)]
        step = [us(r) for r in seg if "zsel_step_kernel" in r["Kernel_Name"]]
        pick = [us(r) for r in seg if "zsel_pick_kernel" in r["Kernel_Name"]]
        assert len(step) == M, (N, M, len(step))
        span = (int(seg[-1]["End_Timestamp"]) - int(seg[0]["Start_Timestamp"])) / 1e3
        j = np.arange(M // 2, M)
        t = np.array(step[M // 2:])
        by = 8.0 * N * (j + 1)
        print("N = %7d  M = %4d: step kernel, picks %d .. %d: %8.1f us per pick (first %7.1f, last %7.1f), %7.1f MB per pick, %.2f TB/s of %.1f"
              % (N, M, M // 2, M - 1, t.mean(), t[0], t[-1], by.mean() / 1e6, by.sum() / t.sum() / 1e6, HBM_TBS))
        print("    all %d picks: step %.1f ms, one-block kernel %.1f ms (median %.1f us per launch), first launch to last end %.1f ms"
              % (M, sum(step) / 1e3, sum(pick) / 1e3, np.median(pick), span / 1e3))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2], sizes(sys.argv[3:]))
    from hetmogp_amd.engine import select_inducing_rows
    var, ell = [1.0, 0.5], [0.02, 0.01]
    select_inducing_rows(np.random.RandomState(0).rand(4096, P), var, ell, 8, device=0)          # warm
    for N, M in sizes(sys.argv[1:]):
        X = np.random.RandomState(1).rand(N, P)
        t = time.perf_counter()
        r = select_inducing_rows(X, var, ell, M, device=0)
        dt = time.perf_counter() - t
        assert r["Mout"] == M, (N, M, r["Mout"])
        print("N = %7d  M = %4d: host wall time %8.1f ms (upload, allocation, read-back included); tr(K_ff - Q_ff) / tr(K_ff) = %.4f, "
              "sqrt(min dpiv / k0) = %.4f" % (N, M, 1e3 * dt, r["trace"][-1] / r["trace"][0], np.sqrt(r["dpiv"].min() / 1.5)))


if __name__ == "__main__":
    main()
