#!/usr/bin/env python
"""Gradients of posterior sample paths, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/pathsgrad_time.py`
(a kernel trace in a run of its own): DESIGN 9v's timing shape (M = 1024, Q = 3, nD = 2, S = 64, Lf = 1024, N = 200 000 inputs) at input
dimension P.  `reps` calls each of paths_eval, paths_eval_grad without values and paths_eval_grad with values, each behind a marker launch of
hmogp_sample (one row) so that the trace can be cut.  `--summarise <kernel_trace.csv>` prints, per call, the median device time of the
feature kernel, rbf_kernel, rbf_dx_kernel (with its bytes over time, next to the figures on record for its neighbours: rbf_kernel 4.8 TB/s,
paths_feature_kernel 6.1 TB/s), the products (against 9v's 15.0 ms of 17.8 ms per paths_eval: a gradient call should cost about 1 + P times
that in products with the values, P times without), the rotation and the transposing copy.
usage: python tools/pathsgrad_time.py [P=1] [N=200000] [M=1024] [S=64] [Lf=1024] [reps=3]
       python tools/pathsgrad_time.py --summarise kernel_trace.csv [P=1] [N=200000] [M=1024] [S=64] [Lf=1024] [reps=3]"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, ND = 3, 2
GROUPS = (("features", ("paths_feature_kernel",)), ("rbf", ("rbf_kernel",)), ("rbf_dx", ("rbf_dx_kernel",)), ("GEMM", ("gemm",)),
          ("rotation", ("paths_dtheta_kernel",)), ("transpose", ("paths_gtrans_kernel",)))
NAMES = ("paths_eval", "paths_eval_grad", "paths_eval_grad+F")
RECORD = "on record (DESIGN 9v, P = 1): paths_eval 17.8 ms of device time, products 15.0 ms; rbf_kernel 4.8 TB/s, paths_feature_kernel 6.1 TB/s"


def args(argv):
    return [int(argv[i]) if len(argv) > i else d for i, d in ((0, 1), (1, 200000), (2, 1024), (3, 64), (4, 1024), (5, 3))]


def summarise(path, P, N, M, S, Lf, reps):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    marks = [i for i, r in enumerate(rows) if "sample_kernel" in r["Kernel_Name"]]          # a marker: one hmogp_sample launch
    marks = marks[-3 * reps - 1:]
    assert len(marks) == 3 * reps + 1, "expected %d marker launches, found %d" % (3 * reps + 1, len(marks))
    print(RECORD)
    gemm = {}
    for k, name in enumerate(NAMES):
        tot, per = [], {g: [] for g, _ in GROUPS}
        for r_ in range(reps):
            seg = rows[marks[k * reps + r_] + 1:marks[k * reps + r_ + 1]]
            tot.append(sum(us(r) for r in seg))
            for g, keys in GROUPS:
                per[g].append(sum(us(r) for r in seg if any(x in r["Kernel_Name"] for x in keys)))
        print("%-18s all kernels: median %11.1f us over %d calls, %d launches per call" % (name, np.median(tot), reps, len(seg)))
        for g, _ in GROUPS:
            if np.max(per[g]) > 0:
                print("    %-14s median %11.1f us" % (g, np.median(per[g])))
        print("    %-14s median %11.1f us" % ("other", np.median(tot) - sum(np.median(per[g]) for g, _ in GROUPS)))
        gemm[name] = np.median(per["GEMM"])
        if name != "paths_eval":
            t = np.median(per["rbf_dx"]) * 1e-6
            b = 8.0 * N * Q * M * (1 + P)
            print("    rbf_dx_kernel:  %.3e bytes read and written -> %.3f TB/s" % (b, b / t / 1e12))
            print("    products:       %.2f times paths_eval's" % (gemm[name] / gemm["paths_eval"]))
        t = np.median(per["rbf"]) * 1e-6
        print("    rbf_kernel:     %.3e bytes written -> %.3f TB/s" % (8.0 * N * Q * M, 8.0 * N * Q * M / t / 1e12))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2], *args(sys.argv[3:]))
    P, N, M, S, Lf, reps = args(sys.argv[1:])
    from hetmogp_amd.engine import Engine, sample
    from hetmogp_amd.synthetic import make_case
    specs = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Poisson", {})]
    prm, X, Y = make_case(specs, [4096] * 3, M=M, Q=Q, P=P, seed=3)
    e = Engine(specs, Q, M, P, device=0)
    e.set_data(X, Y)
    e.elbo_grad(**prm)
    Xn = np.random.RandomState(1).rand(N, P)
    d = [0, 1]
    mark = lambda: sample("Gaussian", np.zeros((1, 1)), seed=0, sigma=0.5)
    sid = e.paths_create(d, size=S, num_features=Lf, seed=1)
    e.paths_eval(sid, Xn[:4096]), e.paths_eval_grad(sid, Xn[:4096], values=True)      # warm: the rotated operand is built here
    wall = {}
    for name, call in (("paths_eval", lambda: e.paths_eval(sid, Xn)), ("paths_eval_grad", lambda: e.paths_eval_grad(sid, Xn)),
                       ("paths_eval_grad+F", lambda: e.paths_eval_grad(sid, Xn, values=True))):
        ts = []
        for _ in range(reps):
            mark()
            t = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t)
        wall[name] = np.median(ts)
    mark()
    for k, v in wall.items():
        print("%-18s host wall time per call (transfers included): median %.2f ms" % (k, 1e3 * v))


if __name__ == "__main__":
    main()
