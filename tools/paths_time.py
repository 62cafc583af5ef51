#!/usr/bin/env python
"""Pathwise posterior samples, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/paths_time.py` (a kernel trace
in a run of its own): one model (M = 1024, Q = 3), a path set of nD = 2 functions, S = 64 samples, Lf = 1024 frequencies, evaluated at N =
200 000 inputs; as the scale, sample_f_joint at N = 2048 in the same run.  `reps` calls each of paths_create (and free), paths_eval and
sample_f_joint, each behind a marker launch of hmogp_sample (one row) so that the trace can be cut.  `--summarise <kernel_trace.csv>`
prints, per call, the median device time of the feature kernel (with bytes/s and sincospi/s), rbf_kernel, the products, the solves and the
draw kernels.
usage: python tools/paths_time.py [N=200000] [M=1024] [S=64] [Lf=1024] [reps=3]
       python tools/paths_time.py --summarise kernel_trace.csv [N=200000] [M=1024] [S=64] [Lf=1024] [reps=3]"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, ND = 3, 2
GROUPS = (("features", ("paths_feature_kernel",)), ("draw kernels", ("paths_omega_kernel", "paths_normal_kernel", "paths_scale_kernel")),
          ("rbf", ("rbf_kernel",)), ("GEMM", ("gemm",)), ("solves", ("trsm",)), ("joint kernels", ("joint_",)))
NAMES = ("paths_create", "paths_eval", "sample_f_joint")


def args(argv):
    return [int(argv[i]) if len(argv) > i else d for i, d in ((0, 200000), (1, 1024), (2, 64), (3, 1024), (4, 3))]


def summarise(path, N, M, S, Lf, reps):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    marks = [i for i, r in enumerate(rows) if "sample_kernel" in r["Kernel_Name"]]          # a marker: one hmogp_sample launch
    marks = marks[-3 * reps - 1:]
    assert len(marks) == 3 * reps + 1, "expected %d marker launches, found %d" % (3 * reps + 1, len(marks))
    for k, name in enumerate(NAMES):
        tot, per = [], {g: [] for g, _ in GROUPS}
        for r_ in range(reps):
            seg = rows[marks[k * reps + r_] + 1:marks[k * reps + r_ + 1]]
            tot.append(sum(us(r) for r in seg))
            for g, keys in GROUPS:
                per[g].append(sum(us(r) for r in seg if any(x in r["Kernel_Name"] for x in keys)))
        print("%-16s all kernels: median %11.1f us over %d calls, %d launches per call" % (name, np.median(tot), reps, len(seg)))
        for g, _ in GROUPS:
            if np.max(per[g]) > 0:
                print("    %-14s median %11.1f us" % (g, np.median(per[g])))
        print("    %-14s median %11.1f us" % ("other", np.median(tot) - sum(np.median(per[g]) for g, _ in GROUPS)))
        if name == "paths_eval":
            t = np.median(per["features"]) * 1e-6
            print("    feature kernel: %.3e bytes written -> %.3f TB/s; %.3e sincospi -> %.3e sincospi/s" %
                  (8.0 * N * Q * 2 * Lf, 8.0 * N * Q * 2 * Lf / t / 1e12, float(N) * Q * Lf, float(N) * Q * Lf / t))
            t = np.median(per["rbf"]) * 1e-6
            print("    rbf_kernel:     %.3e bytes written -> %.3f TB/s" % (8.0 * N * Q * M, 8.0 * N * Q * M / t / 1e12))
            t = np.median(per["GEMM"]) * 1e-6
            print("    products:       %.3e flop -> %.2f TFLOP/s" % (2.0 * N * Q * (2 * Lf + M) * ND * S, 2.0 * N * Q * (2 * Lf + M) * ND * S / t / 1e12))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2], *args(sys.argv[3:]))
    N, M, S, Lf, reps = args(sys.argv[1:])
    from hetmogp_amd.engine import Engine, sample
    from hetmogp_amd.synthetic import make_case
    specs = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Poisson", {})]
    prm, X, Y = make_case(specs, [4096] * 3, M=M, Q=Q, P=1, seed=3)
    e = Engine(specs, Q, M, 1, device=0)
    e.set_data(X, Y)
    e.elbo_grad(**prm)
    Xn = np.random.RandomState(1).rand(N, 1)
    Xj = Xn[:2048]
    d = [0, 1]
    mark = lambda: sample("Gaussian", np.zeros((1, 1)), seed=0, sigma=0.5)
    sid = e.paths_create(d, size=S, num_features=Lf, seed=1)          # warm
    e.paths_eval(sid, Xn[:4096]), e.sample_f_joint(Xj, d, size=S, seed=1)

    def create():
        s = e.paths_create(d, size=S, num_features=Lf, seed=1)
        e.paths_free(s)

    wall = {}
    for name, call in (("paths_create", create), ("paths_eval", lambda: e.paths_eval(sid, Xn)),
                       ("sample_f_joint", lambda: e.sample_f_joint(Xj, d, size=S, seed=1))):
        ts = []
        for _ in range(reps):
            mark()
            t = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t)
        wall[name] = np.median(ts)
    mark()
    for k, v in wall.items():
        print("%-16s host wall time per call (transfers included): median %.2f ms" % (k, 1e3 * v))


if __name__ == "__main__":
    main()
