#!/usr/bin/env python
"""The input gradients of q(f) beside predict_f on the same rows, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/xgrad_time.py` (a kernel trace in a run of its own): one model (M = 1024, Q = 3, P = 2),
N = 200 000 new inputs; `reps` calls each of predict_f and predict_f_grad, each behind a marker launch of hmogp_sample (one row) so that the
trace can be cut.  `--summarise <kernel_trace.csv>` prints, per call (all chunks summed; medians over the calls), the device time of
qf_xgrad_kernel and its achieved bandwidth against the 2 N M Q 8 bytes it must read, the T GEMM, K_uf, the combine, and everything
predict_f launches.
usage: python tools/xgrad_time.py [N=200000] [M=1024] [reps=5]   |   python tools/xgrad_time.py --summarise kernel_trace.csv [N] [M] [reps]"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q, P = 3, 2


def summarise(path, N, M, reps):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    marks = [i for i, r in enumerate(rows) if "sample_kernel" in r["Kernel_Name"]][-2 * reps - 1:]
    assert len(marks) == 2 * reps + 1, "expected %d marker launches, found %d" % (2 * reps + 1, len(marks))
    segs = [rows[marks[k] + 1:marks[k + 1]] for k in range(2 * reps)]
    tot_f = [sum(us(r) for r in s) for s in segs[:reps]]
    print("predict_f        all kernels: median %9.1f us over %d calls, %d launches per call" % (np.median(tot_f), reps, len(segs[0])))
    grad = segs[reps:]
    tot_g = [sum(us(r) for r in s) for s in grad]
    print("predict_f_grad   all kernels: median %9.1f us over %d calls, %d launches per call" % (np.median(tot_g), reps, len(grad[0])))
    pick = lambda s, key: [r for r in s if key in r["Kernel_Name"]]
    xg = [sum(us(r) for r in pick(s, "qf_xgrad_kernel")) for s in grad]
    byts = 2.0 * N * M * Q * 8
    print("    qf_xgrad_kernel    median %9.1f us  (%d launches)  %.2f TB/s of the %.2f GB it must read" %
          (np.median(xg), len(pick(grad[0], "qf_xgrad_kernel")), byts / (np.median(xg) * 1e-6) / 1e12, byts / 1e9))
    for label, key in (("T GEMM", "gemm_f64_kernel"), ("combine", "qf_xgrad_combine_kernel"), ("K_uf", "rbf_kernel")):
        t = [sum(us(r) for r in pick(s, key)) for s in grad]
        print("    %-18s median %9.1f us  (%d launches)" % (label, np.median(t), len(pick(grad[0], key))))
    print("    on top of predict_f: median %9.1f us" % (np.median(tot_g) - np.median(tot_f)))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        a = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((3, 200000), (4, 1024), (5, 5))]
        return summarise(sys.argv[2], *a)
    N, M, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 200000), (2, 1024), (3, 5))]
    from hetmogp_amd.engine import Engine, sample
    from hetmogp_amd.synthetic import make_case
    specs = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Poisson", {})]
    prm, X, Y = make_case(specs, [4096] * 3, M=M, Q=Q, P=P, seed=3)
    e = Engine(specs, Q, M, P, device=0)
    e.set_data(X, Y)
    e.elbo_grad(**prm)
    Xn = np.random.RandomState(1).rand(N, P)
    mark = lambda: sample("Gaussian", np.zeros((1, 1)), seed=0, sigma=0.5)
    e.predict_f(Xn), e.predict_f_grad(Xn)          # warm
    wall = {}
    for name, call in (("predict_f", lambda: e.predict_f(Xn)), ("predict_f_grad", lambda: e.predict_f_grad(Xn))):
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
