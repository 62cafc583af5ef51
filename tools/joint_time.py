#!/usr/bin/env python
"""The joint posterior at new inputs beside predict_f on the same rows, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/joint_time.py` (a kernel trace in a run of its own): one model (M = 1024, Q = 3), N = 2048
new inputs, nD = 2 functions (n = 4096), S = 64 draws; `reps` calls each of predict_f, predict_f_joint and sample_f_joint, each group behind
a marker launch of hmogp_sample (one row) so that the trace can be cut.  `--summarise <kernel_trace.csv>` prints, per
call, the median device time of the assemble kernel, the normal fill, the GEMMs, the factorisation (potrf panels and their updates) and
of everything predict_f launches.
usage: python tools/joint_time.py [N=2048] [M=1024] [S=64] [reps=5]   |   python tools/joint_time.py --summarise kernel_trace.csv [reps=5]"""
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = (("assemble", ("joint_assemble_kernel",)), ("normal fill", ("joint_normal_kernel",)), ("gather", ("joint_gather_kernel",)),
          ("factorisation", ()), ("GEMM", ("gemm",)), ("rbf", ("rbf_kernel",)), ("solves", ("trsm",)))


def summarise(path, reps):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    marks = [i for i, r in enumerate(rows) if "sample_kernel" in r["Kernel_Name"]]          # a marker: one hmogp_sample launch
    marks = marks[-3 * reps - 1:]
    assert len(marks) == 3 * reps + 1, "expected %d marker launches, found %d" % (3 * reps + 1, len(marks))
    names = ("predict_f", "predict_f_joint", "sample_f_joint")
    for k, name in enumerate(names):
        tot, per = [], {g: [] for g, _ in GROUPS}
        for r_ in range(reps):
            seg = rows[marks[k * reps + r_] + 1:marks[k * reps + r_ + 1]]
            tot.append(sum(us(r) for r in seg))
            # the trailing updates of the blocked factorisation are GEMM launches: everything between the first diagonal shift and the
            # normal fill belongs to the factorisation (every rung of the ladder included)
            nm = [r["Kernel_Name"] for r in seg]
            lo = next((i for i, x in enumerate(nm) if "add_diag_copy" in x), len(seg))
            hi = next((i for i, x in enumerate(nm) if "joint_normal_kernel" in x), len(seg))
            for g, keys in GROUPS:
                mine = [r for i, r in enumerate(seg) if (lo <= i < hi if g == "factorisation" else not lo <= i < hi) and
                        (g == "factorisation" or any(x in r["Kernel_Name"] for x in keys))]
                per[g].append(sum(us(r) for r in mine))
        print("%-16s all kernels: median %9.1f us over %d calls, %d launches per call" % (name, np.median(tot), reps, len(seg)))
        for g, _ in GROUPS:
            if np.max(per[g]) > 0:
                print("    %-14s median %9.1f us" % (g, np.median(per[g])))
        print("    %-14s median %9.1f us" % ("other", np.median(tot) - sum(np.median(per[g]) for g, _ in GROUPS)))
        other = {}
        for i, r in enumerate(seg):              # (the last call's launches outside the groups, by kernel)
            if not lo <= i < hi and not any(x in r["Kernel_Name"] for _, ks in GROUPS for x in ks):
                other[r["Kernel_Name"][:60]] = other.get(r["Kernel_Name"][:60], 0.0) + us(r)
        for k_, v in sorted(other.items(), key=lambda kv: -kv[1])[:4]:
            print("        %-60s %9.1f us" % (k_, v))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    N, M, S, reps = [int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((1, 2048), (2, 1024), (3, 64), (4, 5))]
    from hetmogp_amd.engine import Engine, sample
    from hetmogp_amd.synthetic import make_case
    specs = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Poisson", {})]
    prm, X, Y = make_case(specs, [4096] * 3, M=M, Q=3, P=1, seed=3)
    e = Engine(specs, 3, M, 1, device=0)
    e.set_data(X, Y)
    e.elbo_grad(**prm)
    Xn = np.random.RandomState(1).rand(N, 1)
    d = [0, 1]
    mark = lambda: sample("Gaussian", np.zeros((1, 1)), seed=0, sigma=0.5)
    e.predict_f(Xn), e.predict_f_joint(Xn, d), e.sample_f_joint(Xn, d, size=S, seed=1)          # warm
    wall = {}
    for name, call in (("predict_f", lambda: e.predict_f(Xn)), ("predict_f_joint", lambda: e.predict_f_joint(Xn, d)),
                       ("sample_f_joint", lambda: e.sample_f_joint(Xn, d, size=S, seed=1, return_factor=True))):
        ts = []
        for _ in range(reps):
            mark()
            t = time.perf_counter()
            out = call()
            ts.append(time.perf_counter() - t)
        wall[name] = np.median(ts)
        if name == "sample_f_joint":
            print("rung %d, jitter %.3e" % (out[1]["rung"], out[1]["jitter"]))
    mark()
    for k, v in wall.items():
        print("%-16s host wall time per call (transfers included): median %.2f ms" % (k, 1e3 * v))


if __name__ == "__main__":
    main()
