#!/usr/bin/env python
"""Stand-alone timing of the likelihood-parameter gradient kernels, meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/likparam_time.py`: one model with a Gaussian, a Student and a K = 11 Ordinal task of
N rows each, evaluated with hmogp_lik_grad_enable on.  The kernel table then lists lik_grad_kernel<0 | 8 | 9> and lik_grad_reduce_kernel
beside the quadrature kernels of the same rows (quad_kernel<0 | 8 | 9>), which are the yardstick.
usage: python tools/likparam_time.py [N=200000] [reps=5]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hetmogp_amd.engine import Engine  # noqa: E402
from hetmogp_amd.synthetic import make_case  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
specs = [("Gaussian", {"sigma": 0.5}), ("Student", {"deg_free": 5.0}), ("Ordinal", {"K": 11})]
prm, X, Y = make_case(specs, [N] * 3, M=128, Q=1, P=1, seed=3)
e = Engine(specs, 1, 128, 1)
e.set_data(X, Y)
for on in (False, True):
    e.lik_grad_enable(on)
    for r in range(reps):
        out = e.elbo_grad(**prm)
        ms, n = e.timings()
        print("switch %s, N = %d per task, M = 128: quadrature category %.3f ms in %d launches, total %.3f ms (engine events)" %
              ("on " if on else "off", N, ms["quadrature"], n["quadrature"], ms["total"]))
    assert np.isfinite(out["elbo"])
print("gradients:", [e.lik_grad(t).tolist() for t in range(3)])
e.close()
