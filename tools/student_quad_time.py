#!/usr/bin/env python
"""Stand-alone timing of the Student-t quadrature (20 x 20 Gauss-Hermite, one wave per row), meant to run under
`rocprofv3 --kernel-trace --stats -- python tools/student_quad_time.py`: the kernel table then lists
  * var_exp_kernel<8, 0>   the building block (hmogp_var_exp) over N rows, and
  * quad_kernel<8, 0>      the same rule inside one ELBO + gradient evaluation of a one-task Student model with N rows.
usage: python tools/student_quad_time.py [N=200000] [reps=5]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hetmogp_amd.engine import Engine, var_exp  # noqa: E402
from hetmogp_amd.synthetic import make_case  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
rng = np.random.RandomState(0)
y = rng.randn(N)
m = np.stack([y + rng.randn(N), rng.uniform(-2.0, 1.0, N)], 1)
v = 10.0 ** rng.uniform(-4.0, 0.0, (N, 2))
for r in range(reps):
    t0 = time.perf_counter()
    ve, _, _ = var_exp("Student", y, m, v, deg_free=5.0)
    print("var_exp Student, N = %d: %.2f ms wall (incl. host <-> device copies)" % (N, 1e3 * (time.perf_counter() - t0)))
assert np.all(np.isfinite(ve))

specs = [("Student", {"deg_free": 5.0})]
prm, X, Y = make_case(specs, [N], M=128, Q=1, P=1, seed=3)
e = Engine(specs, 1, 128, 1)
e.set_data(X, Y)
for r in range(reps):
    out = e.elbo_grad(**prm)
    ms, _ = e.timings()
    print("ELBO + gradient, one Student task, N = %d, M = 128: quadrature %.3f ms, total %.3f ms (engine events)" %
          (N, ms["quadrature"], ms["total"]))
assert np.isfinite(out["elbo"])
e.close()
