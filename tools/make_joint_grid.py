#!/usr/bin/env python
"""Writes tests/golden/jointgrid.npz: the designed cases of the joint posterior at new inputs (tests/joint_ref.py: CASES) --
per case the parameters, Xnew, and the 50-digit mean, covariance entries and error scales (tests/joint_ref_mp.py) rounded to double.
Cases of joint dimension n <= 48 store the full covariance, larger ones every diagonal entry and a seeded subset of the others.  The file
is this tool's own output: parameters from seeded NumPy generators, values from mpmath.

usage: python tools/make_joint_grid.py              write the grid (a few minutes: M = 128 in 50-digit arithmetic)
       python tools/make_joint_grid.py --measure    print the float64 restatement's ratios against the stored grid (C_ORACLE's raw figures)
                                                    and NumPy / LAPACK's Cholesky reconstruction error on the cases' covariances"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_ref as jr            # noqa: E402


def build_case(case):
    import joint_ref_mp as jm
    prm, Xnew = jr.make_params(case)
    cond = max(jr.cond_estimates(prm, case["P"]))
    assert cond < jr.COND_FLAG, (case["name"], cond)
    ri, ci = jr.stored_entries(case)
    ref = jm.reference(prm, Xnew, case["functions"], ri, ci)
    out = dict(prm)
    out.update(Xnew=Xnew, ri=ri.astype(np.int32), ci=ci.astype(np.int32), **ref)
    return out, cond


def chol_backward(cov):
    """|L L^T - (cov + jitter I)| of NumPy's (LAPACK's) factor on the ladder, in units of n 2^-52 max diag; and the rung."""
    return jr.chol_backward(cov, *jr.jitchol(cov)[:2]), jr.jitchol(cov)[2]


def measure():
    grid = jr.load_grid()
    worst = {"mean": 0.0, "cov": 0.0, "chol": 0.0}
    for name, e in grid.items():
        for strict in (False, True):
            mean, cov = jr.joint(e["prm"], e["Xnew"], e["case"]["functions"], strict=strict)
            rm, rc = jr.case_ratios(e, mean, cov)
            worst["mean"], worst["cov"] = max(worst["mean"], rm), max(worst["cov"], rc)
            print("%-7s %-7s mean %8.3f  cov %8.3f" % (name, "strict" if strict else "default", rm, rc))
        cov = jr.joint(e["prm"], e["Xnew"], e["case"]["functions"])[1]
        cb, rung = chol_backward(cov)
        worst["chol"] = max(worst["chol"], cb)
        print("%-7s LAPACK  L L^T - (cov + jitter I): %.3f n eps max diag, rung %d, min eigenvalue / max diag %.2e" %
              (name, cb, rung, np.min(np.linalg.eigvalsh(cov)) / np.max(np.diag(cov))))
    print("worst: mean %.3f  cov %.3f  chol %.3f" % (worst["mean"], worst["cov"], worst["chol"]))


def main():
    if "--measure" in sys.argv[1:]:
        return measure()
    blob = {}
    for case in jr.CASES:
        out, cond = build_case(case)
        for k, v in out.items():
            blob[case["name"] + "/" + k] = v
        print("%-7s n = %4d, %5d covariance entries, condition estimate %.1f" % (case["name"], out["mean"].shape[0], out["cov"].shape[0], cond))
    np.savez_compressed(jr.GRID, **blob)
    print("wrote %s (%d bytes)" % (jr.GRID, os.path.getsize(jr.GRID)))


if __name__ == "__main__":
    main()
