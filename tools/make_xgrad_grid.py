#!/usr/bin/env python
"""Writes tests/golden/xgradgrid.npz: the 50-digit input gradients (tests/xgrad_ref_mp.py) of the designed cases of tests/xgrad_ref.py,
rounded to double, with the criterion's scale and floor -- a subset of at most 24 rows per case (xgrad_ref.stored_rows); the inputs
themselves regenerate from the cases' seeds.  Beside them the whole-chain references of the engine path at M = 16 (`chain/<case>/...`,
cases of tests/joint_ref.py).

usage: python tools/make_xgrad_grid.py            write the grid (a few minutes: M = 200 at 50 digits)
       python tools/make_xgrad_grid.py --measure  the float64 restatement against the stored grid: the raw figures behind C_ORACLE and
                                                  C_ORACLE_STRICT of tests/xgrad_ref.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import joint_ref as jr            # noqa: E402
import xgrad_ref as xr            # noqa: E402

KEYS = ("dm", "dv", "S_dm", "S_dv", "F_dm", "F_dv")
CHAIN_CASES = ("s_N63", "s_N65", "s_N129")


def chain_rows(name):
    c = jr.CASE_BY_NAME[name]
    return xr.stored_rows(dict(N=c["N"], seed=c["seed"], M=c["M"], shift=0.0))


def write():
    import xgrad_ref_mp as xm
    out = {}
    for c in xr.CASES:
        rows = xr.stored_rows(c)
        ref = xm.reference(xr.make_inputs(c), rows)
        out[c["name"] + "/rows"] = rows
        for k in KEYS:
            out[c["name"] + "/" + k] = ref[k]
        print("%-14s %2d rows" % (c["name"], len(rows)), flush=True)
    for name in CHAIN_CASES:
        prm, Xnew = jr.make_params(jr.CASE_BY_NAME[name])
        rows = chain_rows(name)
        ref = xm.chain_reference(prm, Xnew, rows)
        out["chain/" + name + "/rows"] = rows
        for k in KEYS:
            out["chain/" + name + "/" + k] = ref[k]
        print("chain %-8s %2d rows" % (name, len(rows)), flush=True)
    np.savez_compressed(xr.GRID, **out)
    print("%s: %d bytes" % (xr.GRID, os.path.getsize(xr.GRID)))


def load_chain(name):
    g = np.load(xr.GRID)
    k = "chain/" + name + "/"
    return dict(rows=g[k + "rows"], **{key: g[k + key] for key in KEYS})


def measure():
    grid = xr.load_grid()
    worst = [0.0, 0.0]
    for c in xr.CASES:
        dm, dv = xr.input_grad(xr.make_inputs(c))
        rm, rv = xr.case_ratios(grid[c["name"]], dm, dv)
        worst = [max(worst[0], rm), max(worst[1], rv)]
        print("%-14s dm %.3f dv %.3f" % (c["name"], rm, rv))
    print("building block: worst dm %.3f dv %.3f" % tuple(worst))
    for strict in (False, True):
        worst = [0.0, 0.0]
        for name in CHAIN_CASES:
            prm, Xnew = jr.make_params(jr.CASE_BY_NAME[name])
            e = load_chain(name)
            cond = max(jr.cond_estimates(prm, Xnew.shape[1]))
            dm, dv = xr.chain(prm, Xnew, strict=strict)
            rm = float(np.max(xr.ratios(dm[e["rows"]], e["dm"], cond * e["S_dm"], e["F_dm"])))
            rv = float(np.max(xr.ratios(dv[e["rows"]], e["dv"], cond * e["S_dv"], e["F_dv"])))
            worst = [max(worst[0], rm), max(worst[1], rv)]
            print("chain %-7s %-7s cond_est %.1f dm %.3f dv %.3f" % (name, "strict" if strict else "default", cond, rm, rv))
        print("chain, %s: worst dm %.3f dv %.3f (scale S x cond_est)" % ("strict" if strict else "default", worst[0], worst[1]))


if __name__ == "__main__":
    measure() if "--measure" in sys.argv else write()
