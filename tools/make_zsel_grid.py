#!/usr/bin/env python
"""Writes tests/golden/zselgrid.npz: the designed cases of the inducing-input selection (tests/zsel_ref.py: CASES) -- per case
the inputs and the 50-digit pivots, dpiv and trace (tests/zsel_ref_mp.py) rounded to double; the forced cases also L and d after each
Mmax of the test grid, on every row up to 65 rows and on a subset (pivots, block edges, a seeded sample) beyond.  The file is this
tool's own output: inputs from seeded NumPy generators, values from mpmath.

usage: python tools/make_zsel_grid.py              write the grid (about a minute in 50-digit arithmetic)
       python tools/make_zsel_grid.py --measure    print the float64 restatement's ratios against the stored grid (C_ORACLE's raw figures)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import zsel_ref as zr            # noqa: E402


def build_case(case):
    import zsel_ref_mp as zm
    X, var, ell = zr.make_inputs(case)
    out = dict(X=X, var=var, ell=ell)
    if case in zr.FORCED_CASES:
        piv = zr.forced_pivots(case)
        mm = [m for m in zr.FORCED_MMAX if m <= case["M"]]
        ref = zm.select(X, var, ell, case["M"], forced=piv, d_after=mm)
        rows = zr.stored_rows(case, piv)
        out.update(rows=rows.astype(np.int64), L=ref["L"][rows], d_after=np.stack([ref["d_after"][m][rows] for m in mm]))
    else:
        ref = zm.select(X, var, ell, case["M"])
    out.update(pivots=ref["pivots"], dpiv=ref["dpiv"], trace=ref["trace"], k0=np.float64(ref["k0"]))
    return out


def measure():
    grid = zr.load_grid()
    worst = dict(L=0.0, d=0.0, dpiv=0.0, trace=0.0)
    for case in zr.FORCED_CASES:
        e = grid[case["name"]]
        for m in e["mmax"]:
            r = zr.select(e["X"], e["var"], e["ell"], m, forced=e["pivots"][:m])
            got = zr.prefix_ratios(e, r, m)
            for k in worst:
                worst[k] = max(worst[k], got[k])
            print("%-8s Mmax %2d  L %7.3f  d %7.3f  dpiv %7.3f  trace %7.3f" % (case["name"], m, got["L"], got["d"], got["dpiv"], got["trace"]))
    print("worst: " + "  ".join("%s %.3f" % kv for kv in worst.items()))


def main():
    if "--measure" in sys.argv[1:]:
        return measure()
    blob = {}
    for case in zr.CASES:
        out = build_case(case)
        for k, v in out.items():
            blob[case["name"] + "/" + k] = v
        print("%-8s N = %4d, P = %d, Q = %d, %2d picks, d / k0 down to %.2e" %
              (case["name"], case["N"], case["P"], case["Q"], len(out["pivots"]), np.min(out["dpiv"]) / out["k0"]))
    np.savez_compressed(zr.GRID, **blob)
    print("wrote %s (%d bytes)" % (zr.GRID, os.path.getsize(zr.GRID)))


if __name__ == "__main__":
    main()
