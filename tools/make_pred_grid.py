#!/usr/bin/env python
"""Writes tests/golden/predgrid.npz: the rows on which `hmogp_predictive` is pinned element by element, with the 50-digit value
R and the condition scale S of the reference's rule from tests/lik_ref_mp.py `predictive_row` -- the yardstick of
tests/test_predgrid_cpu.py and tests/test_predgrid_gpu.py.

Rows.  Per family the distinct (m, v, parameter) of the committed tests/golden/likgrid_<family>.npz with their class (0 bulk / 1 edge) and
group; y is dropped.  Appended, class edge, the rows that grid lacks for this rule:
  v_zero       v = 0 in each dimension in turn and in all of them
  clip_outer   m with exp(f) (Exponential: exp(-f)) next to the 1e-9 and the 1e9 clip at the outermost node of the T = 10 and of the
               T = 20 rule, on either side of it (every family with such a clip: Exponential, Gamma, Beta; Bernoulli and Categorical at the
               1e-9 / 1 - 1e-9 clip of p)
  cancel       HetGaussian: |m_0| from 1e2 to 1e7 with v_0 from 1e-8 to 1e-2, where e2 + sq - m_0^2 cancels
Every family with a rule order has R, S at T = 10 and at T = 20; Gaussian, Student and Categorical (always T = 10) have one set, stored as
T = 0, the order `engine.predictive` is asked for.

Rows that overflow in float64 after the reference's own clips (the float64 oracle returns a non-finite element where the rule's value is a
real number) are marked `nf` with the class (1 +inf, 2 -inf, 3 NaN) of every oracle element; only the first 2 % (likgrid.NONFINITE_SHARE,
counted against the rows kept) are kept, in row order, the others are left out.  A Categorical row whose 1 + sum_k exp(f_k) overflows at some
node while every output stays finite (float64 has 0 -> clip where the rule has a quotient) is kept and marked `ovf`: R is the rule's value,
which float64 does not compute there, so only the class (finite) is asserted.  Student's NaN mean (nu <= 1) and +inf variance
(nu <= 2) are the contract's own values, no overflow: those elements are compared by class, their rows are not marked.

Keys: <tag>__m, __v [n, J], __param [n], __cls, __group, __ovf [n], __R<T>, __S<T> [n, 2 Jp], __nf<T> [n, 2 Jp]; `spec` = JSON {tag: [name, kw0,
param_name, groups, Ts]}.  No random numbers: the rows are those of the committed grids plus fixed lists, computed one row at a time in
a process pool whose results are gathered in row order -- the arrays regenerate bit for bit.

usage: python tools/make_pred_grid.py [out.npz]      (about two minutes on 8 CPUs)"""
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import likgrid as lg  # noqa: E402

X10 = float(np.polynomial.hermite.hermgauss(10)[0].max())
X20 = float(np.polynomial.hermite.hermgauss(20)[0].max())
L9 = float(np.log(1e9))
RULE_ORDERS = {"Gaussian": (0,), "Student": (0,), "Categorical": (0,)}


def orders(name):
    return RULE_ORDERS.get(name, (10, 20))


def designed_rows(name, J):
    """[(m, v, group)] appended to a family's rows."""
    rows = []
    base = [0.3, -0.7, 1.1, -0.2, 0.6][:J]
    for d in list(range(J)) + [None]:
        v = [0.5] * J
        for k in range(J):
            if d is None or k == d:
                v[k] = 0.0
        rows.append((base, v, "v_zero"))
        rows.append(([-b for b in base], v, "v_zero"))
    if name in ("Exponential", "Gamma", "Beta", "Bernoulli", "Categorical"):
        for xmax in (X10, X20):
            for vv in (0.5, 4.0):
                for sign in (1.0, -1.0):
                    for off in (-1e-3, 1e-3, -0.4, 0.4):
                        m0 = sign * (L9 + off - xmax * np.sqrt(2.0 * vv))      # the outermost node at sign * (log 1e9 + off)
                        for d in range(min(J, 2)):
                            m = list(base)
                            v = [0.5] * J
                            m[d], v[d] = float(m0), vv
                            rows.append((m, v, "clip_outer"))
    if name == "HetGaussian":
        for m0 in (1e2, -1e3, 1e4, -1e5, 1e6, 1e7):
            for v0 in (1e-8, 1e-5, 1e-2):
                for m1, v1 in ((0.0, 0.5), (-3.0, 1e-3), (2.0, 2.0)):
                    rows.append(([m0, m1], [v0, v1], "cancel"))
    return rows


def family_rows(path):
    g = lg.LikGrid(path)
    groups = list(g.groups)
    seen, rows = set(), []
    for n in range(g.n):
        key = (g.m[n].tobytes(), g.v[n].tobytes(), float(g.param[n]) if g.param_name else 0.0)
        if key in seen:
            continue
        seen.add(key)
        rows.append((g.m[n].copy(), g.v[n].copy(), float(g.param[n]), int(g.cls[n]), int(g.group[n])))
    p0 = float(g.param[0])
    for m, v, grp in designed_rows(g.name, g.J):
        if grp not in groups:
            groups.append(grp)
        params = sorted(set(float(p) for p in g.param)) if g.param_name else [p0]
        for p in params[:3] if g.name == "Student" else params[:1]:
            rows.append((np.array(m, float), np.array(v, float), p, lg.EDGE, groups.index(grp)))
    return g, groups, rows


def _kw(g, p):
    kw = g.kw(p)
    return {k: a for k, a in kw.items() if a is not None}


def oracle_rows(name, kw, m, v, T):
    """The float64 oracle on rows that share kw: [n, 2 Jp]."""
    from oracle import likelihoods_oracle as lo
    with np.errstate(all="ignore"):
        mean, var = lo.predictive(name, m, v, **kw) if name in ("Gaussian", "Student", "Categorical") else lo.predictive(name, m, v, gh_T=T, **kw)
    return np.hstack([np.asarray(mean, float).reshape(m.shape[0], -1), np.asarray(var, float).reshape(m.shape[0], -1)])


def oracle_all(name, param_name, kw0, m, v, param, T):
    out = None
    for p in (np.unique(param) if param_name else [0.0]):
        idx = np.where(param == p)[0] if param_name else np.arange(m.shape[0])
        kw = dict(kw0)
        if param_name:
            kw[param_name] = float(p)
        o = oracle_rows(name, {k: a for k, a in kw.items() if a is not None}, m[idx], v[idx], T)
        if out is None:
            out = np.zeros((m.shape[0], o.shape[1]))
        out[idx] = o
    return out


def _mp_row(task):
    import lik_ref_mp
    name, kw, m, v, T = task
    return lik_ref_mp.predictive_row_f64(name, m, v, T or 10, **kw)


def select(path):
    """Everything of one family's block but the 50-digit values: (tag, LikGrid, spec entry, arrays {m, v, param, cls, group, ovf, nf<T>})."""
    tag = lg.tag_of(path)
    g, groups, rows = family_rows(path)
    m, v = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    param, cls, grp = np.array([r[2] for r in rows]), np.array([r[3] for r in rows], np.uint8), np.array([r[4] for r in rows], np.uint8)
    Ts = orders(g.name)
    orc = {T: oracle_all(g.name, g.param_name, g.kw0, m, v, param, T) for T in Ts}
    contract = np.zeros(orc[Ts[0]].shape, bool)            # elements that are NaN / inf by the contract itself
    if g.name == "Student":
        contract[:, 0], contract[:, 1] = param <= 1.0, param <= 2.0
    over = np.zeros(len(rows), bool)
    for T in Ts:
        over |= np.any(~np.isfinite(orc[T]) & ~contract, axis=1)
    allowed = int(lg.NONFINITE_SHARE * int((~over).sum()))
    keep = ~over | (np.cumsum(over) <= allowed)
    ovf = np.zeros(len(rows), bool)
    if g.name == "Categorical":      # 1 + sum_k exp(f_k) overflows at some node although every output stays finite (inf / inf clipped): float64
        with np.errstate(over="ignore"):   # does not compute the rule there and the outputs do not show it -- kept, marked `ovf`, class only
            ovf = ~over & ~np.isfinite(1.0 + np.exp(np.minimum(m + X10 * np.sqrt(2.0 * v), 709.782712893384)).sum(1))
    assert not np.any((over | ovf) & (cls == lg.BULK))
    arrays = {"m": m[keep], "v": v[keep], "param": param[keep], "cls": cls[keep], "group": grp[keep], "ovf": ovf[keep].astype(np.uint8)}
    for T in Ts:
        nf = lg.classes(orc[T][keep])
        nf[~over[keep]] = 0
        arrays["nf%d" % T] = nf
    return tag, g, [g.name, g.kw0, g.param_name, groups, list(Ts)], arrays


def build(processes=8, only=None):
    spec, out, tasks, where = {}, {}, [], []
    for path in lg.grid_files():
        if only is not None and lg.tag_of(path) not in only:
            continue
        tag, g, spec[tag], arrays = select(path)
        out.update({"%s__%s" % (tag, k): a for k, a in arrays.items()})
        m, v, param = arrays["m"], arrays["v"], arrays["param"]
        for T in spec[tag][4]:
            shape = arrays["nf%d" % T].shape
            out["%s__R%d" % (tag, T)] = np.zeros(shape)
            out["%s__S%d" % (tag, T)] = np.zeros(shape)
            for n in range(m.shape[0]):
                tasks.append((g.name, _kw(g, param[n]), [float(a) for a in m[n]], [float(a) for a in v[n]], T))
                where.append((tag, T, n))
    if processes > 1:
        with multiprocessing.Pool(processes) as pool:
            res = pool.map(_mp_row, tasks, chunksize=4)
    else:
        res = [_mp_row(t) for t in tasks]
    for (tag, T, n), (R, S, real) in zip(where, res):
        out["%s__R%d" % (tag, T)][n], out["%s__S%d" % (tag, T)][n] = R, S
        if np.any(real & ~np.isfinite(R)) and not np.any(out["%s__nf%d" % (tag, T)][n]):       # a real value float64 cannot hold where the
            raise AssertionError((tag, T, n, "the rule overflows float64 but the oracle is finite"))  # oracle is finite: not met
    out["spec"] = np.array(json.dumps(spec, sort_keys=True))
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "predgrid.npz")
    g = build()
    np.savez_compressed(path, **g)
    spec = json.loads(str(g["spec"]))
    for tag in sorted(spec):
        nfr = np.zeros(g[tag + "__m"].shape[0], bool)
        for T in spec[tag][4]:
            nfr |= np.any(g["%s__nf%d" % (tag, T)] != 0, axis=1)
        print("%-16s %5d rows (%d bulk), %d marked non-finite, %d marked ovf" % (tag, len(nfr), int((g[tag + "__cls"] == 0).sum()), int(nfr.sum()),
                                                                                  int(g[tag + "__ovf"].sum())))
    print("%s: %d bytes" % (path, os.path.getsize(path)))
