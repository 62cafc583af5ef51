"""The 50-digit restatement of `hmogp_select_inducing` in mpmath: the iteration of tests/zsel_ref.py with every quantity exact
up to 50 digits -- the squared distances from the double inputs themselves (no GPy rounding order: that order is a property of float64
arithmetic, what it costs shows in C_ORACLE), the exponentials, the chain, the root, the downdate.  Free (argmax d, ties to the smallest
index) or with forced pivots.  tools/make_zsel_grid.py rounds the results to double; tests/test_zsel_cpu.py regenerates a subset."""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50


def k_column(X, xp, var, ell):
    """[k(x_i, x_p)] over the rows of X (lists of mpf)."""
    inv = [1 / (mpf(float(l)) ** 2) for l in ell]
    v = [mpf(float(s)) for s in var]
    out = []
    for x in X:
        r2 = sum(((a - b) ** 2 for a, b in zip(x, xp)), mpf(0))
        out.append(sum((vq * mp.exp(-r2 * iq / 2) for vq, iq in zip(v, inv)), mpf(0)))
    return out


def select(X, var, ell, Mmax, forced=None, d_after=()):
    """Mout = min(Mmax, N) picks without a stop rule (the designed cases stay far above the floor; asserted).  Returns pivots, dpiv, trace
    (Mout + 1), L (N, Mout), and d_after[m] = d after m picks for every m asked for -- all rounded to double."""
    Xd = np.asarray(X, float)
    N = Xd.shape[0]
    Xm = [[mpf(float(v)) for v in row] for row in Xd]
    forced = [] if forced is None else [int(p) for p in forced]
    k0 = sum((mpf(float(s)) for s in var), mpf(0))
    d = [k0] * N
    L = [[] for _ in range(N)]
    piv, dpiv, trace, keep = [], [], [sum(d, mpf(0))], {}
    M = min(int(Mmax), N)
    if 0 in d_after:
        keep[0] = list(d)
    for j in range(M):
        if j < len(forced):
            p = forced[j]
        else:
            p = max(range(N), key=lambda i: (d[i], -i))
        assert d[p] > mpf(2) ** -40 * k0, "a designed case must stay above the floor"
        kc = k_column(Xm, Xm[p], var, ell)
        rs = mp.sqrt(d[p])
        Lp = list(L[p])
        piv.append(p), dpiv.append(d[p])
        for i in range(N):
            c = (kc[i] - mp.fdot(L[i], Lp)) / rs if j else kc[i] / rs
            L[i].append(c)
            d[i] = max(d[i] - c * c, mpf(0))
        d[p] = mpf(0)
        trace.append(sum(d, mpf(0)))
        if j + 1 in d_after:
            keep[j + 1] = list(d)
    f = lambda a: np.array([float(v) for v in a])
    return dict(pivots=np.array(piv, dtype=np.int64), dpiv=f(dpiv), trace=f(trace), k0=float(k0),
                L=np.array([[float(v) for v in row] for row in L]).reshape(N, M), d_after={m: f(v) for m, v in keep.items()})
