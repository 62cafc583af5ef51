"""float64 NumPy restatement of `hmogp_select_inducing` (csrc/zsel.hip) -- inducing inputs chosen from the data by greedy
conditional variance, i.e. pivoted incomplete Cholesky of K_ff under k = sum_q s2_q exp(-r_q^2 / 2) --, free and with forced pivots; the
scales, the constants, the criterion and the designed cases of its grid tests/golden/zselgrid.npz (tools/make_zsel_grid.py; 50-digit
values from tests/zsel_ref_mp.py).

The iteration, as include/hetmogp_hip.h states it:  d_i = k0;  for j = 0 .. Mmax-1:  p_j = forced[j] or argmax d (ties to the smallest
index);  stop with Mout = j if d_p <= max(tol, 2^-40) k0;  c_i = (k(x_i, x_p) - sum_{l<j} L_il L_pl) / sqrt(d_p), one chain over l per
row;  L_ij = c_i,  d_i = max(d_i - c_i^2, 0),  d_p = 0.   k in GPy's rounding order, the sum over q from left to right.

Criterion with forced pivots, element by element against the 50-digit values R:  |got - R| <= C S  with
  S_L(i, j) = 2^-52 (j + 2 + G) sqrt(k0) sqrt(k0 / dmin_j),  dmin_j = min_{l <= j} dpiv_l of the 50-digit run
  S_d(j)    = 2^-52 (j + 2 + G) k0 sqrt(k0 / dmin_j)         for dpiv_j and, with j = Mout (dmin over every pick), for the final d
  S_tr(j)   = N S_d(j) + 2^-52 PATH(N) trace_j               PATH(N) = 9 + ceil(log2 ceil(N / 512)), the device's longest addition path
                                                             (the restatement's halving tree, ceil(log2 N) deep, is never longer)
  G         = sum_q s2_q (2 max_i |x_i|^2 / l_q^2) / k0      what GPy's rounding order costs a kernel entry, in ulps of k0
G is the one change to the scales the issue states (it has j + 2 alone).  With those, this file measured 83.3 on L and 121.2 on d (f_N65:
P = 1, l = 0.05), far beyond the 8 at which the issue says the scale is wrong and not the constant.  The cause is the contract's own
rounding order: r2 = -2 x.z + (|x|^2 + |z|^2) cancels from terms of size up to 4 max |x|^2, so r2 carries 2^-52 4 max |x|^2 and
k_q = s2_q exp(-r2 / (2 l_q^2)) carries 2^-52 k_q 2 max |x|^2 / l_q^2 <= 2^-52 s2_q G_q: 800 ulps at l = 0.05 on [0, 1], 6 .. 9 at the
P > 1 cases.  That enters every column as a fresh error of the same kind as the chain's j + 2 roundings, hence beside them.  (The same
effect made tests/joint_ref.py's C_ORACLE 128.)
C_ORACLE: the largest ratio of THIS file against the grid, rounded up to the next power of two (`python tools/make_zsel_grid.py
--measure` prints the raw figures, tests/test_zsel_cpu.py re-measures them); the device gets C_KERNEL = max(16, 4 C_ORACLE), DESIGN 9k's
rule.  The issue's pilot (longdouble standing in for 50 digits) had the restatement within 0.25 .. 0.44 of S_L."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

EPS = 2.0 ** -52
FLOOR = 2.0 ** -40                 # HMOGP_ZSEL_FLOOR
GRID = os.path.join(HERE, "golden", "zselgrid.npz")
ROWS_PER_BLOCK = 512               # rows of one block of the step kernel (a lane owns two rows, 256 lanes)
GAP_MIN = 1e-9                     # designed free cases: (d_(1) - d_(2)) / k0 at every pick j >= 1
DPIV_MIN = 1e-6                    # ... and dpiv / k0
FULL_ROWS_MAX = 65                 # forced cases up to this many rows store every row of L and d; larger ones a subset
SUBSET_ROWS = 96

# Two kernel sets with unequal variances and lengthscales (the second entry: multiples of the case's base lengthscale).  The forced cases'
# base lengthscale per input dimension lets 33 picks stay above the floor while d / k0 falls to 1e-3 (P = 1), 1e-8 (P = 2), 1e-4 (P = 3)
# and 1e-3 (P = 4): the scales' factor sqrt(k0 / dmin) is exercised over four decades.
KERNELS = {1: (np.array([1.3]), np.array([1.0])), 3: (np.array([0.7, 1.6, 0.4]), np.array([0.8, 1.0, 1.7]))}
ELL_OF_P = {1: 0.05, 2: 0.8, 3: 1.2, 4: 1.2}

# Forced pivots, element by element: N around the lane pair (1, 2), the wave and its pair boundary (63, 64, 65), inside one block (257),
# the block (511, 512, 513) and three blocks (1025); Mmax around the unroll of eight planes (7, 8, 9), one and two picks, and four full
# unroll rounds plus one (33); every input dimension and both kernel sets across the cases.  One 50-digit run per case at the largest
# Mmax: with forced pivots a run at a smaller Mmax is its prefix.
FORCED_N = (1, 2, 63, 64, 65, 257, 511, 512, 513, 1025)
FORCED_MMAX = (1, 2, 7, 8, 9, 33)
FORCED_CASES = tuple(dict(name="f_N%d" % n, N=n, P=1 + i % 4, Q=(1, 3)[(i // 2) % 2], seed=100 + i, M=min(33, n), ell=ELL_OF_P[1 + i % 4])
                     for i, n in enumerate(FORCED_N))
# Free runs whose pivots must equal the 50-digit free run's exactly: random inputs in [0, 1]^P, gaps asserted on the CPU
FREE_CASES = (
    dict(name="g_P1", N=300, P=1, Q=3, seed=201, M=10, ell=0.2),
    dict(name="g_P2", N=513, P=2, Q=1, seed=202, M=20, ell=0.3),
    dict(name="g_P3", N=400, P=3, Q=3, seed=203, M=24, ell=0.3),
    dict(name="g_P4", N=1025, P=4, Q=1, seed=204, M=24, ell=0.8),
)
CASES = FORCED_CASES + FREE_CASES
CASE_BY_NAME = {c["name"]: c for c in CASES}
REGEN_CASES = ("f_N2", "f_N63", "g_P1")         # what tests/test_zsel_cpu.py regenerates (seconds in 50-digit arithmetic)

# measured 2026-10-20 on the CPU, this file against the grid; the raw figure beside each constant (tools/make_zsel_grid.py --measure)
C_ORACLE = {
    "L": 0.5,          # raw 0.405 (f_N65, Mmax 33); the issue's pilot: 0.25 .. 0.44
    "d": 1.0,          # raw 0.608 (f_N65, Mmax 2)
    "dpiv": 0.25,      # raw 0.149 (f_N63)
    "trace": 0.25,     # raw 0.136 (f_N63, Mmax 1)
}


def c_oracle(what):
    return float(C_ORACLE[what])


def c_kernel(what):
    return max(16.0, 4.0 * C_ORACLE[what])


def c_sum(what):
    """Bound between a device result and this file's float64 value: each within its own constant of R."""
    return c_kernel(what) + c_oracle(what)


# ------------------------------------------------------------------------------------------------------------ designed inputs
def kernels(case):
    var, c = KERNELS[case["Q"]]
    return var.copy(), c * case["ell"]


def make_inputs(case):
    """(X, variance, lengthscale): seeded uniform rows in [0, 1]^P."""
    X = np.random.RandomState(case["seed"]).rand(case["N"], case["P"])
    var, ell = kernels(case)
    return X, var, ell


def forced_pivots(case):
    """The forced cases' pivots: those of this file's own free run (so that d stays as large as a selection keeps it); being forced, a
    near-tie in that run is of no consequence."""
    X, var, ell = make_inputs(case)
    r = select(X, var, ell, case["M"])
    assert r["Mout"] == case["M"], (case["name"], r["Mout"])
    return r["pivots"]


def stored_rows(case, pivots):
    """Rows whose L and d the grid stores: all of them up to FULL_ROWS_MAX, else the pivots, the rows around every block boundary and
    the end, and a seeded sample."""
    N = case["N"]
    if N <= FULL_ROWS_MAX:
        return np.arange(N)
    edge = [0, 1, N - 2, N - 1] + [b + o for b in range(ROWS_PER_BLOCK, N, ROWS_PER_BLOCK) for o in (-2, -1, 0, 1)] + \
           [b + o for b in range(64, min(N, 257), 64) for o in (-1, 0)]
    fixed = np.unique(np.concatenate([np.asarray(pivots), np.array([e for e in edge if 0 <= e < N])]))
    rest = np.setdiff1d(np.arange(N), fixed)
    extra = np.random.RandomState(9000 + case["seed"]).choice(rest, SUBSET_ROWS - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, extra]))


# ------------------------------------------------------------------------------------------------------------ the restatement
def k_column(X, xp, var, ell):
    """k(x_i, x_p) for every row: GPy's rounding order per kernel, the sum over q from left to right."""
    X = np.asarray(X, float)
    P = X.shape[1]
    dot, xs, zs = X[:, 0] * xp[0], X[:, 0] * X[:, 0], xp[0] * xp[0]
    for p in range(1, P):
        dot, xs, zs = dot + X[:, p] * xp[p], xs + X[:, p] * X[:, p], zs + xp[p] * xp[p]
    r2 = np.maximum(-2.0 * dot + (xs + zs), 0.0)
    k = None
    for q in range(len(var)):
        r = np.sqrt(r2) / ell[q]
        t = var[q] * np.exp(-0.5 * (r * r))
        k = t if k is None else k + t
    return k


def k_matrix(X, Z, var, ell):
    return np.stack([k_column(X, z, var, ell) for z in np.asarray(Z, float)], 1)


def k_zero(var):
    k0 = var[0]
    for q in range(1, len(var)):
        k0 = k0 + var[q]
    return float(k0)


def tree_sum(a):
    """Halving tree, ceil(log2 n) additions deep."""
    a = np.array(a, dtype=float)
    n = a.shape[0]
    while n > 1:
        h = (n + 1) // 2
        a[:n - h] += a[h:n]
        n = h
    return float(a[0])


def addition_path(N):
    """The device's longest addition path of sum d: pair 1 + wave 6 + block 2 + the tree over the blocks' partials."""
    nb = -(-int(N) // ROWS_PER_BLOCK)
    return 9 + int(np.ceil(np.log2(nb)))


def select(X, var, ell, Mmax, tol=0.0, forced=None, history=False):
    """The iteration in float64.  Returns Mout, pivots, Z, dpiv, trace (Mout + 1), L (N, Mmax), d (N); with history also dhist
    (Mout + 1, N): d before every pick and after the last."""
    X = np.asarray(X, float)
    var, ell = np.asarray(var, float), np.asarray(ell, float)
    N = X.shape[0]
    forced = np.zeros(0, dtype=np.int64) if forced is None else np.asarray(forced, dtype=np.int64)
    k0 = k_zero(var)
    thr = max(tol, FLOOR) * k0
    d = np.full(N, k0)
    L = np.zeros((N, Mmax))
    piv, dpiv, trace, dh = [], [], [tree_sum(d)], [d.copy()]
    for j in range(min(Mmax, N)):
        p = int(forced[j]) if j < len(forced) else int(np.argmax(d))          # (argmax: the first of equal maxima)
        if not d[p] > thr:
            break
        s = np.zeros(N)
        for l in range(j):
            s = s + L[:, l] * L[p, l]
        c = (k_column(X, X[p], var, ell) - s) / np.sqrt(d[p])
        piv.append(p), dpiv.append(d[p])
        L[:, j] = c
        d = np.maximum(d - c * c, 0.0)
        d[p] = 0.0
        trace.append(tree_sum(d))
        if history:
            dh.append(d.copy())
    piv = np.array(piv, dtype=np.int64)
    out = dict(Mout=len(piv), pivots=piv, Z=X[piv], dpiv=np.array(dpiv), trace=np.array(trace), L=L, d=d, k0=k0)
    if history:
        out["dhist"] = np.stack(dh)
    return out


def top_two_gaps(dhist, k0):
    """(d_(1) - d_(2)) / k0 before every pick j >= 1 of a free run (dhist from select(history=True))."""
    out = []
    for j in range(1, dhist.shape[0] - 1):
        t = np.partition(dhist[j], -2)[-2:]
        out.append((t[1] - t[0]) / k0)
    return np.array(out)


# ------------------------------------------------------------------------------------------------------------ scales and criterion
def dmin_upto(dpiv):
    """dmin_j = min_{l <= j} dpiv_l for j = 0 .. Mout-1, and once more at j = Mout (every pick)."""
    dpiv = np.asarray(dpiv, float)
    if len(dpiv) == 0:
        return np.array([np.inf])
    m = np.minimum.accumulate(dpiv)
    return np.concatenate([m, m[-1:]])


def gpy_order_cost(X, var, ell):
    """G: the error GPy's rounding order leaves in a kernel entry, in units of 2^-52 k0 (module docstring)."""
    X, var, ell = np.asarray(X, float), np.asarray(var, float), np.asarray(ell, float)
    x2 = float(np.max(np.sum(X * X, 1)))
    return float(np.sum(var * (2.0 * x2 / (ell * ell))) / k_zero(var))


def scale_L(k0, dpiv_ref, G):
    """S_L(., j) for j = 0 .. Mout-1 (the same for every row)."""
    dm = dmin_upto(dpiv_ref)[:-1]
    j = np.arange(len(dm))
    return EPS * (j + 2 + G) * np.sqrt(k0) * np.sqrt(k0 / dm)


def scale_d(k0, dpiv_ref, G):
    """S_d(j) for j = 0 .. Mout: entries j < Mout for dpiv_j and for d before pick j, entry Mout for the final d."""
    dm = dmin_upto(dpiv_ref)
    j = np.arange(len(dm))
    return EPS * (j + 2 + G) * k0 * np.sqrt(k0 / dm)


def scale_trace(k0, dpiv_ref, trace_ref, N, G):
    return N * scale_d(k0, dpiv_ref, G)[:len(trace_ref)] + EPS * addition_path(N) * np.asarray(trace_ref, float)


def ratios(got, R, scale):
    """|got - R| / scale per entry (0 where both are equal, inf where a value is not finite)."""
    got, R, scale = np.asarray(got, float), np.asarray(R, float), np.asarray(scale, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - R) / scale
    r = np.where(got == R, 0.0, r)
    return np.where(np.isfinite(got), r, np.inf)


def prefix_ratios(entry, res, Mmax):
    """Worst ratios {L, d, dpiv, trace} of a forced run `res` (select's dict or the device's, L (N, Mmax)) at Mmax <= the case's M against
    the loaded grid case: the run is the prefix of the stored one."""
    m, N, k0, rows = int(Mmax), entry["case"]["N"], entry["k0"], entry["rows"]
    if res["Mout"] != m:
        return dict(L=np.inf, d=np.inf, dpiv=np.inf, trace=np.inf)
    dp, G = entry["dpiv"][:m], entry["G"]
    sd = scale_d(k0, dp, G)
    return dict(L=float(np.max(ratios(np.asarray(res["L"])[rows][:, :m], entry["L"][:, :m], scale_L(k0, dp, G)[None, :]))),
                d=float(np.max(ratios(np.asarray(res["d"])[rows], entry["d_after"][m], sd[m]))),
                dpiv=float(np.max(ratios(res["dpiv"], dp, sd[:m]))),
                trace=float(np.max(ratios(res["trace"], entry["trace"][:m + 1], scale_trace(k0, dp, entry["trace"][:m + 1], N, G)))))


def a_posteriori(X, var, ell, pivots, C):
    """The near-tie criterion: given a run's own pivots, this file's forced restatement's d before pick j must have
    d(p_j) >= max_i d_i - 2 C S_d(j), and among the rows within that band of the maximum no EXACTLY tied row may have a smaller index than
    p_j.  Returns the list of violations (empty = pass)."""
    pivots = np.asarray(pivots, dtype=np.int64)
    r = select(X, var, ell, len(pivots), forced=pivots, history=True)
    bad = []
    if r["Mout"] != len(pivots):
        return [("restatement stopped at", r["Mout"])]
    sd = scale_d(r["k0"], r["dpiv"], gpy_order_cost(X, var, ell))
    for j, p in enumerate(pivots):
        dj = r["dhist"][j]
        band = 2.0 * C * sd[j]
        if not dj[p] >= np.max(dj) - band:
            bad.append((j, int(p), "below the band", float(np.max(dj) - dj[p]), float(band)))
        tied = np.nonzero(dj == dj[p])[0]
        if tied[0] < p:
            bad.append((j, int(p), "an exactly tied row with a smaller index", int(tied[0])))
    return bad


# ------------------------------------------------------------------------------------------------------------ the grid
def load_grid(path=GRID):
    g = np.load(path)
    out = {}
    for c in CASES:
        k = c["name"] + "/"
        e = dict(case=c, X=g[k + "X"], var=g[k + "var"], ell=g[k + "ell"], pivots=g[k + "pivots"], dpiv=g[k + "dpiv"], trace=g[k + "trace"],
                 k0=float(g[k + "k0"]))
        e["G"] = gpy_order_cost(e["X"], e["var"], e["ell"])
        if k + "L" in g.files:
            mm = [m for m in FORCED_MMAX if m <= c["M"]]
            e.update(rows=g[k + "rows"], L=g[k + "L"], d_after={m: g[k + "d_after"][i] for i, m in enumerate(mm)}, mmax=mm)
        out[c["name"]] = e
    return out


# ------------------------------------------------------------------------------------------------------------ further designed cases
def duplicates_case():
    """Rows 40 .. 79 repeat rows 0 .. 39 exactly, in 2-D."""
    X = np.random.RandomState(301).rand(120, 2)
    X[40:80] = X[:40]
    var, c = KERNELS[3]
    return X, var.copy(), c * 0.25


def lattice_case():
    """A regular 1-D lattice: symmetric rows tie up to rounding."""
    X = np.linspace(0.0, 1.0, 129)[:, None]
    var, c = KERNELS[1]
    return X, var.copy(), c * 0.06


def small_case():
    """Mmax > N: nine rows."""
    X = np.random.RandomState(302).rand(9, 3)
    var, c = KERNELS[3]
    return X, var.copy(), c * 0.4


TOL_CASE = dict(name="tol", N=257, P=2, Q=3, seed=303, M=33, ell=0.6)
TOL = 1e-3
TOL_MARGIN = 1e-9                  # |dpiv - tol k0| / k0 at the stopping pick and the one before: asserted on the CPU


FACADE_SUBSET_SEED = 306


def facade_case():
    """A 2-D three-task model for the facade: (X_list, variances, lengthscales).  Lengthscales at which sixteen well-placed points resolve
    most of the unit square: the greedy choice's residual trace is 2.6x below the seeded random subset's (asserted on the CPU)."""
    rng = np.random.RandomState(304)
    X_list = [rng.rand(n, 2) for n in (150, 90, 200)]
    return X_list, [1.0, 0.6], [0.5, 0.3]


def nystrom_trace(X, Z, var, ell):
    """tr(K_ff - Q_ff) for given inducing inputs Z, in float64 (Cholesky of K_ZZ)."""
    Kzz, Kxz = k_matrix(Z, Z, var, ell), k_matrix(X, Z, var, ell)
    A = np.linalg.solve(np.linalg.cholesky(Kzz), Kxz.T)
    return float(X.shape[0] * k_zero(var) - np.sum(A * A))


# ------------------------------------------------------------------------------------------------------------ the C ABI
def abi_call(**kw):
    """hmogp_select_inducing on a small valid problem with single arguments replaced: (return code, message)."""
    from hetmogp_amd import _lib
    a = dict(device=0, N=5, P=2, X=np.random.RandomState(1).rand(5, 2), Q=2, variance=np.array([1.0, 0.5]), lengthscale=np.array([0.3, 0.2]),
             Mmax=3, tol=0.0, n_forced=0, forced=None, pivots=np.zeros(3, dtype=np.int64), Z=np.zeros((3, 2)), dpiv=np.zeros(3),
             trace=np.zeros(4), L=None, d=None, Mout=ctypes.c_int32(-7))
    a.update(kw)
    fp = lambda v: None if v is None else v.ctypes.data_as(_lib.c_double_p)
    ip = lambda v: None if v is None else v.ctypes.data_as(_lib.c_int64_p)
    X, var, ell = [None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.float64) for k in ("X", "variance", "lengthscale")]
    fo = None if a["forced"] is None else np.ascontiguousarray(a["forced"], dtype=np.int64)
    rc = _lib.lib.hmogp_select_inducing(a["device"], a["N"], a["P"], fp(X), a["Q"], fp(var), fp(ell), a["Mmax"], a["tol"], a["n_forced"], ip(fo),
                                        ip(a["pivots"]), fp(a["Z"]), fp(a["dpiv"]), fp(a["trace"]), fp(a["L"]), fp(a["d"]),
                                        None if a["Mout"] is None else ctypes.byref(a["Mout"]))
    msg = _lib.lib.hmogp_last_error(None)
    return rc, (msg or b"").decode()


REFUSALS = [
    (dict(N=0), "N"), (dict(P=0), "P"), (dict(P=5), "P"), (dict(Q=0), "Q"), (dict(Q=9), "Q"), (dict(Mmax=0), "Mmax"),
    (dict(X=np.array([[0.1, np.inf]] + [[0.0, 0.0]] * 4)), "X"), (dict(X=np.array([[np.nan, 0.2]] + [[0.0, 0.0]] * 4)), "X"),
    (dict(variance=np.array([1.0, 0.0])), "variance"), (dict(variance=np.array([np.inf, 1.0])), "variance"),
    (dict(lengthscale=np.array([0.3, -0.2])), "lengthscale"), (dict(lengthscale=np.array([np.nan, 0.2])), "lengthscale"),
    (dict(tol=-1e-3), "tol"), (dict(tol=float("nan")), "tol"),
    (dict(n_forced=-1), "n_forced"), (dict(n_forced=4, forced=np.arange(4)), "n_forced"),
    (dict(n_forced=2, forced=np.array([1, 5])), "forced"), (dict(n_forced=2, forced=np.array([-1, 2])), "forced"),
    (dict(n_forced=2, forced=np.array([2, 2])), "repeated"), (dict(n_forced=1, forced=None), "forced"),
    (dict(X=None), "X"), (dict(variance=None), "variance"), (dict(lengthscale=None), "lengthscale"), (dict(pivots=None), "pivots"),
    (dict(Z=None), "Z"), (dict(dpiv=None), "dpiv"), (dict(trace=None), "trace"), (dict(Mout=None), "Mout"),
]
