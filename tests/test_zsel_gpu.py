"""GPU: inducing inputs by greedy conditional variance (`hmogp_select_inducing`, csrc/zsel.hip) against the 50-digit grid
tests/golden/zselgrid.npz and the restatement of tests/zsel_ref.py -- forced pivots element by element, free runs on the designed cases,
the a-posteriori criterion on near-ties, the stop rules, row independence, ties to the existing kernels, `keep`, the refusals, the facade.

Criterion (zsel_ref's docstring): |got - R| <= C S with C = max(16, 4 C_ORACLE) = 16 for L, d, dpiv and trace alike, on the grid's stored rows;
every row is held to the float64 restatement with C_KERNEL + C_ORACLE.  Measured on the MI355X, 2026-10-20, worst over the 52 forced runs:
L 0.404, d 0.608, dpiv 0.149, trace 0.136 against 50 digits (the restatement's own figures); L 0.343, d 0.482, dpiv 0.082, trace 0.036 against
the restatement on every row.  Every case and figure: DESIGN 9s.

Shapes: N in {1, 2, 63, 64, 65, 257, 511, 512, 513, 1025} -- the lane pair (a lane owns two neighbouring rows), the 64-lane wave, the
512-row block, three blocks -- crossed with Mmax in {1, 2, 7, 8, 9, 33} capped at N -- the eight-plane unroll of the chain and four rounds of
it plus one; P = 1 .. 4 and Q in {1, 3} across the cases."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import zsel_ref as zr            # noqa: E402

pytestmark = pytest.mark.gpu

GRID = zr.load_grid()
WHAT = ("L", "d", "dpiv", "trace")
FORCED = [(c["name"], m) for c in zr.FORCED_CASES for m in zr.FORCED_MMAX if m <= c["M"]]
_CACHE = {}


def run(X, var, ell, Mmax, **kw):
    from hetmogp_amd.engine import select_inducing_rows
    return select_inducing_rows(X, var, ell, Mmax, return_factor=True, device=0, **kw)


def forced_run(name, m):
    """The device's forced run of a grid case at Mmax = m and the restatement's: computed once, left unchanged."""
    if (name, m) not in _CACHE:
        e = GRID[name]
        _CACHE[(name, m)] = (run(e["X"], e["var"], e["ell"], m, forced=e["pivots"][:m]),
                             zr.select(e["X"], e["var"], e["ell"], m, forced=e["pivots"][:m]))
    return _CACHE[(name, m)]


def restated_ratios(e, got, ref):
    """Worst ratios of a device run against the float64 restatement of the same run, on EVERY row (scales from the restatement's dpiv)."""
    m, N, k0, G = ref["Mout"], e["X"].shape[0], ref["k0"], zr.gpy_order_cost(e["X"], e["var"], e["ell"])
    if got["Mout"] != m or not np.array_equal(got["pivots"], ref["pivots"]):
        return dict.fromkeys(WHAT, np.inf)
    sd = zr.scale_d(k0, ref["dpiv"], G)
    return dict(L=float(np.max(zr.ratios(got["L"][:, :m], ref["L"][:, :m], zr.scale_L(k0, ref["dpiv"], G)[None, :]))) if m else 0.0,
                d=float(np.max(zr.ratios(got["d"], ref["d"], sd[m]))),
                dpiv=float(np.max(zr.ratios(got["dpiv"], ref["dpiv"], sd[:m]))) if m else 0.0,
                trace=float(np.max(zr.ratios(got["trace"], ref["trace"], zr.scale_trace(k0, ref["dpiv"], ref["trace"], N, G)))))


@pytest.mark.parametrize("name,m", FORCED, ids=["%s-M%d" % nm for nm in FORCED])
def test_forced_pivots_element_by_element(name, m):
    e = GRID[name]
    got, ref = forced_run(name, m)
    assert got["Mout"] == m and np.array_equal(got["pivots"], e["pivots"][:m]) and np.array_equal(got["Z"], e["X"][e["pivots"][:m]])
    assert got["L"].shape == (e["case"]["N"], m) and got["trace"].shape == (m + 1,)
    r50, r64 = zr.prefix_ratios(e, got, m), restated_ratios(e, got, ref)
    print("%-8s Mmax %2d against 50 digits: " % (name, m) + "  ".join("%s %.3f" % (k, r50[k]) for k in WHAT) +
          " | against float64, all rows: " + "  ".join("%s %.3f" % (k, r64[k]) for k in WHAT))
    for k in WHAT:
        assert r50[k] <= zr.c_kernel(k), (k, r50[k])
        assert r64[k] <= zr.c_sum(k), (k, r64[k])
    assert np.all(got["d"][e["pivots"][:m]] == 0.0) and np.all(got["d"] >= 0.0)


@pytest.mark.parametrize("case", zr.FREE_CASES, ids=[c["name"] for c in zr.FREE_CASES])
def test_free_runs_pick_the_grid_pivots(case):
    e = GRID[case["name"]]
    got = run(e["X"], e["var"], e["ell"], case["M"])
    assert got["Mout"] == case["M"] and np.array_equal(got["pivots"], e["pivots"]) and got["pivots"][0] == 0
    sd = zr.scale_d(e["k0"], e["dpiv"], e["G"])
    rd = float(np.max(zr.ratios(got["dpiv"], e["dpiv"], sd[:-1])))
    rt = float(np.max(zr.ratios(got["trace"], e["trace"], zr.scale_trace(e["k0"], e["dpiv"], e["trace"], case["N"], e["G"]))))
    print("%-5s dpiv %.3f trace %.3f" % (case["name"], rd, rt))
    assert rd <= zr.c_kernel("dpiv") and rt <= zr.c_kernel("trace")
    assert np.all(np.diff(got["trace"]) <= 0.0) and abs(got["trace"][0] - case["N"] * e["k0"]) <= zr.EPS * zr.addition_path(case["N"]) * case["N"] * e["k0"]
    half = run(e["X"], e["var"], e["ell"], case["M"], forced=e["pivots"][:case["M"] // 2])           # forced first, then free
    assert np.array_equal(half["pivots"], got["pivots"]) and np.array_equal(half["L"], got["L"]) and np.array_equal(half["d"], got["d"])


def test_exact_duplicates_are_never_picked():
    X, var, ell = zr.duplicates_case()
    got = run(X, var, ell, 100)
    piv = got["pivots"].tolist()
    assert 40 <= got["Mout"] <= 80 and len(set(piv)) == len(piv)
    assert not {p + 40 for p in piv if p < 40} & set(piv) and not {p - 40 for p in piv if 40 <= p < 80} & set(piv)
    assert all(p < 40 or p >= 80 for p in piv)                       # of two identical rows the smaller index is the one picked
    assert np.all(got["d"][got["pivots"]] == 0.0)                    # exactly
    assert zr.a_posteriori(X, var, ell, got["pivots"], zr.c_sum("d")) == []
    assert np.all(got["L"][:, got["Mout"]:] == 0.0)


def test_lattice_meets_the_a_posteriori_criterion():
    X, var, ell = zr.lattice_case()
    got = run(X, var, ell, 40)
    assert got["Mout"] == 40 and got["pivots"][0] == 0 and np.all(got["d"][got["pivots"]] == 0.0)
    assert zr.a_posteriori(X, var, ell, got["pivots"], zr.c_sum("d")) == []


def test_more_picks_than_rows_stops():
    X, var, ell = zr.small_case()
    got = run(X, var, ell, 40)
    assert got["Mout"] <= X.shape[0] and got["L"].shape == (9, 40) and np.all(got["L"][:, got["Mout"]:] == 0.0)
    assert sorted(got["pivots"].tolist()) == sorted(set(got["pivots"].tolist()))
    assert zr.a_posteriori(X, var, ell, got["pivots"], zr.c_sum("d")) == []
    ref = zr.select(X, var, ell, 40)
    assert got["Mout"] == ref["Mout"] == 9 and got["trace"][-1] == 0.0


def test_tol_stop_and_forced_pick_below_the_floor():
    X, var, ell = zr.make_inputs(zr.TOL_CASE)
    M = zr.TOL_CASE["M"]
    ref, got = zr.select(X, var, ell, M, tol=zr.TOL), run(X, var, ell, M, tol=zr.TOL)
    m = ref["Mout"]                                                  # (dpiv is 1e-5 k0 or more away from tol k0 around the stop: CPU test)
    assert 2 < m < M and got["Mout"] == m and np.array_equal(got["pivots"], ref["pivots"])
    assert got["L"].shape == (X.shape[0], M) and np.all(got["L"][:, m:] == 0.0) and np.any(got["L"][:, m - 1] != 0.0)
    assert got["trace"].shape == (m + 1,) and got["dpiv"][-1] > zr.TOL * ref["k0"]
    assert all(v <= zr.c_sum(k) for k, v in restated_ratios(dict(X=X, var=var, ell=ell), got, ref).items())
    Xd, var, ell = zr.duplicates_case()
    f = run(Xd, var, ell, 5, forced=[3, 43])                         # row 43 repeats row 3: after the first pick its d is rounding noise
    assert f["Mout"] == 1 and f["pivots"].tolist() == [3] and np.all(f["L"][:, 1:] == 0.0) and f["d"][43] <= zr.FLOOR * zr.k_zero(var)
    one = run(Xd, var, ell, 5, tol=1.0)                              # d_p = k0 <= tol k0: stops before the first pick
    assert one["Mout"] == 0 and one["trace"].shape == (1,) and abs(one["trace"][0] - 120 * zr.k_zero(var)) <= zr.EPS * zr.addition_path(120) * 120 * zr.k_zero(var) and np.all(one["L"] == 0.0)


def test_rows_do_not_depend_on_the_other_rows():
    """With forced pivots, a row's L and d are the same bits whether the row is computed among all rows or among a subset: another
    position in the lane pair, the wave, the block, another grid."""
    e = GRID["f_N1025"]
    got, _ = forced_run("f_N1025", 33)
    piv = e["pivots"]
    sub = np.unique(np.concatenate([piv, np.random.RandomState(7).choice(1025, 300, replace=False)]))
    sub = sub[np.random.RandomState(8).permutation(len(sub))]        # and another order
    where = {int(r): i for i, r in enumerate(sub)}
    part = run(e["X"][sub], e["var"], e["ell"], 33, forced=[where[int(p)] for p in piv])
    assert part["Mout"] == 33
    assert np.array_equal(part["L"], got["L"][sub]) and np.array_equal(part["d"], got["d"][sub]) and np.array_equal(part["dpiv"], got["dpiv"])


def test_ties_to_the_existing_kernels():
    from hetmogp_amd.engine import rbf_cross_cov
    e = GRID["g_P3"]
    got = run(e["X"], e["var"], e["ell"], e["case"]["M"])
    Z = got["Z"]
    Kzz = sum(rbf_cross_cov(Z, Z, v, l, device=0, exact=True) for v, l in zip(e["var"], e["ell"]))
    sL = zr.scale_L(e["k0"], e["dpiv"], e["G"])
    Lz = got["L"][got["pivots"]]
    assert np.max(np.abs(np.triu(Lz, 1)) / sL[None, :]) <= zr.c_kernel("L")
    worst = float(np.max(zr.ratios(np.tril(Lz), np.linalg.cholesky(Kzz), sL[None, :])))
    print("L[pivots] against the Cholesky factor of sum_q rbf_cross_cov(Z, Z, exact): %.3f" % worst)
    assert worst <= 2.0 * zr.c_kernel("L")                           # two kernel-built factors of one matrix
    # full rank at N = 257: L L^T = sum_q rbf_cross_cov(X, X) to Higham's bound beside the kernel entries' own G ulps
    X = np.random.RandomState(305).rand(257, 3)
    var, c = zr.KERNELS[3]
    ell = c * 0.15
    full = run(X, var, ell, 257)
    assert full["Mout"] == 257 and np.all(full["d"] == 0.0)
    K = sum(rbf_cross_cov(X, X, v, l, device=0) for v, l in zip(var, ell))
    err = float(np.max(np.abs(full["L"] @ full["L"].T - K)) / (zr.EPS * (257 + 2 + zr.gpy_order_cost(X, var, ell)) * zr.k_zero(var)))
    print("full rank, N = 257: |L L^T - K| = %.3f of the bound; d / k0 down to %.2e" % (err, full["dpiv"].min() / zr.k_zero(var)))
    assert err <= 1.0


def test_refusals_are_followed_by_valid_calls():
    from hetmogp_amd import _lib
    ok = zr.abi_call()
    assert ok[0] == 0, ok
    for kw, word in zr.REFUSALS:
        rc, msg = zr.abi_call(**kw)
        assert rc == _lib.E_INVALID and word in msg, (kw, rc, msg)
        assert zr.abi_call()[0] == 0
    rc, msg = zr.abi_call(device=64)
    assert rc == _lib.E_NO_DEVICE
    # more than the device's free memory: refused before any allocation, the message gives the bytes
    N, Mmax = 1 << 20, 1 << 20
    X = np.zeros((N, 1))
    rc, msg = zr.abi_call(N=N, P=1, X=X, Mmax=Mmax, pivots=np.zeros(Mmax, dtype=np.int64), Z=np.zeros((Mmax, 1)), dpiv=np.zeros(Mmax),
                    trace=np.zeros(Mmax + 1))
    import re
    need = re.search(r"need (\d+) bytes", msg)
    assert rc == _lib.E_INVALID and need and float(need.group(1)) >= 8.0 * N * Mmax, (rc, msg)
    X, var, ell = zr.small_case()
    assert run(X, var, ell, 4)["Mout"] == 4


def test_keep_points_come_first():
    import hetmogp_amd as hm
    from hetmogp_amd.kern import RBF
    X_list, var, ell = zr.facade_case()
    kern = [RBF(2, v, l) for v, l in zip(var, ell)]
    keep = np.array([[0.5, 0.5], [0.05, 0.95], [2.0, 2.0]])
    Z, info = hm.select_inducing(X_list, 12, kern, keep=keep, return_info=True)
    assert Z.shape == (12, 2) and np.array_equal(Z[:3], keep)
    assert info["rows"][:3].tolist() == [[-1, 0], [-1, 1], [-1, 2]] and np.all(info["rows"][3:, 0] >= 0)
    for (t, r), z in zip(info["rows"][3:], Z[3:]):
        assert np.array_equal(X_list[t][r], z)
    N0 = sum(x.shape[0] for x in X_list)
    assert info["pivots"][:3].tolist() == [N0, N0 + 1, N0 + 2] and not info["stopped_by_tol"]
    ref = zr.select(np.vstack(X_list + [keep]), var, ell, 12, forced=[N0, N0 + 1, N0 + 2])
    assert np.array_equal(info["pivots"], ref["pivots"])
    assert info["chol_diag_min"] == np.sqrt(np.min(info["cond_var"])) and info["cond_var"].shape == (12,) and info["trace"].shape == (13,)
    Zt, it = hm.select_inducing(X_list, 400, kern, tol=1e-2, return_info=True)
    assert it["stopped_by_tol"] and Zt.shape[0] < 400 and np.min(it["cond_var"]) > 1e-2 * zr.k_zero(np.array(var))


def test_facade_end_to_end():
    """Z = select_inducing(X_list, 16, kern_list) for a 2-D three-task model; SVMOGP(Z=Z, ...) constructs and returns a finite ELBO; the
    residual trace is below a seeded random subset's of the same size (margin 2.6x on the CPU: tests/test_zsel_cpu.py)."""
    import hetmogp_amd as hm
    X_list, var, ell = zr.facade_case()
    rng = np.random.RandomState(11)
    Y = [np.sin(6.0 * X_list[0][:, :1]) + 0.1 * rng.randn(150, 1), (rng.rand(90, 1) < 0.5).astype(float),
         rng.poisson(np.exp(X_list[2][:, 1:2])).astype(float)]
    likelihood = hm.HetLikelihood([hm.Gaussian(sigma=0.3), hm.Bernoulli(), hm.Poisson()])
    kern_list = hm.latent_functions_prior(2, lenghtscale=np.array(ell), variance=np.array(var), input_dim=2)
    Z, info = hm.select_inducing(X_list, 16, kern_list, return_info=True)
    assert Z.shape == (16, 2) and info["rows"].shape == (16, 2) and info["rows"][0].tolist() == [0, 0]
    for (t, r), z in zip(info["rows"], Z):
        assert np.array_equal(X_list[t][r], z)
    assert np.array_equal(hm.select_inducing(X_list, 16, kern_list), Z)
    X = np.vstack(X_list)
    ref = zr.select(X, var, ell, 16)
    assert np.array_equal(info["pivots"], ref["pivots"])
    sub = np.random.RandomState(zr.FACADE_SUBSET_SEED).choice(X.shape[0], 16, replace=False)
    assert info["trace"][-1] < zr.nystrom_trace(X, X[sub], var, ell)
    assert abs(info["trace"][-1] - zr.nystrom_trace(X, Z, var, ell)) <= 1e-9 * info["trace"][0]
    np.random.seed(0)
    model = hm.SVMOGP(X=X_list, Y=Y, Z=Z, kern_list=kern_list, likelihood=likelihood, Y_metadata=likelihood.generate_metadata())
    model.parameters_changed()
    elbo = float(np.ravel(model.log_likelihood())[0])
    print("ELBO %.6f, sqrt(min dpiv) %.4f" % (elbo, info["chol_diag_min"]))
    assert np.isfinite(elbo)
