"""Inducing inputs by greedy conditional variance, CPU side: the float64 restatement (tests/zsel_ref.py) against the 50-digit
grid tests/golden/zselgrid.npz, the grid's regeneration, the criterion's sensitivity, the designed cases' gaps, the properties of the
restated factor, the new C-ABI symbol with its host-side refusals, and the facade's argument checks.  The device is held to the same grid
in tests/test_zsel_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import zsel_ref as zr            # noqa: E402

GRID = zr.load_grid()
WHAT = ("L", "d", "dpiv", "trace")


@pytest.fixture(scope="module")
def free_runs():
    """The float64 free run of every designed free case, with the history of d, computed once."""
    return {c["name"]: zr.select(GRID[c["name"]]["X"], GRID[c["name"]]["var"], GRID[c["name"]]["ell"], c["M"], history=True)
            for c in zr.FREE_CASES}


def test_cases_cover_the_issue():
    assert tuple(c["N"] for c in zr.FORCED_CASES) == (1, 2, 63, 64, 65, 257, 511, 512, 513, 1025) and zr.FORCED_MMAX == (1, 2, 7, 8, 9, 33)
    assert {c["P"] for c in zr.FORCED_CASES} == {1, 2, 3, 4} == {c["P"] for c in zr.FREE_CASES}
    assert {c["Q"] for c in zr.FORCED_CASES} == {1, 3} == {c["Q"] for c in zr.FREE_CASES}
    for Q, (var, c) in zr.KERNELS.items():
        assert len(var) == Q and (Q == 1 or (len(set(var)) == Q and len(set(c)) == Q))      # unequal variances and lengthscales
    assert zr.FLOOR == 2.0 ** -40 and zr.addition_path(1) == 9 and zr.addition_path(513) == 10 and zr.addition_path(1025) == 11


def test_grid_holds_the_designed_inputs():
    for c in zr.CASES:
        X, var, ell = zr.make_inputs(c)
        e = GRID[c["name"]]
        assert np.array_equal(X, e["X"]) and np.array_equal(var, e["var"]) and np.array_equal(ell, e["ell"]), c["name"]
        assert abs(e["k0"] - zr.k_zero(var)) <= zr.EPS * e["k0"] and len(e["pivots"]) == c["M"] and e["trace"].shape == (c["M"] + 1,)
        assert len(set(e["pivots"].tolist())) == c["M"]
    for c in zr.FORCED_CASES:
        e = GRID[c["name"]]
        assert np.array_equal(e["pivots"], zr.forced_pivots(c)), c["name"]
        assert np.array_equal(e["rows"], zr.stored_rows(c, e["pivots"])) and np.all(np.isin(e["pivots"], e["rows"]))
        assert e["L"].shape == (len(e["rows"]), c["M"]) and sorted(e["d_after"]) == [m for m in zr.FORCED_MMAX if m <= c["M"]]
        assert np.min(e["dpiv"]) > 1e3 * zr.FLOOR * e["k0"]                                # far above the floor: no stop
    assert os.path.getsize(zr.GRID) < 512 * 1024


def test_grid_regenerates_on_a_subset():
    import make_zsel_grid as mk
    for n in zr.REGEN_CASES:
        out, e = mk.build_case(zr.CASE_BY_NAME[n]), GRID[n]
        for k in ("pivots", "dpiv", "trace"):
            assert np.array_equal(out[k], e[k]), (n, k)
        if "L" in e:
            assert np.array_equal(out["L"], e["L"]) and np.array_equal(out["rows"], e["rows"])
            assert np.array_equal(out["d_after"], np.stack([e["d_after"][m] for m in e["mmax"]]))


def test_restatement_against_the_grid():
    worst = dict.fromkeys(WHAT, 0.0)
    for c in zr.FORCED_CASES:
        e = GRID[c["name"]]
        for m in e["mmax"]:
            got = zr.prefix_ratios(e, zr.select(e["X"], e["var"], e["ell"], m, forced=e["pivots"][:m]), m)
            print("%-8s Mmax %2d " % (c["name"], m) + "  ".join("%s %.3f" % (k, got[k]) for k in WHAT))
            for k in WHAT:
                worst[k] = max(worst[k], got[k])
    for k in WHAT:
        assert worst[k] <= zr.c_oracle(k), (k, worst[k])
        assert worst[k] > zr.c_oracle(k) / 2.0, "C_ORACLE[%s] is not the measured figure rounded up to a power of two any more" % k
        assert zr.c_kernel(k) == 16.0                      # max(16, 4 C_ORACLE)
    assert zr.c_oracle("L") <= 8.0                         # beyond that the issue calls the scale wrong, not the constant


def test_designed_free_cases_have_no_near_ties(free_runs):
    """The top-two gap (d_(1) - d_(2)) / k0 >= 1e-9 at every pick j >= 1 and dpiv / k0 >= 1e-6: a few-eps error in d cannot change a pick,
    so the float64 restatement, the 50-digit run and the device must agree on the pivots exactly."""
    for c in zr.FREE_CASES:
        r, e = free_runs[c["name"]], GRID[c["name"]]
        gaps = zr.top_two_gaps(r["dhist"], r["k0"])
        print("%-5s min gap %.2e  min dpiv / k0 %.2e" % (c["name"], gaps.min(), r["dpiv"].min() / r["k0"]))
        assert r["Mout"] == c["M"] and len(gaps) == c["M"] - 1
        assert gaps.min() >= zr.GAP_MIN and r["dpiv"].min() / r["k0"] >= zr.DPIV_MIN
        assert np.array_equal(r["pivots"], e["pivots"]) and r["pivots"][0] == 0
        sd = zr.scale_d(r["k0"], e["dpiv"], e["G"])
        assert np.max(zr.ratios(r["dpiv"], e["dpiv"], sd[:-1])) <= zr.c_oracle("dpiv")
        assert np.max(zr.ratios(r["trace"], e["trace"], zr.scale_trace(r["k0"], e["dpiv"], e["trace"], c["N"], e["G"]))) <= zr.c_oracle("trace")


def test_a_moved_result_is_caught():
    """An entry off by 2 C S fails the device's criterion, whichever array it is in."""
    for n in ("f_N2", "f_N65", "f_N257"):
        e = GRID[n]
        m = e["mmax"][-1]
        r = zr.select(e["X"], e["var"], e["ell"], m, forced=e["pivots"][:m])
        assert all(v <= zr.c_kernel(k) for k, v in zr.prefix_ratios(e, r, m).items())
        sd, sL = zr.scale_d(e["k0"], e["dpiv"], e["G"]), zr.scale_L(e["k0"], e["dpiv"], e["G"])
        for what in WHAT:
            moved = {k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in r.items()}
            Ck = zr.c_kernel(what)
            if what == "L":
                i = e["rows"][len(e["rows"]) // 2]
                moved["L"][i, m - 1] = e["L"][len(e["rows"]) // 2, m - 1] + 2.0 * Ck * sL[m - 1]
            elif what == "d":
                moved["d"][e["rows"][-1]] = e["d_after"][m][-1] + 2.0 * Ck * sd[m]
            elif what == "dpiv":
                moved["dpiv"][m - 1] = e["dpiv"][m - 1] + 2.0 * Ck * sd[m - 1]
            else:
                moved["trace"][m] = e["trace"][m] + 2.0 * Ck * zr.scale_trace(e["k0"], e["dpiv"], e["trace"], e["case"]["N"], e["G"])[m]
            got = zr.prefix_ratios(e, moved, m)
            assert got[what] > Ck, (n, what, got[what])
            assert all(got[k] <= zr.c_kernel(k) for k in WHAT if k != what)
    bad = np.array(GRID["f_N2"]["dpiv"])
    bad[0] = np.nan
    assert np.isinf(np.max(zr.ratios(bad, GRID["f_N2"]["dpiv"], 1.0)))
    short = zr.select(GRID["f_N65"]["X"], GRID["f_N65"]["var"], GRID["f_N65"]["ell"], 7, forced=GRID["f_N65"]["pivots"][:7])
    assert np.isinf(zr.prefix_ratios(GRID["f_N65"], short, 8)["L"])           # a run that stopped early is no prefix


def test_free_and_forced_restatements_agree(free_runs):
    for c in zr.FREE_CASES:
        e, r = GRID[c["name"]], free_runs[c["name"]]
        f = zr.select(e["X"], e["var"], e["ell"], c["M"], forced=r["pivots"])
        for k in ("pivots", "Z", "dpiv", "trace", "L", "d"):
            assert np.array_equal(f[k], r[k]), (c["name"], k)
        half = zr.select(e["X"], e["var"], e["ell"], c["M"], forced=r["pivots"][:c["M"] // 2])      # forced first, then free
        assert np.array_equal(half["pivots"], r["pivots"]) and np.array_equal(half["L"], r["L"])


def test_factor_at_the_pivots_is_the_cholesky_factor_of_kzz(free_runs):
    """L[pivots] is lower triangular (to rounding: the entries above the diagonal are c of an earlier pivot) with diagonal sqrt(dpiv), and equals LAPACK's Cholesky factor of the restated K_ZZ in pick order: two
    float64 factorisations of one matrix, each with an error of the size of S_L -- LAPACK's is not pinned to 50 digits, so it gets the
    kernels' constant and this file's the oracle's."""
    for c in zr.FREE_CASES:
        e, r = GRID[c["name"]], free_runs[c["name"]]
        Lz = r["L"][r["pivots"]]
        sL = zr.scale_L(r["k0"], e["dpiv"], e["G"])
        assert np.max(np.abs(np.triu(Lz, 1)) / sL[None, :]) <= zr.c_oracle("L")          # above the diagonal: 0 in exact arithmetic
        Lz = np.tril(Lz)
        # the diagonal is sqrt(dpiv): L_pp within C_L S_L of its 50-digit value sqrt(R), dpiv within C_d S_d of R
        sd = zr.scale_d(r["k0"], e["dpiv"], e["G"])[:-1]
        assert np.all(np.abs(np.diag(Lz) - np.sqrt(r["dpiv"])) <= zr.c_oracle("L") * sL + zr.c_oracle("dpiv") * sd / np.sqrt(r["dpiv"]))
        ch = np.linalg.cholesky(zr.k_matrix(r["Z"], r["Z"], e["var"], e["ell"]))
        worst = float(np.max(zr.ratios(Lz, ch, sL[None, :])))
        print("%-5s L[pivots] against LAPACK: %.3f" % (c["name"], worst))
        assert worst <= zr.c_sum("L")
        assert np.array_equal(r["d"][r["pivots"]], np.zeros(c["M"]))


def test_trace_is_the_nystrom_residual(free_runs):
    for c in zr.FREE_CASES:
        e, r = GRID[c["name"]], free_runs[c["name"]]
        assert np.all(np.diff(r["trace"]) <= 0.0) and abs(r["trace"][0] - c["N"] * r["k0"]) <= zr.EPS * zr.addition_path(c["N"]) * c["N"] * r["k0"]
        S = zr.scale_trace(r["k0"], e["dpiv"], e["trace"], c["N"], e["G"])
        for j in (1, c["M"] // 2, c["M"]):
            want = c["N"] * r["k0"] - np.sum(r["L"][:, :j] ** 2)
            assert abs(r["trace"][j] - want) <= zr.c_sum("trace") * S[j] + zr.EPS * c["N"] * r["k0"], (c["name"], j)
        nys = zr.nystrom_trace(e["X"], r["Z"], e["var"], e["ell"])
        assert abs(r["trace"][-1] - nys) <= 1e-9 * c["N"] * r["k0"], (c["name"], r["trace"][-1], nys)


def test_full_rank_run_reproduces_k():
    """Mmax = N = 65: L L^T = K to rounding -- Higham's bound for a Cholesky factor, |L L^T - K| <= (n + 1) 2^-53 |L| |L^T| with
    (|L| |L^T|)_ii' <= k0, beside the kernel entries' own G ulps: 2^-52 (N + 2 + G) k0 per entry."""
    X = np.random.RandomState(305).rand(65, 3)
    var, c = zr.KERNELS[3]
    ell = c * 0.12
    r = zr.select(X, var, ell, 65)
    assert r["Mout"] == 65 and sorted(r["pivots"].tolist()) == list(range(65)) and np.all(r["d"] == 0.0)
    K = zr.k_matrix(X, X, var, ell)
    err = float(np.max(np.abs(r["L"] @ r["L"].T - K)) / (zr.EPS * (65 + 2 + zr.gpy_order_cost(X, var, ell)) * r["k0"]))
    print("full rank: |L L^T - K| = %.3f of the bound; d / k0 down to %.2e" % (err, r["dpiv"].min() / r["k0"]))
    assert err <= 1.0 and abs(r["trace"][-1]) == 0.0


def test_stop_rules_in_the_restatement():
    """The tol case stops where dpiv is not within 1e-9 k0 of tol k0 (the GPU test relies on it); Mmax > N stops with Mout <= N; a forced
    pick below the floor stops; exact duplicates of a picked row are never picked."""
    X, var, ell = zr.make_inputs(zr.TOL_CASE)
    full, r = zr.select(X, var, ell, zr.TOL_CASE["M"]), zr.select(X, var, ell, zr.TOL_CASE["M"], tol=zr.TOL)
    m = r["Mout"]
    assert 2 < m < zr.TOL_CASE["M"] == full["Mout"] and np.array_equal(r["pivots"], full["pivots"][:m])
    assert full["dpiv"][m] <= zr.TOL * r["k0"] < full["dpiv"][m - 1]
    assert min(abs(full["dpiv"][j] / r["k0"] - zr.TOL) for j in (m - 1, m)) > 1e3 * zr.TOL_MARGIN
    assert np.all(r["L"][:, m:] == 0.0) and r["trace"].shape == (m + 1,)
    X, var, ell = zr.small_case()
    r = zr.select(X, var, ell, 40)
    assert r["Mout"] <= X.shape[0]
    X, var, ell = zr.duplicates_case()
    r = zr.select(X, var, ell, 100)
    assert r["Mout"] <= 80 and len(set(r["pivots"].tolist()) & {p + 40 for p in r["pivots"].tolist() if p < 40}) == 0
    assert zr.a_posteriori(X, var, ell, r["pivots"], zr.c_oracle("d")) == []
    f = zr.select(X, var, ell, 5, forced=[3, 43])              # row 43 repeats row 3: its d is rounding noise after the first pick
    assert f["Mout"] == 1 and np.all(f["L"][:, 1:] == 0.0)
    X, var, ell = zr.lattice_case()
    r = zr.select(X, var, ell, 40)
    assert zr.a_posteriori(X, var, ell, r["pivots"], zr.c_oracle("d")) == []
    wrong = r["pivots"].copy()
    wrong[1] = 1                                               # not the row of largest d at pick 1
    assert zr.a_posteriori(X, var, ell, wrong[:2], zr.c_sum("d")) != []


def test_facade_margin_on_the_cpu():
    """The greedy choice's tr(K_ff - Q_ff) is at least 2x below a seeded random subset's of the same size (the GPU facade test asserts the
    device's trace is below the random subset's)."""
    X_list, var, ell = zr.facade_case()
    X = np.vstack(X_list)
    r = zr.select(X, var, ell, 16)
    sub = np.random.RandomState(zr.FACADE_SUBSET_SEED).choice(X.shape[0], 16, replace=False)
    rnd = zr.nystrom_trace(X, X[sub], var, ell)
    print("greedy %.4f  random subset %.4f" % (r["trace"][-1], rnd))
    assert r["Mout"] == 16 and 2.0 * r["trace"][-1] <= rnd


# ------------------------------------------------------------------------------------------------------------ the C ABI and the facade
def test_abi_symbol_and_host_side_refusals():
    """The symbol exists, the ABI version stays 8, every host-side refusal is HMOGP_E_INVALID with a message that names the argument -- with or
    without a device, so before it is touched -- and the valid call gets past them: HMOGP_E_NO_DEVICE on a machine without a GPU."""
    import torch
    from hetmogp_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.lib.hmogp_abi_version() == 8
    assert "hmogp_select_inducing" in _lib.EXPORTS and hasattr(_lib.lib, "hmogp_select_inducing")
    header = open(os.path.join(ROOT, "include", "hetmogp_hip.h")).read()
    assert "hmogp_select_inducing(" in header and "#define HMOGP_ABI_VERSION 8" in header
    assert "#define HMOGP_ZSEL_FLOOR 9.094947017729282e-13" in header and 9.094947017729282e-13 == 2.0 ** -40 == _lib.ZSEL_FLOOR
    for kw, word in zr.REFUSALS:
        rc, msg = zr.abi_call(**kw)
        assert rc == _lib.E_INVALID, (kw, rc, msg)
        assert msg.startswith("hmogp_select_inducing: ") and word in msg, (kw, msg)
    rc, msg = zr.abi_call(n_forced=0, forced=None, L=None, d=None)          # forced with n_forced = 0, L and d may be NULL
    if torch.cuda.is_available():
        assert rc == 0, msg
    else:
        assert rc == _lib.E_NO_DEVICE, (rc, msg)
    # in the source the refusals are one function that the C ABI calls before it selects the device, and the memory question precedes the first allocation
    csrc = os.path.join(ROOT, "hetmogp_amd", "csrc")
    abi = open(os.path.join(csrc, "abi.hip")).read()
    body = abi[abi.index("int hmogp_select_inducing("):]
    assert 0 < body.index("select_inducing_check(") < body.index("need_device(device)") < body.index("select_inducing_run(") < body.index("\n}\n")
    src = open(os.path.join(csrc, "zsel.hip")).read()
    check = src[src.index("void select_inducing_check("):src.index("void select_inducing_run(")]
    for m in ("N must", "P must", "Q must", "Mmax must", "X has a non-finite", "variance must", "lengthscale must", "tol must", "n_forced must",
              "forced index out of range", "forced index repeated", "X is NULL", "Mout is NULL"):
        assert 'refuse("%s' % m in check, m
    assert "hip" not in check                                  # no runtime call among the refusals
    run = src[src.index("void select_inducing_run("):]
    assert "refuse(" in run and 0 < run.index("hipMemGetInfo") < run.index(".ensure(")


def test_select_inducing_argument_checks():
    import hetmogp_amd as hm
    from hetmogp_amd import _lib
    from hetmogp_amd.kern import RBF
    X = np.random.RandomState(2).rand(20, 2)
    k = [RBF(2, 1.0, 0.3), RBF(2, 0.5, 0.2)]
    with pytest.raises(_lib.InvalidArgument, match="keep must have shape"):
        hm.select_inducing(X, 4, k, keep=np.zeros((2, 3)))
    with pytest.raises(_lib.InvalidArgument, match="keep must have shape"):
        hm.select_inducing(X, 4, k, keep=np.zeros(2))
    with pytest.raises(_lib.InvalidArgument, match="more than M"):
        hm.select_inducing(X, 4, k, keep=np.zeros((5, 2)))
    with pytest.raises(_lib.InvalidArgument, match="same number of columns"):
        hm.select_inducing([X, np.zeros((3, 1))], 4, k)
    with pytest.raises(_lib.InvalidArgument, match="Mmax"):
        hm.select_inducing(X, 0, k)
    with pytest.raises(_lib.InvalidArgument, match="tol"):
        hm.select_inducing(X, 4, k[0], tol=-1.0)
    with pytest.raises(_lib.InvalidArgument, match="X has a non-finite"):
        hm.select_inducing([X, np.array([[np.nan, 0.0]])], 4, k)
