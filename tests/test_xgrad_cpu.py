"""Gradients of q(f) with respect to the new inputs, CPU side: the float64 restatement (tests/xgrad_ref.py) against the 50-digit
grid tests/golden/xgradgrid.npz, the grid's regeneration, the formula itself against central differences at 50 digits, the criterion's
sensitivity, the scale, the properties of the restated gradients, the two new C-ABI symbols with every host-side refusal, and the designed
sensitivity case.  The device is held to the same grid in tests/test_xgrad_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import joint_ref as jr            # noqa: E402
import xgrad_ref as xr            # noqa: E402

GRID = xr.load_grid()
NAMES = [c["name"] for c in xr.CASES]


@pytest.fixture(scope="module")
def restated():
    """(inputs, dm, dv, S_dm, S_dv, F_dm, F_dv) of every case, computed once."""
    out = {}
    for c in xr.CASES:
        inp = xr.make_inputs(c)
        out[c["name"]] = (inp,) + xr.input_grad(inp, return_scale=True)
    return out


def test_cases_cover_the_issue():
    assert {c["N"] for c in xr.CASES} == {1, 63, 64, 65, 257}
    assert {c["M"] for c in xr.CASES} >= {1, 2, 63, 64, 65, 127, 128, 129, 200}
    assert {c["P"] for c in xr.CASES} == {1, 2, 3, 4} and {c["Q"] for c in xr.CASES} == {1, 3} and {c["Df"] for c in xr.CASES} == {1, 4}
    assert {c["exact"] for c in xr.CASES} == {True, False}
    ells = [l for c in xr.CASES for l in c["ell"]]
    assert min(ells) == 0.05 and max(ells) == 0.9 and any(c["shift"] == 10.0 for c in xr.CASES)
    for c in xr.CASES:
        inp = xr.make_inputs(c)
        C = inp["C"]
        assert np.array_equal(C, np.transpose(C, (0, 2, 1)))
        if c["M"] > 1:
            ev = np.linalg.eigvalsh(C[0])
            assert ev[0] < 0.0 < ev[-1]                      # indefinite
        if c["Q"] * c["Df"] > 1:
            assert np.sum(inp["W"] == 0.0) == 1              # dense otherwise: the functions share the latents
        on, far = xr.special_rows(c)
        P = c["P"]
        for i in on:                                         # exactly on an inducing input
            assert any(np.any(np.all(inp["Z"][:, q * P:(q + 1) * P] == inp["X"][i], 1)) for q in range(c["Q"]))
        if far is not None:                                  # every k underflows: at least FAR lengthscales from every z, every latent
            for q in range(c["Q"]):
                d = np.sqrt(np.sum((inp["Z"][:, q * P:(q + 1) * P] - inp["X"][far]) ** 2, 1))
                assert np.min(d) >= xr.FAR * c["ell"][q]
    assert sum(len(xr.special_rows(c)[0]) == 3 for c in xr.CASES) >= 8


def test_grid_holds_the_designed_rows():
    for c in xr.CASES:
        e = GRID[c["name"]]
        rows = xr.stored_rows(c)
        assert np.array_equal(rows, e["rows"]) and len(rows) == min(xr.MAX_ROWS, c["N"])
        on, far = xr.special_rows(c)
        for i in [0, c["N"] - 1] + [i for i in (62, 63, 64, 65) if i < c["N"]] + on + ([far] if far is not None else []):
            assert i in rows
        for k in ("dm", "dv", "S_dm", "S_dv", "F_dm", "F_dv"):
            assert e[k].shape == (len(rows), c["Df"], c["P"]) and np.all(np.isfinite(e[k]))
        assert np.all(e["S_dm"] >= 0) and np.all(e["F_dm"] >= 0) and np.all(e["F_dv"] >= 0)
        if far is not None:                                  # the far row: the 50-digit value is below the smallest subnormal
            k = int(np.searchsorted(rows, far))
            assert np.all(e["dm"][k] == 0.0) and np.all(e["dv"][k] == 0.0)
    assert os.path.getsize(xr.GRID) < 300 * 1000


def test_restatement_against_the_grid(restated):
    worst = {"dm": 0.0, "dv": 0.0}
    for n in NAMES:
        _, dm, dv = restated[n][:3]
        rm, rv = xr.case_ratios(GRID[n], dm, dv)
        print("%-14s dm %.3f dv %.3f" % (n, rm, rv))
        worst["dm"], worst["dv"] = max(worst["dm"], rm), max(worst["dv"], rv)
    for what in ("dm", "dv"):
        assert worst[what] <= xr.c_oracle(what), (what, worst[what])
    assert xr.c_kernel("dm") == 16.0 and xr.c_kernel("dv") == 16.0
    assert max(xr.C_ORACLE.values()) <= 8.0 and max(xr.C_ORACLE_STRICT.values()) <= 8.0      # (above 8 the SCALE would be wrong)


def test_grid_regenerates_on_a_subset():
    import xgrad_ref_mp as xm
    rng = np.random.RandomState(3)
    for n in xr.REGEN_CASES:
        e = GRID[n]
        pick = np.sort(rng.choice(len(e["rows"]), min(3, len(e["rows"])), replace=False))
        ref = xm.reference(xr.make_inputs(xr.CASE_BY_NAME[n]), e["rows"][pick])
        for k in ("dm", "dv", "S_dm", "S_dv", "F_dm", "F_dv"):
            assert np.array_equal(ref[k], e[k][pick]), (n, k)


def test_chain_restatements_against_the_grid():
    """The whole chain from (Z, m_u, L_flat, hypers) at M = 16, explicit-C and solve-based, against its 50-digit reference: scale S x
    cond_est, the constant recorded as C_ORACLE_STRICT; one row of the stored reference regenerates bit for bit."""
    import make_xgrad_grid as mg
    import xgrad_ref_mp as xm
    for name in mg.CHAIN_CASES:
        prm, Xnew = jr.make_params(jr.CASE_BY_NAME[name])
        e = mg.load_chain(name)
        assert np.array_equal(e["rows"], mg.chain_rows(name))
        cond = max(jr.cond_estimates(prm, Xnew.shape[1]))
        for strict in (False, True):
            dm, dv = xr.chain(prm, Xnew, strict=strict)
            rm = np.max(xr.ratios(dm[e["rows"]], e["dm"], cond * e["S_dm"], e["F_dm"]))
            rv = np.max(xr.ratios(dv[e["rows"]], e["dv"], cond * e["S_dv"], e["F_dv"]))
            print("%s strict=%s: dm %.3f dv %.3f" % (name, strict, rm, rv))
            assert rm <= xr.c_oracle("dm", True) and rv <= xr.c_oracle("dv", True)
    prm, Xnew = jr.make_params(jr.CASE_BY_NAME["s_N63"])
    e = mg.load_chain("s_N63")
    ref = xm.chain_reference(prm, Xnew, e["rows"][5:6])
    for k in ("dm", "dv", "S_dm", "S_dv"):
        assert np.array_equal(ref[k], e[k][5:6]), k


def test_the_formula_against_central_differences_at_50_digits():
    """dm and dv are the derivatives of m and v: central differences of the 50-digit m and v with h = 1e-22 relative (truncation ~ h^2,
    rounding ~ 1e-50 / h) agree with the 50-digit dm and dv to 1e-18 of the scale."""
    import mpmath as mp
    import xgrad_ref_mp as xm
    for n, rows in (("M2_N63", (0, 2, 40)), ("M16_N65_shift", (1, 32)), ("M63_N64", (7,))):
        c = xr.CASE_BY_NAME[n]
        inp = xr.make_inputs(c)
        I = xm.prepare(inp)
        for i in rows:
            x = xm._vec(inp["X"][i])
            dm, dv, sm, sv, _, _ = xm.grad(I, x, scale=True)
            for j in range(c["P"]):
                h = mp.mpf(10) ** -22 * max(1, abs(x[j]))
                xp, xn = list(x), list(x)
                xp[j], xn[j] = x[j] + h, x[j] - h
                (mp_, vp_), (mn_, vn_) = xm.mean_var(I, xp), xm.mean_var(I, xn)
                for d in range(c["Df"]):
                    fm, fv = (mp_[d] - mn_[d]) / (2 * h), (vp_[d] - vn_[d]) / (2 * h)
                    assert abs(fm - dm[d][j]) <= mp.mpf(10) ** -18 * sm[d][j], (n, i, d, j)
                    assert abs(fv - dv[d][j]) <= mp.mpf(10) ** -18 * sv[d][j], (n, i, d, j)


def test_a_moved_result_is_caught(restated):
    """An entry off by 2 C (2^-52 S + 2^-1022 F) fails the device's criterion, whichever entry it is."""
    for n in ("M1_N1", "M65_N257", "M128_N257", "M16_N65_shift"):
        e = GRID[n]
        _, dm, dv = restated[n][:3]
        for what, C_ in (("dm", xr.c_kernel("dm")), ("dv", xr.c_kernel("dv"))):
            rm0, rv0 = xr.case_ratios(e, dm, dv)
            assert (rm0 if what == "dm" else rv0) <= C_
            for k in range(len(e["rows"])):
                moved = np.array(dm if what == "dm" else dv)
                idx = (e["rows"][k], e[what].shape[1] - 1, 0)
                moved[idx] = e[what][k, -1, 0] + 2.0 * C_ * (xr.EPS * e["S_" + what][k, -1, 0] + xr.TINY * e["F_" + what][k, -1, 0])
                r = xr.case_ratios(e, moved, dv)[0] if what == "dm" else xr.case_ratios(e, dm, moved)[1]
                assert r > C_, (n, what, k)
    bad = np.array(restated["M1_N1"][1])
    bad[0, 0, 0] = np.nan
    assert np.isinf(xr.case_ratios(GRID["M1_N1"], bad, restated["M1_N1"][2])[0])


def test_float64_scale_equals_the_50_digit_scale(restated):
    for n in NAMES:
        e = GRID[n]
        _, _, _, sm, sv, fm, fv = restated[n]
        for got, key in ((sm, "S_dm"), (sv, "S_dv"), (fm, "F_dm"), (fv, "F_dv")):
            want = e[key]
            assert np.all(np.abs(got[e["rows"]] - want) <= 1e-9 * want), (n, key)


def test_dv_vanishes_with_C_and_dm_is_linear(restated):
    rng = np.random.RandomState(8)
    for n in ("M2_N63", "M65_N257", "M129_N64"):
        inp = restated[n][0]
        zero = dict(inp, C=np.zeros_like(inp["C"]))
        dm0, dv0 = xr.input_grad(zero)
        assert np.all(dv0 == 0.0) and np.array_equal(dm0, restated[n][1])           # dm does not read C
        a2, W2 = rng.randn(*inp["a"].shape), rng.randn(*inp["W"].shape)
        _, _, sm = xr.input_grad(inp, return_scale=True)[:3]
        # linear in a: dm(a + 2 a2) = dm(a) + 2 dm(a2); in W: dm(W + 2 W2) = dm(W) + 2 dm(W2) -- each to a few ulps of the scales involved
        for key, other in (("a", a2), ("W", W2)):
            lhs, _, sl = xr.input_grad(dict(inp, **{key: inp[key] + 2.0 * other}), return_scale=True)[:3]
            rhs2, _, s2 = xr.input_grad(dict(inp, **{key: other}), return_scale=True)[:3]
            tol = 8.0 * xr.EPS * (sl + sm + 2.0 * s2)
            assert np.all(np.abs(lhs - (restated[n][1] + 2.0 * rhs2)) <= tol), (n, key)


def test_far_rows_and_rows_on_inducing_inputs(restated):
    for n in NAMES:
        c = xr.CASE_BY_NAME[n]
        on, far = xr.special_rows(c)
        _, dm, dv = restated[n][:3]
        if far is not None:
            assert np.all(dm[far] == 0.0) and np.all(dv[far] == 0.0)
        assert np.all(np.isfinite(dm)) and np.all(np.isfinite(dv))
        for i in on:
            assert np.any(dm[i] != 0.0)


def _ptr(a):
    from hetmogp_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib.c_double_p)


def _call(device=0, N=2, P=1, M=3, Q=1, Df=2, null=(), var=1.0, ell=0.5):
    from hetmogp_amd import _lib
    arr = dict(X=np.zeros((max(N, 1), max(P, 1))), Z=np.zeros((max(M, 1), max(Q, 1) * max(P, 1))), variance=np.full(max(Q, 1), var),
               lengthscale=np.full(max(Q, 1), ell), a=np.zeros((max(Q, 1), max(M, 1))), C=np.zeros((max(Q, 1), max(M, 1), max(M, 1))),
               W=np.ones((max(Q, 1), max(Df, 1))), dm=np.zeros((max(N, 1), max(Df, 1), max(P, 1))), dv=np.zeros((max(N, 1), max(Df, 1), max(P, 1))))
    p = {k: (None if k in null else _ptr(v)) for k, v in arr.items()}
    rc = _lib.lib.hmogp_qf_input_grad(device, N, P, p["X"], M, Q, p["Z"], p["variance"], p["lengthscale"], 1, p["a"], p["C"], Df, p["W"],
                                      p["dm"], p["dv"])
    msg = _lib.lib.hmogp_last_error(None)
    return rc, (msg.decode() if msg else "")


NO_SUCH_DEVICE = 1 << 20           # an ordinal no machine has: the answer is the same with and without a GPU


def test_abi_symbols():
    from hetmogp_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.lib.hmogp_abi_version() == 8
    assert "hmogp_qf_input_grad" in _lib.EXPORTS and "hmogp_predict_f_grad" in _lib.EXPORTS
    assert hasattr(_lib.lib, "hmogp_qf_input_grad") and hasattr(_lib.lib, "hmogp_predict_f_grad")
    header = open(os.path.join(ROOT, "include", "hetmogp_hip.h")).read()
    assert "int hmogp_qf_input_grad(" in header and "int hmogp_predict_f_grad(" in header and "#define HMOGP_ABI_VERSION 8" in header


@pytest.mark.parametrize("kw,word", [
    (dict(N=-1), "N"), (dict(P=0), "P"), (dict(P=5), "P"), (dict(M=0), "M"), (dict(Q=0), "Q"), (dict(Q=9), "Q"), (dict(Df=0), "Df"),
    (dict(null=("X",)), "X"), (dict(null=("Z",)), "Z"), (dict(null=("variance",)), "variance"), (dict(null=("lengthscale",)), "lengthscale"),
    (dict(null=("a",)), "a is"), (dict(null=("C",)), "C is"), (dict(null=("W",)), "W"), (dict(null=("dm",)), "dm"), (dict(null=("dv",)), "dv"),
    (dict(var=0.0), "variance"), (dict(var=-1.0), "variance"), (dict(var=np.nan), "variance"), (dict(var=np.inf), "variance"),
    (dict(ell=0.0), "lengthscale"), (dict(ell=np.nan), "lengthscale"), (dict(ell=np.inf), "lengthscale"), (dict(ell=-0.5), "lengthscale"),
], ids=lambda a: "" if isinstance(a, str) else "-".join("%s=%s" % kv for kv in a.items()))
def test_host_side_refusals_come_before_the_device(kw, word):
    """HMOGP_E_INVALID with a message naming the argument -- asked of a device ordinal that does not exist, so the refusal provably sits in
    front of the first device call."""
    from hetmogp_amd import _lib
    rc, msg = _call(device=NO_SUCH_DEVICE, **kw)
    assert rc == _lib.E_INVALID and msg.startswith("hmogp_qf_input_grad: ") and word in msg, (rc, msg)


def test_no_device_and_empty_calls():
    from hetmogp_amd import _lib, engine
    rc, msg = _call(device=NO_SUCH_DEVICE)
    assert rc == _lib.E_NO_DEVICE, (rc, msg)
    assert _call(device=NO_SUCH_DEVICE, N=0)[0] == 0                                   # N = 0 returns success at once ...
    assert _call(device=NO_SUCH_DEVICE, N=0, null=("X", "Z", "a", "C", "W", "dm", "dv"))[0] == 0      # ... whatever the pointers
    assert _call(device=NO_SUCH_DEVICE, N=0, P=7)[0] == _lib.E_INVALID                 # but not whatever the shapes
    with pytest.raises(_lib.HetMOGPError) as ei:
        engine.qf_input_grad_rows(np.zeros((2, 1)), np.zeros((3, 1)), [1.0], [1.0], np.zeros((1, 3)), np.zeros((1, 3, 3)), np.ones((1, 2)),
                                  device=NO_SUCH_DEVICE)
    assert ei.value.code == _lib.E_NO_DEVICE
    with pytest.raises(_lib.InvalidArgument):
        engine.qf_input_grad_rows(np.zeros((2, 1)), np.zeros((3, 2)), [1.0], [1.0], np.zeros((1, 3)), np.zeros((1, 3, 3)), np.ones((1, 2)))
    dm, dv = engine.qf_input_grad_rows(np.zeros((0, 2)), np.zeros((3, 2)), [1.0], [1.0], np.zeros((1, 3)), np.zeros((1, 3, 3)), np.ones((1, 2)),
                                       device=NO_SUCH_DEVICE)
    assert dm.shape == (0, 2, 2) and dv.shape == (0, 2, 2)
    # the engine path: a NULL handle is refused on the host
    X, out = np.zeros((2, 1)), np.zeros((2, 1, 1))
    assert _lib.lib.hmogp_predict_f_grad(None, _ptr(X), 2, None, None, _ptr(out), _ptr(out)) == _lib.E_INVALID
    assert b"handle" in _lib.lib.hmogp_last_error(None)


def test_designed_sensitivity_case():
    """2-D inputs, q(u)'s mean a function of column 0 only, small S: the restated root-mean-square gradient of column 0 is at least ten
    times that of column 1, for every function."""
    prm, X = xr.sensitivity_case()
    assert max(jr.cond_estimates(prm, 2)) < jr.COND_FLAG
    dm, dv = xr.chain(prm, X)
    s = xr.sensitivity(dm)
    print("sensitivity (Df, P):\n%s" % s)
    assert s.shape == (jr.DF, 2) and np.all(s[:, 0] >= 10.0 * s[:, 1]) and np.all(s[:, 0] > 0.1)
