"""Gradients of posterior sample paths with respect to new inputs, CPU side: the float64 restatement (tests/pathsgrad_ref.py)
against the 50-digit grid tests/golden/pathsgradgrid.npz and the two P = 3 cases beyond it, the 50-digit formula against the numerical derivative of the
50-digit path, the grid's regeneration, the mean identity against the gradients of q(f), the exact zero at a coincident input,
the finite-difference figures the device test takes its tolerance from, the statistical case on the restatement's own gradients and the new
C-ABI symbol.  The device is held to the same references in tests/test_pathsgrad_gpu.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import paths_ref as pr            # noqa: E402
import pathsgrad_ref as gr        # noqa: E402
import xgrad_ref as xr            # noqa: E402

GRID = gr.load_grid()
NAMES = [c["name"] for c in gr.CASES]


def test_cases_cover_the_designed_shapes():
    C = gr.CASES
    assert len(GRID) == len(C) == 10
    assert {c["S"] for c in C} == {1, 3} and {c["Lf"] for c in C} == {1, 8, 50, 64} and {c["M"] for c in C} == {16, 128}
    assert {c["P"] for c in C} == {1, 2, 4} and {1, 63, 65, 129} <= {c["N"] for c in C}
    for c, c9v in zip(C, pr.CASES):                                                  # the model set-up of DESIGN 9r / 9v: same seeds
        assert all(c[k] == c9v[k] for k in ("name", "M", "Q", "P", "N", "functions", "seed", "Lf"))
    o = gr.ODD_CASE                                                                  # what the ten cases do not reach: M odd, P = 3
    assert o["M"] % 2 == 1 and o["P"] == 3 and o["N"] > 64
    o = gr.EVEN_P3_CASE                                                              # ... and P = 3 on the 16-byte branch
    assert o["M"] % 2 == 0 and o["P"] == 3 and o["N"] > 64
    for n in NAMES:
        c = GRID[n]["case"]
        size = c["S"] * len(c["functions"]) * c["N"] * c["P"]
        assert len(GRID[n]["G"]) == (size if size <= gr.FULL_MAX else gr.N_SUBSET)
    assert os.path.getsize(gr.GRID) < 400 * 1024


def test_restatement_against_the_grid():
    import make_pathsgrad_grid as mk
    worst = 0.0
    for n in NAMES:
        e, c = GRID[n], GRID[n]["case"]
        G, sG = gr.evaluate_grad(gr.synthetic_state(c, e["prm"]), e["prm"], c["P"], e["Xnew"], return_scale=True)
        r = gr.grad_ratios(e, G)
        assert np.allclose(gr.pick(sG, e["i_G"]), e["G_scale"], rtol=1e-9, atol=0.0), n       # the scale in both arithmetics
        print("%-7s G %.3f" % (n, r))
        worst = max(worst, r)
    for c in gr.EXTRA_CASES:
        r = mk.extra_case_ratio(c)
        print("%-7s G %.3f" % (c["name"], r))
        worst = max(worst, r)
    assert worst <= gr.c_oracle(), worst
    assert worst > gr.c_oracle() / 64.0, "C_ORACLE is not the measured figure any more"


@pytest.mark.parametrize("name", gr.REGEN_CASES)
def test_formula_against_the_numerical_derivative_of_the_50_digit_path(name):
    """The 50-digit formula against mp.diff of the 50-digit PATH (paths_ref_mp's pieces): relative 1e-30 of the entry's scale."""
    import pathsgrad_ref_mp as gm
    e, c = GRID[name], GRID[name]["case"]
    st = gr.synthetic_state(c, e["prm"])
    idx = e["i_G"][::max(1, len(e["i_G"]) // 12)][:12]
    R, sc = gm.evaluate_grad_mp(st, e["prm"], c["P"], e["Xnew"], idx)
    nd = gm.numeric_grad(st, e["prm"], c["P"], e["Xnew"], idx)
    worst = max(float(abs(a - b) / s) for a, b, s in zip(nd, R, sc))
    print("%s: worst |formula - numerical| / scale %.3e on %d entries" % (name, worst, len(idx)))
    assert worst <= 1e-30


def test_grid_regenerates_bit_for_bit():
    import make_pathsgrad_grid as mk
    for n in gr.REGEN_CASES:
        ref = mk.build_case(GRID[n]["case"])
        for k, v in ref.items():
            assert np.array_equal(v, GRID[n][k]), (n, k)


def test_a_moved_result_is_caught():
    for n in ("s_N1", "s_N64", "r_N65"):
        e = GRID[n]
        j = len(e["G"]) // 2
        moved = e["G"].copy()
        assert np.max(gr.ratios(moved, e["G"], e["G_scale"])) == 0.0
        moved[j] += 2.0 * gr.c_kernel() * gr.EPS * e["G_scale"][j]
        assert np.max(gr.ratios(moved, e["G"], e["G_scale"])) > gr.c_kernel()
        moved[0] = np.nan
        assert np.isinf(np.max(gr.ratios(moved, e["G"], e["G_scale"])))


@pytest.mark.parametrize("name", ["s_N63", "s_N65", "r_N64"])
def test_mean_identity(name):
    """With theta~ = 0 and v~ = w K^-1 m the path is the posterior mean: the restatement's gradient equals xgrad_ref's dm, each within its own
    constant of the exact value in its own scale.  (K^-1 m is xgrad_ref's own vector: the identity is about the gradient, not the solve.)"""
    e, c = GRID[name], GRID[name]["case"]
    d = list(c["functions"])
    inp, _ = xr.chain_inputs(e["prm"], e["Xnew"])
    st = gr.mean_state(e["prm"], c["P"], d, alpha=inp["a"])
    G, sG = gr.evaluate_grad(st, e["prm"], c["P"], e["Xnew"], return_scale=True)
    dm, _, sm, _, fm, _ = xr.chain(e["prm"], e["Xnew"], return_scale=True)
    got = np.transpose(G[0], (1, 0, 2))                                              # (N, nD, P)
    bound = gr.EPS * (gr.c_oracle() * np.transpose(sG[0], (1, 0, 2)) + xr.c_oracle("dm") * sm[:, d]) + 2.0 ** -1022 * fm[:, d]
    worst = float(np.max(np.abs(got - dm[:, d]) / bound))
    print("%s: worst |G - dm| / bound %.3f" % (name, worst))
    assert worst <= 1.0 and np.max(np.abs(dm[:, d])) > 0.0


def test_coincident_input_gives_an_exact_zero():
    """A row whose x equals an inducing input bit for bit has D(p) = 0 exactly at that m (and nowhere else): one subtraction per term."""
    for name in ("s_N64", "r_N65"):
        c = gr.CASE_BY_NAME[name]
        prm, Xnew = gr.make_params(c)
        for q in range(c["Q"]):
            lt = pr.latent_q(prm, q, c["P"])
            X = Xnew[:5].copy()
            X[2] = lt["Zq"][7]
            A = lt["var"] * np.exp(-0.5 * gr.jr.r2_gpy(X, lt["Zq"], lt["ell"]))
            for p in range(c["P"]):
                D = gr.derivative_image(A, lt["Zq"], X, lt["ell"], p)
                assert D[2, 7] == 0.0 and A[2, 7] > 0.0
                assert D[2, 6] != 0.0 and D[2, 8] != 0.0


@pytest.mark.parametrize("name", gr.FD_CASES)
def test_finite_difference_figures(name):
    """The error of the float64 restatement's central differences (h = 2^-10 l_min) against the 50-digit gradient is the recorded figure: the
    device test allows FD_FACTOR times FD_MEASURED."""
    import make_pathsgrad_grid as mk
    err = mk.fd_error(name)
    print("%s: %.3e of max |G| (recorded %.3e)" % (name, err, gr.FD_MEASURED[name]))
    assert gr.FD_MEASURED[name] / 2.0 < err <= gr.FD_MEASURED[name]


def test_statistical_thresholds_hold_for_the_restatement():
    """The statistical case of the GPU suite on the restatement's own gradients (same seed): given the frequencies theta, theta' and eps have
    mean 0, so the mean of G over the samples is d m_d / d x; the per-entry standard deviation is the paths' own linear map's."""
    prm, Xnew, d = gr.stat_case()
    P = Xnew.shape[1]
    st = pr.state(prm, P, d, gr.STAT_DRAWS, gr.STAT_FEATURES, gr.STAT_SEED)
    G = gr.evaluate_grad(st, prm, P, Xnew).reshape(gr.STAT_DRAWS, -1)
    dm = np.transpose(xr.chain(prm, Xnew)[0][:, list(d)], (1, 0, 2)).reshape(-1)
    B = gr.grad_linear_map(st["omega"], prm, P, d, Xnew)
    sd = np.sqrt((B * B).sum(1))
    z, count = gr.stat_mean_z(G, dm, sd)
    t = pr.z_threshold(count)
    print("worst |z| %.2f over %d statistics, threshold %.2f" % (z, count, t))
    assert count == 32 and z <= t
    # the standard deviation is the gradients' own: the sample variance agrees with it (a loose guard that sd is not inflated)
    assert np.all(np.abs(G.std(0) / sd - 1.0) < 0.1)
    # ... and a planted error of 0.2 sigma_d / l in the mean gradient is rejected
    sig = np.sqrt(((prm["W"][:, list(d)] ** 2 + prm["kappa"][:, list(d)]) * prm["variance"][:, None]).sum(0))        # prior sd of f_d
    plant = np.repeat(0.2 * sig / np.max(prm["lengthscale"]), Xnew.shape[0] * P)
    assert gr.stat_mean_z(G, dm + plant, sd)[0] > t


def test_abi_symbol_and_refusals_without_a_device():
    """The symbol exists in the built library, the ABI version stays 8, a NULL handle is refused on the host with a message.  (The refusals
    that need an engine: tests/test_pathsgrad_gpu.py::test_refusals.)"""
    import ctypes as C
    from hetmogp_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.lib.hmogp_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "hetmogp_hip.h")).read()
    assert "hmogp_paths_eval_grad" in _lib.EXPORTS and "hmogp_paths_eval_grad(" in header and "#define HMOGP_ABI_VERSION 8" in header
    assert hasattr(_lib.lib, "hmogp_paths_eval_grad")
    buf = np.zeros(4)
    bp = buf.ctypes.data_as(_lib.c_double_p)
    assert _lib.lib.hmogp_paths_eval_grad(None, 0, bp, 1, None, bp) == _lib.E_INVALID
    assert b"handle is NULL" in _lib.lib.hmogp_last_error(None) and b"hmogp_paths_eval_grad" in _lib.lib.hmogp_last_error(None)
    assert _lib.lib.hmogp_paths_eval_grad(None, 0, None, 0, None, None) == _lib.E_INVALID
    assert np.all(buf == 0.0)
    # a thin guard, as in tests/test_paths_cpu.py: the state check comes before the device is named, the memory question before the allocations
    src = open(os.path.join(ROOT, "hetmogp_amd", "csrc", "engine_optim.hip")).read()
    body = src[src.index("void hmogp_engine::paths_eval_grad("):]
    assert 0 <= body.index("HMOGP_E_STATE") < body.index("hipSetDevice") < body.index("hipMemGetInfo") < body.index(".ensure(")
