"""CPU: the Dirichlet likelihood of DESIGN 9d at the layers that need no device -- the C enum and limit, the ctypes ids, the
descriptor, its metadata with a multi-column Y, the synthetic generator -- and the yardstick itself: the float64 restatement
oracle/lik_dirichlet.py against the high-precision one (tests/dirichlet_ref_mp.py) on the committed grid tests/golden/dirgrid.npz,
under the criterion of tests/likgrid.py,  |got - R| <= C 2^-52 S  per element.

C_ORACLE: the largest |lik_dirichlet - R| / (2^-52 S) over the committed grid per row class and output kind (ve, dm, dv), rounded
up to a power of two.  Measured 2026-10-17 (NumPy / SciPy on the CPU), raw figures:
    bulk   1.22 / 1.06 / 1.40          edge   1.35 / 2.85 / 1.36
No element of the grid is non-finite, no element is excepted, no bulk row is above the bulk constants."""
import importlib.util
import os
import re

import mpmath
import numpy as np
import pytest

from oracle import lik_dirichlet
import dirichlet_ref_mp
import likgrid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
GRID = os.path.join(ROOT, "tests", "golden", "dirgrid.npz")
BULK, EDGE = likgrid.BULK, likgrid.EDGE

C_ORACLE = {BULK: (2.0, 2.0, 2.0), EDGE: (2.0, 4.0, 2.0)}


def c_kernel():
    """The kernel's constants: max(16, 4 C_ORACLE), the rule of DESIGN 9a (wave-shuffle summation order, 1-2 ulp special functions)."""
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE.items()}


def load_grid():
    return np.load(GRID)


def kind_of(K):
    return np.array([0] + [1] * K + [2] * K)


def grid_groups(g):
    """[(K, row indices)]"""
    return [(K, np.where(g["K"] == K)[0]) for K in (2, 3, 4)]


def evaluate(g, fn):
    """fn(y, m, v, K=K) -> (ve, dm, dv) over the rows of the grid: {K: packed [n_K, 1 + 2 K]}."""
    out = {}
    for K, idx in grid_groups(g):
        ve, dm, dv = fn(g["y"][idx, :K], g["m"][idx, :K], g["v"][idx, :K], K=K)
        out[K] = likgrid.pack(ve, dm, dv, len(idx))
    return out


def assert_grid(g, got, C, what):
    """The criterion per K; returns the worst figure per class and output kind over all K."""
    worst = {BULK: [0.0] * 3, EDGE: [0.0] * 3}
    for K, idx in grid_groups(g):
        n = 1 + 2 * K
        assert np.all(np.isfinite(got[K])), (what, K)
        w = likgrid.assert_rows(got[K], g["R"][idx, :n], g["S"][idx, :n], np.zeros(got[K].shape, np.uint8), kind_of(K), g["cls"][idx], C,
                                "%s, K = %d" % (what, K))
        for c in worst:
            worst[c] = [max(a, b) for a, b in zip(worst[c], w[c])]
    return worst


# ---------------------------------------------------------------------------------------------------- ids, limit, descriptor
def test_header_declares_dirichlet_id_and_limit():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_DIRICHLET\s*=\s*10\b", src)
    assert int(re.search(r"#define HMOGP_DIRICHLET_MAXK (\d+)", src).group(1)) == 4
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump


def test_python_ids_and_dims():
    from hetmogp_amd import _lib, engine, synthetic
    assert _lib.LIK_DIRICHLET == 10 and _lib.LIK_IDS_BY_NAME["Dirichlet"] == 10 and _lib.DIRICHLET_MAXK == 4
    assert engine.LIK_IDS["Dirichlet"] == 10
    assert engine.lik_dim_f("Dirichlet", K=3) == 3 and engine.lik_dim_y("Dirichlet", K=3) == 3 and engine.lik_dim_y("Beta") == 1
    assert engine.lik_param("Dirichlet", K=4) == 4.0
    assert synthetic._dim_f("Dirichlet", {"K": 3}) == 3


def test_descriptor_metadata_and_specs():
    from hetmogp_amd import HetLikelihood, Gaussian, Dirichlet, Categorical
    d = Dirichlet(3)
    assert d.get_metadata() == (3, 3, 3) and d.ismulti() is True and d.kwargs() == {"K": 3} and d.name == "Dirichlet"
    assert Dirichlet(K=2, gp_link=None).K == 2
    assert "zeros" in Dirichlet.__doc__                                       # the caller replaces them: the docstring says so
    h = HetLikelihood([Gaussian(), Dirichlet(3), Categorical(K=3)])
    md = h.generate_metadata()
    assert md["y_index"].tolist() == [0, 1, 1, 1, 2]
    assert md["function_index"].tolist() == [0, 1, 1, 1, 2, 2] and md["d_index"].tolist() == [0, 0, 1, 2, 0, 1]
    assert md["pred_index"].tolist() == [0, 1, 1, 1, 2, 2]
    assert h.specs()[1] == ("Dirichlet", {"K": 3}) and h.ismulti(1) and not h.ismulti(0)
    assert h.num_output_functions(md) == 6


def test_library_needs_a_device_for_the_family_as_for_every_other():
    """Without a device every entry point answers HMOGP_E_NO_DEVICE (there is no CPU path); with one the same calls succeed."""
    import torch
    from hetmogp_amd import _lib, engine
    y = np.array([[0.2, 0.3, 0.5], [0.6, 0.3, 0.1]])
    m, v = np.zeros((2, 3)), np.ones((2, 3))
    calls = (lambda: engine.Engine([("Dirichlet", {"K": 3})], Q=1, M=4, P=1).close(), lambda: engine.var_exp("Dirichlet", y, m, v, K=3),
             lambda: engine.predictive("Dirichlet", m, v, K=3), lambda: engine.sample("Dirichlet", m, K=3),
             lambda: engine.log_predictive_rows("Dirichlet", y, m, v, num_samples=4, K=3))
    for call in calls:
        if torch.cuda.is_available():
            call()
        else:
            with pytest.raises(_lib.HetMOGPError) as ei:
                call()
            assert ei.value.code == _lib.E_NO_DEVICE


def test_synthetic_compositions():
    from hetmogp_amd.synthetic import make_case
    prm, X, Y = make_case([("Gaussian", {"sigma": 0.5}), ("Dirichlet", {"K": 3})], [50, 200], M=16, Q=2, seed=4)
    assert Y[1].shape == (200, 3) and np.all(Y[1] > 0.0) and np.max(np.abs(Y[1].sum(1) - 1.0)) < 1e-12
    assert prm["W"].shape == (2, 4)


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_small_and_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "dirgrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    assert os.path.getsize(GRID) < likgrid.SIZE_BOUND // 8


def test_grid_design():
    g = load_grid()
    bulk = g["cls"] == BULK
    assert set(g["K"].tolist()) == {2, 3, 4} and all(np.any(bulk & (g["K"] == K)) and np.any(~bulk & (g["K"] == K)) for K in (2, 3, 4))
    assert (g["K"] == 4).sum() < (g["K"] == 3).sum() < (g["K"] == 2).sum()
    for i in range(len(bulk)):
        K = g["K"][i]
        y, m, v = g["y"][i, :K], g["m"][i, :K], g["v"][i, :K]
        assert np.all(np.isnan(g["y"][i, K:])) and np.all(np.isfinite(g["R"][i, :1 + 2 * K])) and np.all(np.isnan(g["R"][i, 1 + 2 * K:]))
        assert np.all(y > 0.0) and abs(y.sum() - 1.0) <= 1e-6                                   # what the library accepts
        assert np.all(np.abs(g["R"][i, :1 + 2 * K]) <= g["S"][i, :1 + 2 * K] * (1 + 1e-15))
        if bulk[i]:
            assert np.all(np.abs(m) <= 3.0) and np.all((v >= 1e-3) & (v <= 4.0))
    e = ~bulk
    assert np.nanmax(g["m"][e]) == 750.0 and np.nanmin(g["m"][e]) == -750.0                     # both sides of safe_exp
    assert {20.7, 20.75, -20.7, -20.75} <= set(g["m"][e][:, 0].tolist())                        # both sides of the clips of alpha
    assert np.nanmin(g["v"][e]) == 0.0 and np.nanmax(g["v"][e]) == 1e4
    assert np.nanmin(g["y"][e]) <= 1e-300 and np.any(np.isclose(g["y"][e], 1e-6, rtol=1e-3))
    assert np.any(np.nanmax(g["m"][e], 1) - np.nanmin(g["m"][e], 1) == 60.0)                    # one alpha 1e18 times another
    assert np.any(np.nanmax(g["m"][e], 1) == -30.0)                                             # all alpha at 1e-9
    assert np.any(g["m"][e] == np.log(1.4616321449683623))                                      # digamma's zero


def test_float64_restatement_against_high_precision_grid():
    """Where C_ORACLE comes from; also the three conditions on the restatement: no non-finite element, no exception list, no
    bulk row above the bulk constants (assert_grid applies the bulk constants to every bulk row and takes no exceptions)."""
    g = load_grid()
    w = assert_grid(g, evaluate(g, lik_dirichlet.var_exp), C_ORACLE, "lik_dirichlet on dirgrid")
    for c in (BULK, EDGE):                                                         # the constants are the measured figures, rounded up
        for k in range(3):
            assert w[c][k] > C_ORACLE[c][k] / 2.0, (c, k, w[c][k])


def test_float64_scale_matches_high_precision_scale():
    g = load_grid()
    for K, idx in grid_groups(g):
        S = lik_dirichlet.var_exp_scale(g["y"][idx, :K], g["m"][idx, :K], g["v"][idx, :K], K)
        assert np.allclose(S, g["S"][idx, :1 + 2 * K], rtol=1e-12, atol=0), K


def test_fixture_regenerates_bit_identically():
    spec = importlib.util.spec_from_file_location("make_dirichlet_grid", os.path.join(ROOT, "tools", "make_dirichlet_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.build(), load_grid()
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


def test_high_precision_trigamma_is_mpmath_s():
    with mpmath.mp.workdps(dirichlet_ref_mp.WORK_DPS):
        for x in (1e-9, 4e-9, 0.3, 1.4616321449683623, 7.5, 24.99, 25.0, 1e3, 1e9, 4e9):
            a, b = dirichlet_ref_mp.trigamma(mpmath.mpf(x)), mpmath.psi(1, mpmath.mpf(x))
            assert abs(a - b) <= abs(b) * mpmath.mpf(10) ** -(dirichlet_ref_mp.WORK_DPS - 2), x


# ---------------------------------------------------------------------------------------------------- properties of the model
def _bulk(rng, N, K):
    y = np.maximum(rng.dirichlet(np.full(K, 1.0), N), 1e-12)
    return y / y.sum(1, keepdims=True), rng.uniform(-3.0, 3.0, (N, K)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, K)))


def test_k2_is_the_oracle_s_beta_in_exact_mode():
    """K = 2 with y = (y, 1 - y) is Beta without its quirk (weights divided by sqrt(pi) once): same rule, same nodes.  Both sides
    are float64 evaluations of the same sums, so each sits within its bulk constant of the true value in units of 2^-52 S: Beta's
    (likgrid.C_ORACLE, exact mode) and this family's add."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(2)
    N = 200
    y2, m, v = _bulk(rng, N, 2)
    y1 = y2[:, 0]
    y2 = np.stack([y1, 1.0 - y1], 1)
    want = likgrid.pack(*lo.var_exp_all("Beta", y1, m, v, exact=True), N)
    got = likgrid.pack(*lik_dirichlet.var_exp(y2, m, v, K=2), N)
    S = lik_dirichlet.var_exp_scale(y2, m, v, 2)
    C = np.array(C_ORACLE[BULK])[kind_of(2)] + np.array(likgrid.c_oracle("Beta", "exact")[BULK])[kind_of(2)]
    r = np.abs(got - want) / (likgrid.EPS * S)
    relerr = np.max(np.abs(got - want) / np.abs(want), 0)
    print("K = 2 against Beta (exact): worst |a - b| / (2^-52 S) ve/dm/dv %s, worst relative error %s" %
          (" ".join("%.3g" % r[:, kind_of(2) == k].max() for k in range(3)), " ".join("%.3g" % relerr[kind_of(2) == k].max() for k in range(3))))
    assert np.all(r <= C[None, :]), r.max(0)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_decomposed_form_is_the_full_tensor_sum(K):
    """The contract's form differs from the plain tensor sum of log p and its derivatives by (sum(w) - 1) per dimension only."""
    y, m, v = _bulk(np.random.RandomState(K), 12, K)
    a = likgrid.pack(*lik_dirichlet.var_exp(y, m, v, K), 12)
    b = likgrid.pack(*lik_dirichlet.var_exp_full(y, m, v, K), 12)
    S = lik_dirichlet.var_exp_scale(y, m, v, K)
    assert np.all(np.abs(a - b) <= 64.0 * likgrid.EPS * S)


@pytest.mark.parametrize("K", [3, 4])
def test_derivatives_are_those_of_ve(K):
    """dm, dv of the 10-node rule against central differences, in m and in v, of a FINER rule's ve (T = 16 per dimension): the two
    agree as far as the 10-node rule has converged, 1e-9 .. 1e-7 for v <= 0.5 (h = 1e-4: truncation 1e-8 relative, rounding 1e-11)."""
    rng = np.random.RandomState(10 + K)
    N = 4
    y, m, _ = _bulk(rng, N, K)
    m, v = 0.5 * m, np.exp(rng.uniform(np.log(1e-3), np.log(0.5), (N, K)))
    _, dm, dv = lik_dirichlet.var_exp(y, m, v, K)
    h = 1e-4
    fine = lambda mm, vv: lik_dirichlet.var_exp(y, mm, vv, K, T=16)[0]
    worst = 0.0
    for k in range(K):
        e = np.zeros(K)
        e[k] = h
        fm = (fine(m + e, v) - fine(m - e, v)) / (2 * h)
        hv = h * v[:, k]
        ev = np.zeros((N, K))
        ev[:, k] = hv
        fv = (fine(m, v + ev) - fine(m, v - ev)) / (2 * hv)
        scale = 1.0 + np.abs(fm) + np.abs(fv)
        worst = max(worst, np.max(np.abs(dm[:, k] - fm) / scale), np.max(np.abs(dv[:, k] - fv) / scale))
    print("K = %d: worst |derivative - central difference of the finer rule| / (1 + |.|) = %.3g" % (K, worst))
    assert worst <= 1e-6


def test_outputs_are_finite_at_the_extremes():
    for K in (2, 3, 4):
        for m0 in (750.0, -750.0, 30.0, -30.0, 20.7, -20.7, 0.0):
            for v0 in (0.0, 1e-12, 1.0, 1e4):
                for tiny in (1e-300, 1e-6):
                    y = np.full((1, K), (1.0 - tiny) / (K - 1))
                    y[0, 0] = tiny
                    m = np.full((1, K), 0.3)
                    m[0, K - 1] = m0
                    out = likgrid.pack(*lik_dirichlet.var_exp(y, m, np.full((1, K), v0), K), 1)
                    assert np.all(np.isfinite(out)), (K, m0, v0, tiny)


@pytest.mark.parametrize("K", [2, 3, 4])
def test_predictive_means_sum_to_one(K):
    rng = np.random.RandomState(K)
    N = 8 if K == 4 else 40
    m, v = rng.uniform(-3.0, 3.0, (N, K)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N, K)))
    for T in (10, 20) if K < 4 else (10,):
        mean, var = lik_dirichlet.predictive(m, v, K, gh_T=T)
        assert mean.shape == (N, K) and np.all(mean > 0.0) and np.all(var > 0.0)
        assert np.max(np.abs(mean.sum(1) - 1.0)) <= 16 * likgrid.EPS                           # (sum(w))^K = 1 to rounding
    # v = 0: the moments at f = m
    mean, var = lik_dirichlet.predictive(m, np.zeros_like(m), K, gh_T=10)
    mu, vr = lik_dirichlet.moments(m)
    assert np.allclose(mean, mu, rtol=1e-13, atol=0) and np.allclose(var, vr, rtol=1e-9, atol=1e-16)
