"""CPU: the Ordinal (ordered probit) likelihood of DESIGN 9b at the layers that need no device -- the C enum and export, the
ctypes ids, the table registry, the descriptor, its metadata, the synthetic generator -- and the yardstick itself: the float64
restatement oracle/lik_ordinal.py against the high-precision one (tests/ordinal_ref_mp.py) on the committed grid
tests/golden/ordgrid.npz, under the criterion of tests/likgrid.py,  |got - R| <= C 2^-52 S  per element.

C_ORACLE: the largest |lik_ordinal - R| / (2^-52 S) over the committed grid per row class and output kind (ve, dm, dv), rounded
up to a power of two.  Measured 2026-10-16 (NumPy / SciPy on the CPU), raw figures:
    bulk   5.59 / 4.59 / 6.92          edge   1.09e5 / 296 / 294
    predictive (mean, variance)   1.97 / 1.60
The edge figure of ve is a narrow bin's: log P of a bin of 1e-6 sigma carries the cancellation of E(b) - E(a), 1e-16 / 1e-6
absolute, against S = |log P| ~ 14.  No element of the grid is non-finite and no element is excepted."""
import importlib.util
import os
import re

import numpy as np
import pytest
from scipy import special

import likgrid
from oracle import lik_ordinal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
GRID = os.path.join(ROOT, "tests", "golden", "ordgrid.npz")
BULK, EDGE = likgrid.BULK, likgrid.EDGE
KIND = np.array([0, 1, 2])

C_ORACLE = {BULK: (8.0, 8.0, 8.0), EDGE: (2.0 ** 17, 512.0, 512.0)}
C_ORACLE_PRED = (2.0, 2.0)                      # mean, variance


def c_kernel():
    """The kernel's constants: max(16, 4 C_ORACLE), the margin of DESIGN 9a (device erfcx / log / erfc are 1-2 ulp series)."""
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE.items()}


def c_kernel_pred():
    return tuple(max(16.0, 4.0 * a) for a in C_ORACLE_PRED)


def load_grid():
    return np.load(GRID)


def grid_groups(g, prefix=""):
    """[(kw, row indices)]: the rows that share one table (K, edges, sigma)."""
    K, E, s = g[prefix + "K"], g[prefix + "edges"], g[prefix + "sigma"]
    seen = {}
    for i in range(len(K)):
        key = (int(K[i]), float(s[i])) + tuple(float(x) for x in E[i, :K[i] - 1])
        seen.setdefault(key, []).append(i)
    return [(dict(bin_edges=list(k[2:]), sigma=k[1]), np.array(idx)) for k, idx in seen.items()]


def evaluate(g, fn):
    """fn(y, m, v, **kw) -> (ve, dm, dv) over the var_exp rows of the grid, packed [n, 3]."""
    out = np.empty((len(g["y"]), 3))
    for kw, idx in grid_groups(g):
        ve, dm, dv = fn(g["y"][idx], g["m"][idx], g["v"][idx], **kw)
        out[idx] = likgrid.pack(ve, dm, dv, len(idx))
    return out


# ---------------------------------------------------------------------------------------------------- ids, exports, descriptor
def test_header_declares_ordinal_id_and_table_export():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_ORDINAL\s*=\s*9\b", src)
    assert re.search(r"\bint\s+hmogp_ordinal_table\s*\(", src)
    assert int(re.search(r"#define HMOGP_ORDINAL_MAXK (\d+)", src).group(1)) >= 16
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump


def test_python_ids_dims_and_symbol():
    from hetmogp_amd import _lib, engine
    assert _lib.LIK_ORDINAL == 9 and _lib.LIK_IDS_BY_NAME["Ordinal"] == 9
    assert engine.LIK_IDS["Ordinal"] == 9
    assert engine.lik_dim_f("Ordinal", K=5) == 1
    assert "hmogp_ordinal_table" in _lib.EXPORTS and hasattr(_lib.lib, "hmogp_ordinal_table")
    from hetmogp_amd import synthetic
    assert synthetic._DIM_F["Ordinal"] == 1


def test_table_registry():
    """hmogp_ordinal_table needs no device: ids are positive integers, an identical table keeps its id, a different one gets
    another, and every invalid table is HMOGP_E_INVALID."""
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import ordinal_table, lik_param
    a = ordinal_table(bin_edges=[-1.25, 0.5, 3.0], sigma=0.75)
    assert a >= 1.0 and a == int(a)
    assert ordinal_table(K=4, bin_edges=[-1.25, 0.5, 3.0], sigma=0.75) == a
    assert lik_param("Ordinal", bin_edges=[-1.25, 0.5, 3.0], sigma=0.75) == a
    assert ordinal_table(bin_edges=[-1.25, 0.5, 3.0], sigma=0.5) != a
    assert ordinal_table(bin_edges=[-1.25, 0.5, 3.5], sigma=0.75) != a
    assert ordinal_table(K=_lib.ORDINAL_MAXK) >= 1.0
    inf, nan = float("inf"), float("nan")
    for kw in (dict(bin_edges=[]), dict(K=1), dict(K=_lib.ORDINAL_MAXK + 1), dict(bin_edges=[0.0, 0.0]), dict(bin_edges=[1.0, 0.5]),
               dict(bin_edges=[0.0, inf]), dict(bin_edges=[-inf, 0.0]), dict(bin_edges=[nan]), dict(K=3, sigma=0.0),
               dict(K=3, sigma=-1.0), dict(K=3, sigma=inf), dict(K=3, sigma=nan)):
        with pytest.raises(_lib.InvalidArgument) as ei:
            ordinal_table(**kw)
        assert "Ordinal" in str(ei.value), kw


def test_descriptor_rules_and_metadata():
    from hetmogp_amd import Ordinal
    o = Ordinal(K=5)
    assert o.get_metadata() == (1, 1, 1) and o.K == 5 and o.sigma == 1.0
    assert np.array_equal(o.bin_edges, [-1.5, -0.5, 0.5, 1.5])                  # b_k = k - K/2
    assert np.array_equal(Ordinal(None, 2).bin_edges, [0.0])                      # the reference's positional order: gp_link first
    o = Ordinal(bin_edges=[-1.0, 0.25, 4.0], sigma=0.3)
    assert o.K == 4 and o.kwargs() == {"K": 4, "bin_edges": [-1.0, 0.25, 4.0], "sigma": 0.3}
    assert Ordinal(K=4, bin_edges=[-1.0, 0.25, 4.0]).K == 4
    with pytest.raises(ValueError):
        Ordinal()                                                                 # at least one of K / bin_edges
    with pytest.raises(ValueError):
        Ordinal(K=5, bin_edges=[-1.0, 0.25, 4.0])                                 # both given must agree


def test_het_likelihood_metadata_with_ordinal():
    from hetmogp_amd import HetLikelihood, Gaussian, Ordinal, Categorical
    md = HetLikelihood([Gaussian(), Ordinal(K=5), Categorical(K=3)]).generate_metadata()
    assert md["function_index"].tolist() == [0, 1, 2, 2] and md["d_index"].tolist() == [0, 0, 0, 1]
    assert md["y_index"].tolist() == [0, 1, 2] and md["pred_index"].tolist() == [0, 1, 2, 2]


def test_synthetic_labels_cover_every_class():
    from hetmogp_amd.synthetic import make_case
    for kw in ({"K": 5}, {"bin_edges": [-2.0, -0.5, 0.1, 3.0], "sigma": 0.5}, {"K": 2}):
        K = kw.get("K", 5)
        _, _, Y = make_case([("Gaussian", {"sigma": 0.5}), ("Ordinal", kw)], [500, 2000], M=16, Q=2, seed=4)
        y = Y[1]
        assert y.shape == (2000, 1) and np.array_equal(y, np.round(y))
        assert sorted(np.unique(y).tolist()) == list(range(1, K + 1)), np.unique(y)


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_fixture_is_out_of_the_other_grids_way():
    assert not any(os.path.basename(p) == "ordgrid.npz" for p in likgrid.grid_files() + likgrid.reference_fixtures())
    largest = max(os.path.getsize(p) for p in likgrid.grid_files())
    assert os.path.getsize(GRID) < largest


def test_grid_design():
    g = load_grid()
    bulk = g["cls"] == BULK
    assert np.all(np.abs(g["m"][bulk]) <= 3.0) and np.all((g["v"][bulk] >= 1e-3) & (g["v"][bulk] <= 4.0))
    for i in np.where(bulk)[0]:
        w = np.diff(g["edges"][i, :g["K"][i] - 1]) / g["sigma"][i]
        assert np.all((w >= 0.25 * (1 - 1e-12)) & (w <= 4.0 * (1 + 1e-12)))
    assert {(int(k), int(y)) for k, y in zip(g["K"][bulk], g["y"][bulk])} == {(K, y) for K in (2, 3, 5, 11) for y in range(1, K + 1)}
    assert np.all(np.isfinite(g["R"])) and np.all(np.isfinite(g["S"])) and np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
    edge = ~bulk
    far = np.array([np.nanmin(np.abs(g["edges"][i] - g["m"][i])) / g["sigma"][i] for i in range(len(bulk))])
    assert far[edge].max() >= 999.0 and g["v"][edge].max() >= 1e4 and g["v"][edge].min() == 0.0
    assert g["R"][edge, 0].min() < -4e5                                           # P far below DBL_MIN (log DBL_MIN = -708)
    assert {1e-3, 1e3} <= set(g["sigma"][edge].tolist())


def test_float64_restatement_against_high_precision_grid():
    """Where C_ORACLE comes from; also the three conditions of DESIGN 9b on the restatement: no non-finite element, no exception
    list, no bulk row above the bulk constants."""
    g = load_grid()
    got = evaluate(g, lik_ordinal.var_exp)
    assert np.all(np.isfinite(got))
    w = likgrid.assert_rows(got, g["R"], g["S"], np.zeros(got.shape, np.uint8), KIND, g["cls"], C_ORACLE, "lik_ordinal on ordgrid")
    for c in (BULK, EDGE):                                                         # the constants are the measured figures, rounded up
        for k in range(3):
            assert w[c][k] > C_ORACLE[c][k] / 2.0, (c, k, w[c][k])
            assert C_ORACLE[c][k] <= 2.0 ** 27


def test_predictive_restatement_against_high_precision_rows():
    g = load_grid()
    got = np.empty((len(g["p_m"]), 2))
    logp = np.empty(len(g["p_m"]))
    for kw, idx in grid_groups(g, "p_"):
        mean, var = lik_ordinal.predictive(g["p_m"][idx], g["p_v"][idx], **kw)
        got[idx] = np.concatenate([mean, var], 1)
        logp[idx] = lik_ordinal.log_prob(g["p_y"][idx], g["p_m"][idx], g["p_v"][idx], **kw)
    r = np.abs(got - g["p_R"]) / (likgrid.EPS * g["p_S"])
    print("[ordgrid] predictive of lik_ordinal, worst |got - R| / (2^-52 S): mean %.3g variance %.3g" % tuple(r.max(0)))
    assert np.all(r <= np.array(C_ORACLE_PRED))
    assert np.all(np.abs(logp - g["p_logp"]) <= 1e-12 * np.maximum(1.0, np.abs(g["p_logp"])))


def test_fixture_regenerates_bit_identically():
    spec = importlib.util.spec_from_file_location("make_ordinal_grid", os.path.join(ROOT, "tools", "make_ordinal_grid.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    new, old = mod.build(), load_grid()
    assert sorted(new) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k


def test_probabilities_sum_to_one_and_probit_limit():
    rng = np.random.RandomState(3)
    N = 400
    m, v = rng.uniform(-6.0, 6.0, N), 10.0 ** rng.uniform(-6.0, 2.0, N)
    for K, sigma in ((2, 1.0), (3, 0.3), (5, 1.0), (11, 4.0)):
        e = np.sort(rng.uniform(-4.0, 4.0, K - 1)) + 1e-3 * np.arange(K - 1)
        P = lik_ordinal.class_probs(m, v, bin_edges=e, sigma=sigma)
        assert np.all(P >= 0.0) and np.max(np.abs(P.sum(1) - 1.0)) <= 4e-16 * K
    # K = 2 with b_1 = 0 is the probit Bernoulli: P(y = 2) = Phi(m / s), s = sqrt(sigma^2 + v)
    for sigma in (0.3, 1.0, 4.0):
        s = np.sqrt(sigma * sigma + v)
        mean, var = lik_ordinal.predictive(m, v, K=2, sigma=sigma)
        p = special.ndtr(m / s)
        assert np.max(np.abs(mean[:, 0] - (1.0 + p))) <= 4e-16 and np.max(np.abs(var[:, 0] - p * (1.0 - p))) <= 1e-15
        assert np.allclose(lik_ordinal.log_prob(np.full(N, 2.0), m, v, K=2, sigma=sigma), special.log_ndtr(m / s), rtol=1e-13, atol=0)
        # and var_exp's derivative at v = 0 is the probit score phi / (sigma Phi)
        ve, dm, dv = lik_ordinal.var_exp(np.full(N, 2.0), m, np.zeros(N), K=2, sigma=sigma)
        assert np.allclose(ve, special.log_ndtr(m / sigma), rtol=1e-13, atol=0)
        want = np.exp(-0.5 * (m / sigma) ** 2 - special.log_ndtr(m / sigma)) / (np.sqrt(2.0 * np.pi) * sigma)
        assert np.allclose(dm[:, 0], want, rtol=1e-12, atol=0)
