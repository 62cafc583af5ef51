"""CPU: the parameter group "likelihood parameters"  at the layers that need no device -- the header's five new
symbols beside an unchanged ABI version and eval_flags mask, the ctypes binding, the descriptors' Params and their chain rule --
and the yardstick of the GPU tests: the float64 restatement of the three per-row derivatives (tests/likparam_ref.py) against the
high-precision evaluation of the same finite rules, under the project's criterion  |got - R| <= C 2^-52 S  per element.

C_ORACLE: the largest |restatement - R| / (2^-52 S) per family, row class and output, rounded up to a power of two.  Measured
2026-10-18 (NumPy / SciPy on the CPU), raw figures:
    Gaussian  d sigma             bulk 0.70                  edge 0 (every element correctly rounded)
    Student   d nu                bulk 0.15                  edge 16.9
    Ordinal   d lo / d hi / d s   bulk 47.3 / 197 / 1.62     edge 1.37e4 / 1.43e4 / 5.36
The Ordinal figures of d lo / d hi are relative errors (their addends have one sign, S = |R|): in the bulk they are the rounding of
d = (a^2 - b^2) / 2 ~ 200 in exp(-d) at K = 32 (a bin 20 sigma from f), at the edge a bin of 1e-3 sigma carries the cancellation of
E(b) - E(a), 1e-16 / 1e-3.  No element of the grid is non-finite and none is excepted."""
import os
import re

import numpy as np
import pytest

import likparam_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")
BULK, EDGE = L.BULK, L.EDGE

C_ORACLE = {
    "Gaussian": {BULK: (1.0,), EDGE: (1.0,)},
    "Student": {BULK: (1.0,), EDGE: (32.0,)},
    "Ordinal": {BULK: (64.0, 256.0, 2.0), EDGE: (2.0 ** 14, 2.0 ** 14, 8.0)},
}
NEW_SYMBOLS = ("hmogp_var_exp_dparam", "hmogp_lik_param_count", "hmogp_set_lik_params", "hmogp_lik_grad_enable", "hmogp_lik_grad_read")


def c_kernel(name):
    """The kernels' constants: max(16, 4 C_ORACLE), the rule of tests/test_ordinal_gpu.py."""
    return {c: tuple(max(16.0, 4.0 * a) for a in t) for c, t in C_ORACLE[name].items()}


def c_kernel_vs_restatement(name):
    """Kernel against the float64 restatement instead of R: each sits within its own constant of R, so the two constants add."""
    k = c_kernel(name)
    return {c: tuple(a + b for a, b in zip(k[c], C_ORACLE[name][c])) for c in k}


def assert_within(got, g, C, what):
    r = L.ratios(got, g)
    w = {c: r[g["cls"] == c].max(0) for c in (BULK, EDGE)}
    print("[likparam] %-36s worst |got - R| / (2^-52 S): bulk %s | edge %s" %
          (what, " ".join("%.3g" % a for a in w[BULK]), " ".join("%.3g" % a for a in w[EDGE])))
    assert np.all(np.isfinite(got)), what
    bound = np.array([C[c] for c in g["cls"]])
    bad = np.argwhere(r > bound)
    assert bad.size == 0, (what, [(int(i), int(j), float(r[i, j]), float(bound[i, j])) for i, j in bad[:8]])
    return w


# ---------------------------------------------------------------------------------------------------- header, binding
def test_header_declares_the_new_symbols_and_nothing_else_moves():
    src = open(HEADER).read()
    for n in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % n, src), n
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8          # additive: no ABI bump
    flags = dict(re.findall(r"#define (HMOGP_EVAL_\w+) (\d+)u", src))
    assert flags == {"HMOGP_EVAL_STRICT_QF": "1", "HMOGP_EVAL_NO_G_L": "2"}               # no new eval_flags bit: 4 stays refused
    assert int(re.search(r"#define HMOGP_ORDINAL_MAXTABLES (\d+)", src).group(1)) == 4096


def test_binding_carries_the_new_symbols():
    from hetmogp_amd import _lib, engine
    assert _lib.ABI_VERSION == 8
    for n in NEW_SYMBOLS:
        assert n in _lib.EXPORTS and hasattr(_lib.lib, n), n
    for m in ("lik_param_count", "set_lik_params", "lik_grad_enable", "lik_grad"):
        assert hasattr(engine.Engine, m), m
    assert callable(engine.var_exp_dparam)


# ---------------------------------------------------------------------------------------------------- the yardstick
def test_grid_design():
    G = L.grid()
    o = G["Ordinal"]
    Ks = {len(kw["bin_edges"]) + 1 for kw, _ in o["groups"]}
    assert Ks == {2, 3, 5, 11, 32}
    bulk = o["cls"] == BULK
    assert np.all(np.abs(o["m"][bulk]) <= 3.0) and np.all((o["v"][bulk] >= 1e-3) & (o["v"][bulk] <= 4.0))
    width = min(np.min(np.diff(kw["bin_edges"])) / kw["sigma"] for kw, idx in o["groups"] if len(kw["bin_edges"]) > 1)
    assert width <= 1e-3 * (1 + 1e-9)                                                       # bins down to 1e-3 sigma
    far = max(np.max(np.abs(o["m"][idx])) / kw["sigma"] for kw, idx in o["groups"])
    assert far >= 40.0 * (1 - 1e-12)                                                        # |m| up to 40 sigma
    assert {kw["deg_free"] for kw, idx in G["Student"]["groups"] if np.any(G["Student"]["cls"][idx] == EDGE)} == \
        {0.7, 2.5, 5.0, 30.0, 64.0, 1e3, 1e6}
    for name in G:
        g = G[name]
        assert np.all(np.isfinite(g["R"])) and np.all(np.abs(g["R"]) <= g["S"] * (1 + 1e-15))
    # an infinite cut contributes exactly 0: label 1 has no lower cut, label K no upper one
    for kw, idx in o["groups"]:
        K = len(kw["bin_edges"]) + 1
        y = o["y"][idx]
        assert np.all(o["R"][idx][y == 1, 0] == 0.0) and np.all(o["R"][idx][y == K, 1] == 0.0)


@pytest.mark.parametrize("name", ["Gaussian", "Student", "Ordinal"])
def test_restatement_against_high_precision_rules(name):
    """Where C_ORACLE comes from: the constants are the measured figures rounded up, not chosen in advance."""
    g = L.grid()[name]
    got = L.evaluate(g, L.dparam, name)
    w = assert_within(got, g, C_ORACLE[name], "restatement, " + name)
    for c in (BULK, EDGE):
        for k, a in enumerate(C_ORACLE[name][c]):
            assert a == 1.0 or w[c][k] > a / 2.0, (name, c, k, w[c][k])


def test_student_constant_series_joins_the_digamma_form():
    """C'(nu) is O(nu^-2) while its terms are O(log nu): from nu = 64 on the series must hold RELATIVE accuracy."""
    import mpmath
    for nu in (64.0, 65.5, 100.0, 1e3, 1e6, 1e12):
        with mpmath.mp.workdps(60):
            want = float(sum(L.student_dlogc_mp(nu)))
        assert abs(L.student_dlogc(nu) - want) <= 4e-16 * abs(want), nu
    for nu in (0.7, 5.0, 30.0, 63.999):
        with mpmath.mp.workdps(60):
            t = L.student_dlogc_mp(nu)
        assert abs(L.student_dlogc(nu) - float(sum(t))) <= 4 * L.EPS * float(sum(abs(x) for x in t)), nu


def test_derivatives_are_derivatives_of_the_float64_oracle():
    """Central differences of the oracle's own var_exp (oracle/: lik_ordinal, lik_student, the Gaussian closed form) in the parameter."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(2)
    n = 40
    m, v = rng.uniform(-2, 2, (n, 2)), np.exp(rng.uniform(-3, 1, (n, 2)))
    h = 1e-6

    def fd(name, y, mm, vv, key, kw):
        a, b = dict(kw), dict(kw)
        a[key], b[key] = kw[key] * (1 + h), kw[key] * (1 - h)
        return (lo.var_exp_all(name, y, mm, vv, **a)[0] - lo.var_exp_all(name, y, mm, vv, **b)[0]).reshape(-1) / (2 * h * kw[key])

    y = rng.randn(n, 1)
    assert np.allclose(L.gaussian_dsigma(y, m[:, 0], v[:, 0], sigma=0.7)[:, 0], fd("Gaussian", y, m[:, :1], v[:, :1], "sigma", dict(sigma=0.7)),
                       rtol=1e-7, atol=1e-8)
    assert np.allclose(L.student_dnu(y, m, v, deg_free=4.0)[:, 0], fd("Student", y, m, v, "deg_free", dict(deg_free=4.0)), rtol=1e-6, atol=1e-8)
    e = np.array([-1.3, -0.2, 0.9, 2.0])
    yo = rng.randint(1, 6, (n, 1)).astype(float)
    d = L.ordinal_dparam(yo, m[:, 0], v[:, 0], bin_edges=e, sigma=0.8)
    assert np.allclose(d[:, 2], fd("Ordinal", yo, m[:, :1], v[:, :1], "sigma", dict(bin_edges=e, sigma=0.8)), rtol=1e-6, atol=1e-8)
    for c in range(4):                                   # cut c + 1: d hi of label c + 1, d lo of label c + 2
        ep, em = e.copy(), e.copy()
        ep[c] += h
        em[c] -= h
        want = (lo.var_exp_all("Ordinal", yo, m[:, :1], v[:, :1], bin_edges=ep, sigma=0.8)[0] -
                lo.var_exp_all("Ordinal", yo, m[:, :1], v[:, :1], bin_edges=em, sigma=0.8)[0]).reshape(-1) / (2 * h)
        got = np.where(yo[:, 0] == c + 1, d[:, 1], 0.0) + np.where(yo[:, 0] == c + 2, d[:, 0], 0.0)
        assert np.allclose(got, want, rtol=1e-6, atol=1e-8), c
    g = L.ordinal_bin_gradient(yo, d, 5)
    assert np.isclose(g[:4].sum(), d[:, 0].sum() + d[:, 1].sum()) and np.isclose(g[4], d[:, 2].sum())


# ---------------------------------------------------------------------------------------------------- descriptors
def test_descriptors_defaults_off_and_current_values():
    from hetmogp_amd import Gaussian, Student, Ordinal
    assert Gaussian(sigma=0.3).learnable_params() == [] and Student(deg_free=4.0).learnable_params() == []
    assert Ordinal(K=5).learnable_params() == []
    g = Gaussian(sigma=0.3, learn_sigma=True)
    (n, p), = g.learnable_params()
    assert n == "sigma" and p.positive and float(p.values[0]) == 0.3 and g.sigma == 0.3 and isinstance(g.sigma, float)
    p.values[...] = 0.4
    assert g.sigma == 0.4 and g.kwargs() == {"sigma": 0.4}
    s = Student(deg_free=4.0, learn_deg_free=True)
    assert [n for n, _ in s.learnable_params()] == ["deg_free"] and s.learnable_params()[0][1].positive
    o = Ordinal(bin_edges=[-1.0, 0.25, 4.0], sigma=0.3, learn_edges=True, learn_sigma=True)
    names = [n for n, _ in o.learnable_params()]
    assert names == ["edge0", "gaps", "sigma"]
    d = dict(o.learnable_params())
    assert not d["edge0"].positive and d["gaps"].positive and d["sigma"].positive
    assert np.allclose(o.bin_edges, [-1.0, 0.25, 4.0]) and isinstance(o.bin_edges, np.ndarray)
    d["gaps"].values[...] = [2.0, 1.0]
    assert np.allclose(o.bin_edges, [-1.0, 1.0, 2.0]) and o.kwargs()["bin_edges"] == [-1.0, 1.0, 2.0]
    assert np.allclose(o.engine_values(), [-1.0, 1.0, 2.0, 0.3])
    # chain rule from the raw gradient (g_1 .. g_{K-1}, g_sigma): g_{b_1} = sum_k g_k, g_{delta_j} = sum_{k > j} g_k
    o.set_engine_gradient(np.array([1.0, 10.0, 100.0, 7.0]))
    assert d["edge0"].gradient[0] == 111.0 and d["gaps"].gradient.tolist() == [110.0, 100.0] and d["sigma"].gradient[0] == 7.0
    o2 = Ordinal(K=3, learn_sigma=True)                                               # sigma alone: the cuts stay what they are
    assert [n for n, _ in o2.learnable_params()] == ["sigma"]
    o2.set_engine_gradient(np.array([1.0, 2.0, 3.0]))
    assert o2.learnable_params()[0][1].gradient[0] == 3.0


def test_ordinal_attributes_stay_assignable():
    from hetmogp_amd import Ordinal
    for learn in (False, True):
        o = Ordinal(bin_edges=[-1.0, 0.25, 4.0], sigma=0.3, learn_edges=learn, learn_sigma=learn)
        o.sigma = 0.7
        o.bin_edges = [-2.0, 0.0, 0.5]
        assert o.sigma == 0.7 and np.allclose(o.bin_edges, [-2.0, 0.0, 0.5]) and o.kwargs()["sigma"] == 0.7
        if learn:
            assert np.allclose(o.engine_values(), [-2.0, 0.0, 0.5, 0.7])
        with pytest.raises(ValueError):
            o.bin_edges = [0.0, 1.0]
