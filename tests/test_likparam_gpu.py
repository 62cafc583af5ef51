"""GPU: the parameter group "likelihood parameters"  through every layer -- the per-row derivative kernels against the
high-precision rules and the float64 restatement (tests/likparam_ref.py; constants: tests/test_likparam_cpu.py), the engine's
gradient on every path against the oracle's q(f) rows and against central differences of the oracle's ELBO, mutable parameters
(a private table per Ordinal task, thousands of updates), refusals, the switch, and the model facade.

Kernel bounds = max(16, 4 C_ORACLE):  Gaussian 16 | 16,  Student 16 | 128,  Ordinal 256 / 1024 / 16 | 2^16 / 2^16 / 32  (bulk | edge).
Measured on one MI355X, 2026-10-18, largest |got - R| / (2^-52 S), raw figures:
    Gaussian  d sigma             bulk 0.696                 edge 0
    Student   d nu                bulk 2.31                  edge 17.1
    Ordinal   d lo / d hi / d s   bulk 46.7 / 197 / 1.81     edge 1.37e4 / 1.43e4 / 4.47
no non-finite element, no exception list.  Engine gradient against batch_scale * sum_rows restatement on the oracle's q(f) rows: largest
element-wise excess over all paths 4.0e-8 (of 1); against the central difference of the oracle's ELBO: relative 2.1e-8 (Gaussian sigma),
3.7e-9 / 9.5e-10 / 5.9e-10 / 6.0e-10 (cuts of K = 5), 1.9e-8 (Ordinal sigma), 2.7e-9 (nu).  Facade, three VEM iterations on the toy: final
ELBO -838.40 learnable against -867.33 fixed; sigma 1.0 -> 0.9275 (true 0.2); cuts 0.4 x true -> [-0.600, -0.194, 0.212, 0.618]."""
import warnings

import numpy as np
import pytest

import likparam_ref as L
import model_cases as mc
import test_likparam_cpu as pc
from conftest import assert_parity, elementwise_excess

pytestmark = pytest.mark.gpu

FAMILIES = ["Gaussian", "Student", "Ordinal"]
EDGES5 = [-2.0, -0.9, 0.1, 1.7]
GAUSS = ("Gaussian", {"sigma": 0.5})
STUD = ("Student", {"deg_free": 5.0})
ORD3 = ("Ordinal", {"K": 3, "bin_edges": [-0.8, 0.45], "sigma": 0.3})
ORD5 = ("Ordinal", {"K": 5, "bin_edges": EDGES5, "sigma": 0.8})
ORD11 = ("Ordinal", {"K": 11})
ORD32 = ("Ordinal", {"K": 32})
SETS = {"Gaussian+Ordinal5+Bernoulli": [GAUSS, ORD5, ("Bernoulli", {})], "Student+Ordinal3+Ordinal11": [STUD, ORD3, ORD11], "Ordinal32": [ORD32]}
NS = [300, 257, 129]


def _gpu(name, y, m, v, **kw):
    from hetmogp_amd.engine import var_exp_dparam
    return var_exp_dparam(name, y, m, v, **kw)


# ------------------------------------------------------------------------------------------------ 1. row by row
@pytest.mark.parametrize("name", FAMILIES)
def test_rows_on_the_high_precision_grid(name):
    g = L.grid()[name]
    got = L.evaluate(g, _gpu, name)
    pc.assert_within(got, g, pc.c_kernel(name), "kernel, " + name)


def _bulk_rows(name, N, seed):
    rng = np.random.RandomState(seed)
    J = 2 if name == "Student" else 1
    m, v = rng.uniform(-3.0, 3.0, (N, J)), 10.0 ** rng.uniform(-3.0, np.log10(4.0), (N, J))
    if name == "Gaussian":
        return dict(sigma=0.7), m[:, 0] + 0.7 * rng.randn(N), m, v
    if name == "Student":
        return dict(deg_free=4.0), m[:, 0] + np.exp(0.5 * m[:, 1]) * rng.standard_t(4.0, N), m, v
    return dict(bin_edges=EDGES5, sigma=0.8), rng.randint(1, 6, N).astype(float), m, v


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", FAMILIES)
def test_rows_match_restatement(name, N):
    """Bulk-range rows.  Kernel and restatement each sit within their own bulk constant of the true value: the two constants add."""
    kw, y, m, v = _bulk_rows(name, N, 31 * N + len(name))
    got = _gpu(name, y, m, v, **kw)
    want, S = L.dparam(name, y, m, v, **kw), L.dparam_scale(name, y, m, v, **kw)
    assert got.shape == want.shape == (N, 3 if name == "Ordinal" else 1) and np.all(np.isfinite(got))
    r = L.ratios(got, dict(R=want, S=S))               # (0 where got == want: an infinite cut's element is exactly 0, and so is its S)
    assert np.all(r <= np.array(pc.c_kernel_vs_restatement(name)[L.BULK])[None, :]), (name, N, r.max(0))


@pytest.mark.parametrize("name", FAMILIES)
def test_rows_are_position_independent(name):
    kw, y, m, v = _bulk_rows(name, 130, 5)
    base = _gpu(name, y, m, v, **kw)
    rng = np.random.RandomState(0)
    for shift in (1, 63, 64, 257):
        perm = rng.permutation(len(y))
        pad = np.concatenate([np.arange(shift) % len(y), perm])
        assert np.array_equal(_gpu(name, y[pad], m[pad], v[pad], **kw)[shift:], base[perm]), shift


def test_rows_refusals():
    from hetmogp_amd import _lib
    y, m, v = np.ones(4), np.zeros((4, 1)), np.ones((4, 1))
    for name, kw in (("Bernoulli", {}), ("Poisson", {}), ("Categorical", {"K": 2})):
        with pytest.raises(_lib.InvalidArgument):
            _gpu(name, y, m, v, **kw)
    with pytest.raises(_lib.InvalidArgument):
        _gpu("Student", y, np.zeros((4, 2)), np.ones((4, 2)), deg_free=-1.0)
    with pytest.raises(_lib.InvalidArgument):
        _gpu("Ordinal", np.array([1.0, 7.0, 2.0, 1.0]), m, v, K=3)
    assert np.all(np.isfinite(_gpu("Ordinal", y, m, v, K=3)))


# ------------------------------------------------------------------------------------------------ 2. whole model, every path
def _want_lik_grads(case, bs=None, rows=None, strict=False):
    """batch_scale * sum_rows restatement(y, m, v), (m, v) the oracle's q(f) rows; {task: gradient in the engine's layout}."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = case
    if strict:
        prob = dict(prob, strict_qf=True)
    if rows is not None:
        X, Y = [x[b:e] for x, (b, e) in zip(X, rows)], [y[b:e] for y, (b, e) in zip(Y, rows)]
    bs = [1.0] * len(X) if bs is None else bs
    out_rows = []
    so.local_stats(prm, prob, so.u_algebra(prm, prob), X, Y, bs, rows_out=out_rows)
    want = {}
    for r in out_rows:
        t = r["t"]
        name, kw = prob["specs"][t]
        if name not in FAMILIES:
            continue
        d = L.dparam(name, Y[t], r["m"], r["v"], **kw)
        g = L.ordinal_bin_gradient(Y[t], d, kw["K"]) if name == "Ordinal" else d.sum(0)
        want[t] = bs[t] * g
    return want


def _check_lik_grads(e, want, what):
    for t, w in want.items():
        got = e.lik_grad(t)
        print("[lik_grad] %-28s task %d: element-wise excess %.3g" % (what, t, elementwise_excess(got, w)))
        assert_parity(got, w, "%s lik_grad[%d]" % (what, t))


@pytest.fixture(scope="module", params=sorted(SETS))
def case128(request):
    specs = SETS[request.param]
    Ns = NS[:len(specs)]
    return mc.family_case(4100 + len(specs), specs, Ns, 128, 2, 1), Ns


def test_engine_gradient_one_pool_several_pools_minibatch(case128):
    case, Ns = case128
    prm, prob, X, Y = case
    want = _want_lik_grads(case)
    rb = [n // 5 for n in Ns]
    re = [min(n, b + max(1, n // 3)) for n, b in zip(Ns, rb)]
    bs = [float(n) / (e - b) for n, b, e in zip(Ns, rb, re)]
    wantb = _want_lik_grads(case, bs, list(zip(rb, re)))
    for kw in ({}, {"chunk_rows": 97}):
        e = mc.make_engine(prob, X, Y, **kw)
        e.lik_grad_enable(True)
        mc.run(e, prm)
        _check_lik_grads(e, want, "pools %s" % (kw or "one"))
        first = [e.lik_grad(t) for t in want]
        mc.run(e, prm)
        assert all(np.array_equal(a, e.lik_grad(t)) for a, t in zip(first, want))       # fixed-order sums: the same bits
        mc.run(e, prm, bs, row_begin=rb, row_end=re)
        _check_lik_grads(e, wantb, "minibatch %s" % (kw or "one"))
        e.close()


@pytest.mark.parametrize("key", sorted(SETS))
def test_engine_gradient_small_path_and_regular_kernels(key):
    specs = SETS[key]
    Ns = NS[:len(specs)]
    case = mc.family_case(4200 + len(specs), specs, Ns, 48, 2, 1)
    prm, prob, X, Y = case
    want = _want_lik_grads(case)
    es, er = mc.make_engine(prob, X, Y), mc.make_engine(prob, X, Y, small_path=False)
    es.lik_grad_enable(True), er.lik_grad_enable(True)
    seen = []
    for _ in range(3):                                     # the third is a replay of the captured graph
        mc.run(es, prm)
        seen.append([es.lik_grad(t) for t in want])
    assert es.graph_stats()[0] >= 1 and es.graph_stats()[1] >= 1 and er.graph_stats() == (0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(seen[0], seen[2]))
    _check_lik_grads(es, want, "small path, replayed")
    mc.run(er, prm)
    _check_lik_grads(er, want, "small_path=False")
    # a replay with ANOTHER batch scale: the captured kernels read it from the parameter block
    bs = [1.5, 2.0, 3.0][:len(specs)]
    for _ in range(3):
        mc.run(es, prm, bs)
    _check_lik_grads(es, _want_lik_grads(case, bs), "small path, batch scale")
    es.close(), er.close()


@pytest.mark.parametrize("key", sorted(SETS))
def test_engine_gradient_strict_qf(key):
    specs = SETS[key]
    Ns = NS[:len(specs)]
    case = mc.family_case(4300 + len(specs), specs, Ns, 128, 2, 1)
    prm, prob, X, Y = case
    want = _want_lik_grads(case, strict=True)
    e = mc.make_engine(prob, X, Y, strict_qf=True)
    e.lik_grad_enable(True)
    mc.run(e, prm)
    _check_lik_grads(e, want, "strict q(f)")
    first = [e.lik_grad(t) for t in want]
    mc.run(e, prm)
    assert all(np.array_equal(a, e.lik_grad(t)) for a, t in zip(first, want))           # the same bits on this path too
    d = mc.make_engine(prob, X, Y)                                                       # per-evaluation flag on a default engine
    d.lik_grad_enable(True)
    mc.run(d, prm, strict_qf=True)
    _check_lik_grads(d, want, "strict q(f) by eval flag")
    e.close(), d.close()


# ------------------------------------------------------------------------------------------------ 3. derivative of the ELBO
def test_gradient_is_the_derivative_of_the_oracles_elbo():
    """Central difference of the ORACLE's ELBO at theta (1 +- 1e-4), per parameter, every cut of K = 5 included.  For these shapes
    (|ELBO| < 1e4, N <= 300) the quotient's rounding, 2^-52 |ELBO| / (2 h theta), and its truncation, h^2 theta^2 |f'''| / 6, are below
    1e-7 relative; asserted: element-wise 1e-5 relative with the project's 1e-9 floor."""
    from oracle import svmogp_oracle as so
    specs = [GAUSS, ORD5, STUD]
    case = mc.family_case(4400, specs, NS, 16, 2, 1)
    prm, prob, X, Y = case
    e = mc.make_engine(prob, X, Y)
    e.lik_grad_enable(True)
    mc.run(e, prm)
    h = 1e-4

    def elbo(t, key, idx, factor):
        sp = [(n, dict(kw)) for n, kw in specs]
        if idx is None:
            sp[t][1][key] = sp[t][1][key] * factor
        else:
            sp[t][1][key] = list(sp[t][1][key])
            sp[t][1][key][idx] *= factor
        return so.elbo_grad_fused(prm, so.make_problem(sp, prob["Q"], prob["M"], prob["P"]), X, Y)["elbo"]

    plan = {0: [("sigma", None)], 1: [("bin_edges", i) for i in range(4)] + [("sigma", None)], 2: [("deg_free", None)]}
    for t, params in plan.items():
        fd = []
        for key, idx in params:
            theta = specs[t][1][key] if idx is None else specs[t][1][key][idx]
            fd.append((elbo(t, key, idx, 1 + h) - elbo(t, key, idx, 1 - h)) / (2 * h * theta))
        got, fd = e.lik_grad(t), np.array(fd)
        ex = elementwise_excess(got, fd)
        print("[lik_grad] task %d vs central difference of the oracle's ELBO: relative %s, excess %.3g" %
              (t, np.array2string(np.abs(got - fd) / np.abs(fd), precision=2), ex))
        assert ex <= 1.0, (t, got, fd)
    e.close()


# ------------------------------------------------------------------------------------------------ 4. updates
NEW = {0: [0.37], 1: [-1.7, -0.2, 0.3, 2.4, 0.55], 2: [7.5]}


def _all_outputs(e, prm, tasks):
    out = mc.run(e, prm)
    return [np.array(out[k], copy=True) for k in mc.KEYS] + [e.lik_grad(t) for t in tasks]


@pytest.mark.parametrize("M", [128, 48], ids=["regular", "small-path-replayed"])
def test_update_equals_a_fresh_engine(M):
    from oracle import svmogp_oracle as so
    specs = [GAUSS, ORD5, STUD]
    prm, prob, X, Y = mc.family_case(4500, specs, NS, M, 2, 1)
    e = mc.make_engine(prob, X, Y)
    e.lik_grad_enable(True)
    assert [e.lik_param_count(t) for t in range(3)] == [1, 5, 1]
    for _ in range(3):
        old = _all_outputs(e, prm, NEW)
    for t, vals in NEW.items():
        e.set_lik_params(t, vals)
    for _ in range(3):
        got = _all_outputs(e, prm, NEW)
    new_specs = [("Gaussian", {"sigma": 0.37}), ("Ordinal", {"K": 5, "bin_edges": NEW[1][:4], "sigma": 0.55}), ("Student", {"deg_free": 7.5})]
    f = mc.make_engine(so.make_problem(new_specs, 2, M, 1), X, Y)
    f.lik_grad_enable(True)
    for _ in range(3):
        want = _all_outputs(f, prm, NEW)
    if M == 48:
        assert e.graph_stats()[1] >= 1 and f.graph_stats()[1] >= 1
    assert not np.array_equal(old[0], got[0])
    for a, b, k in zip(got, want, mc.KEYS + ["lik_grad"] * 3):
        assert np.array_equal(a, b), k
    e.close(), f.close()


def test_thousands_of_updates_do_not_touch_the_registry():
    """5000 distinct tables on one task: the process-wide registry holds 4096."""
    prm, prob, X, Y = mc.family_case(4600, [("Ordinal", {"K": 4})], [8], 8, 1, 1)
    e = mc.make_engine(prob, X, Y)
    e.lik_grad_enable(True)
    for i in range(5000):
        e.set_lik_params(0, [-1.0 - 1e-4 * i, 0.0, 1.0 + 1e-4 * i, 1.0 + 1e-5 * i])
    out = mc.run(e, prm)
    assert np.isfinite(out["elbo"]) and np.all(np.isfinite(e.lik_grad(0)))
    from hetmogp_amd.engine import ordinal_table                   # ... which still takes new tables afterwards
    assert ordinal_table(bin_edges=[-3.25, 0.125, 2.5], sigma=0.875) >= 1.0
    e.close()


def test_refusals_leave_the_engine_unchanged():
    from hetmogp_amd import _lib
    specs = [GAUSS, ORD5, STUD, ("Bernoulli", {})]
    prm, prob, X, Y = mc.family_case(4700, specs, NS + [100], 128, 2, 1)
    e = mc.make_engine(prob, X, Y)
    e.lik_grad_enable(True)
    tasks = (0, 1, 2)
    base = _all_outputs(e, prm, tasks)
    nan, inf = float("nan"), float("inf")
    bad = [(1, [-1.0, -1.0, 0.0, 1.0, 0.5]), (1, [-1.0, 0.5, 0.0, 1.0, 0.5]), (1, EDGES5 + [0.0]), (1, EDGES5 + [-1.0]), (1, EDGES5 + [nan]),
           (1, [nan, 0.0, 1.0, 2.0, 0.5]), (1, [-1.0, 0.0, 1.0, inf, 0.5]), (1, EDGES5), (1, EDGES5 + [0.5, 0.5]), (0, [0.0]), (0, [-0.5]),
           (0, [nan]), (0, [inf]), (0, [0.5, 0.5]), (2, [0.0]), (2, [nan]), (2, []), (3, [1.0]), (3, []), (7, [1.0])]
    for t, vals in bad:
        with pytest.raises(_lib.InvalidArgument):
            e.set_lik_params(t, vals)
        again = _all_outputs(e, prm, tasks)
        assert all(np.array_equal(a, b) for a, b in zip(base, again)), (t, vals)
    assert e.lik_param_count(3) == 0
    with pytest.raises(_lib.InvalidArgument):
        e.lik_grad(3)
    with pytest.raises(_lib.InvalidArgument) as ei:
        e.step_begin(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                     W=prm["W"], kappa=prm["kappa"])
    assert "likelihood-parameter" in str(ei.value)
    again = _all_outputs(e, prm, tasks)
    assert all(np.array_equal(a, b) for a, b in zip(base, again))
    e.lik_grad_enable(False)
    e.step_begin(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                 W=prm["W"], kappa=prm["kappa"])                      # switch off: the split step is what it was
    fin = e.step_finish()
    assert abs(fin["elbo"] - float(base[0])) <= 1e-10 * abs(float(base[0]))
    e.close()


# ------------------------------------------------------------------------------------------------ 5. off means off
@pytest.mark.parametrize("M", [48, 128])
def test_off_means_off(M):
    from hetmogp_amd import _lib
    specs = [GAUSS, ORD5, STUD]
    prm, prob, X, Y = mc.family_case(4800, specs, NS, M, 2, 1)
    a, b = mc.make_engine(prob, X, Y), mc.make_engine(prob, X, Y)

    def _outs(e):                                                                        # ONE evaluation
        out = mc.run(e, prm)
        return [np.array(out[k], copy=True) for k in mc.KEYS]

    for _ in range(3):
        oa = _outs(a)
        ob = _outs(b)
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
    assert all(np.all(b.lik_grad(t) == 0.0) for t in range(3))                          # switch off: zeros
    b.lik_grad_enable(True)
    mc.run(b, prm, group_mask=_lib.GROUP_QU)
    assert all(np.all(b.lik_grad(t) == 0.0) for t in range(3))                          # gated with the hyper-parameters: zeros
    mc.run(b, prm, group_mask=_lib.GROUP_QU | _lib.GROUP_Z)
    assert all(np.all(b.lik_grad(t) == 0.0) for t in range(3))
    mc.run(b, prm)
    assert all(np.any(b.lik_grad(t) != 0.0) for t in range(3))
    on_launches = b.timings()[1]
    b.lik_grad_enable(False)
    b_after_disable = b.graph_stats()
    assert all(np.all(b.lik_grad(t) == 0.0) for t in range(3))
    for _ in range(3):
        ob2 = _outs(b)
        mc.run(a, prm)
    assert all(np.array_equal(x, y) for x, y in zip(ob, ob2))                           # before / after an enable-disable cycle
    assert a.timings()[1] == b.timings()[1], (a.timings()[1], b.timings()[1])           # launch counts per category
    assert on_launches["quadrature"] > b.timings()[1]["quadrature"]
    c = mc.make_engine(prob, X, Y)                                                       # an engine that never heard of the feature
    for _ in range(6):
        mc.run(c, prm)
    for _ in range(3):
        mc.run(b, prm)
    # a never heard of the feature, c neither: the same number of evaluations, the same (captured, replayed)
    assert a.graph_stats() == c.graph_stats() and (a.graph_stats()[0] >= 1) == (M == 48), (a.graph_stats(), c.graph_stats())
    assert c.timings()[1] == b.timings()[1]
    # b, counted from after the disable (the enable and the disable each dropped its graphs): a FRESH engine's figures again --
    # f runs what b ran since then, six evaluations of one key
    f = mc.make_engine(prob, X, Y)
    b0 = b_after_disable
    for _ in range(6):
        mc.run(f, prm)
    got = tuple(x - y for x, y in zip(b.graph_stats(), b0))
    assert got == f.graph_stats(), (got, f.graph_stats())
    a.close(), b.close(), c.close(), f.close()


# ------------------------------------------------------------------------------------------------ 6. facade
def _toy(seed, N=500):
    """The toy of tests/test_ordinal_gpu.py: a Gaussian output and a K = 5 Ordinal output, the binned, noisy version of a correlated
    latent function."""
    rng = np.random.RandomState(seed)
    lat = lambda x: 1.8 * np.sin(2.0 * np.pi * x) + 0.6 * np.cos(5.0 * x)
    edges, sigma = np.array([-1.5, -0.5, 0.5, 1.5]), 0.4
    Xg, Xo = np.sort(rng.rand(N, 1), 0), np.sort(rng.rand(N, 1), 0)
    Yg = 0.8 * lat(Xg) + 0.3 + 0.2 * rng.randn(N, 1)
    label = lambda x: (1 + (lat(x) + sigma * rng.randn(*x.shape) > edges[None, :]).sum(1, keepdims=True)).astype(float)
    Xt = np.sort(rng.rand(300, 1), 0)
    return Xg, Yg, Xo, label(Xo), Xt, label(Xt), edges, sigma


def _model(learn, batch_size=None):
    import hetmogp_amd as H
    Xg, Yg, Xo, Yo, Xt, Yt, edges, sigma = _toy(5)
    likelihood = H.HetLikelihood([H.Gaussian(sigma=1.0, learn_sigma=learn),
                                  H.Ordinal(bin_edges=0.4 * edges, sigma=sigma, learn_edges=learn)])
    Q, M = 2, 12
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.1]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [np.eye(Q, 2)[q][:, None] * 0.9 + 0.1 for q in range(Q)]
    np.random.seed(0)
    return H.HetMOGP(X=[Xg, Xo], Y=[Yg, Yo], Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood,
                     Y_metadata=likelihood.generate_metadata(), W_list=W_list, batch_size=batch_size), likelihood, edges


def test_facade_learns_sigma_and_cuts():
    import hetmogp_amd as H
    final = {}
    for learn in (True, False):
        model, lik, edges = _model(learn)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            H.vem_algorithm(model, stochastic=False, vem_iters=3)
        final[learn] = float(model.log_likelihood()[0, 0])
        if learn:
            learned, lik_learned = model, lik
    print("final ELBO learnable %.4f, fixed %.4f" % (final[True], final[False]))
    assert final[True] > final[False]
    g, o = lik_learned.likelihoods_list
    print("sigma 1.0 -> %.4f (true 0.2); cuts %s -> %s (true %s)" % (g.sigma, 0.4 * edges, o.bin_edges, edges))
    assert np.all(np.diff(o.bin_edges) > 0.0)
    assert abs(np.log(g.sigma) - np.log(0.2)) < abs(np.log(1.0) - np.log(0.2))
    assert len(learned["likelihood.*"]) == 3 and len(learned["likelihood\\.1\\..*"]) == 2
    learned["likelihood.*"].unfix()
    names = [n for n, _ in learned._named_params()]
    assert names[-3:] == ["likelihood.0.sigma", "likelihood.1.edge0", "likelihood.1.gaps"]
    x = learned.optimizer_array.copy()
    before = [np.array(p.values, copy=True) for _, p in learned._named_params()]
    learned.optimizer_array = x
    assert np.allclose(learned.optimizer_array, x, rtol=1e-12, atol=1e-12)
    assert all(np.allclose(a, p.values, rtol=1e-12, atol=1e-14) for a, (_, p) in zip(before, learned._named_params()))
    # predictive follows training: the learned cuts, not the constructor's
    rng = np.random.RandomState(1)
    m, v = rng.randn(50, 1), 0.1 + rng.rand(50, 1)
    mean, var = o.predictive(m, v)
    fresh = H.Ordinal(bin_edges=o.bin_edges, sigma=o.sigma).predictive(m, v)
    start = H.Ordinal(bin_edges=0.4 * edges, sigma=o.sigma).predictive(m, v)
    assert np.array_equal(mean, fresh[0]) and np.array_equal(var, fresh[1]) and not np.array_equal(mean, start[0])
    Xt = np.linspace(0, 1, 40)[:, None]
    pm, pv = learned.predictive([Xt, Xt])
    assert np.all(np.isfinite(pm[1])) and np.all((pm[1] >= 1.0) & (pm[1] <= 5.0))


def test_device_adadelta_moves_sigma():
    model, lik, _ = _model(True, batch_size=64)
    opt = model.device_adadelta(step_rate=0.1, momentum=0.9)
    assert opt is not None and any(p is lik.likelihoods_list[0].learnable_params()[0][1] for p in opt.small)
    it = iter(opt)
    for _ in range(10):
        next(it)
    it.close()
    s = lik.likelihoods_list[0].sigma
    print("sigma after 10 device-Adadelta iterations: %.6f" % s)
    assert np.isfinite(s) and s > 0.0 and s != 1.0
    assert np.all(np.diff(lik.likelihoods_list[1].bin_edges) > 0.0)


def test_sharded_model_refuses_learnable_likelihoods():
    import hetmogp_amd as H
    Xg, Yg, Xo, Yo, _, _, edges, sigma = _toy(5, N=64)
    likelihood = H.HetLikelihood([H.Gaussian(sigma=1.0, learn_sigma=True), H.Ordinal(bin_edges=edges, sigma=sigma)])
    kern_list = H.latent_functions_prior(1, lenghtscale=np.array([0.1]), variance=np.array([1.0]), input_dim=1)
    with pytest.raises(NotImplementedError):
        H.HetMOGP(X=[Xg, Xo], Y=[Yg, Yo], Z=np.linspace(0, 1, 8)[:, None], kern_list=kern_list, likelihood=likelihood,
                  Y_metadata=likelihood.generate_metadata(), distributed=True)


def test_facade_rereads_the_gradient_after_the_switch_to_strict_qf():
    """strict_qf="auto" (the constructor default) in the jitter-ladder regime: the flagged evaluation is repeated through the
    solve-based forms, and the likelihood gradient the model holds is that evaluation's -- the strict engine's, bit for bit --
    not the first one's."""
    import json
    import os
    import hetmogp_amd as H
    from conftest import GOLDEN
    from oracle import svmogp_oracle as so
    g = np.load(os.path.join(GOLDEN, "lad_h_mix_M128_ladder.npz"))
    T, Q, P = int(g["T"]), int(g["Q"]), int(g["P"])
    specs = json.loads(str(g["spec"]))
    assert specs[0][0] == "Gaussian"
    liks = [H.Gaussian(learn_sigma=True, **specs[0][1])] + [getattr(H, n)(**kw) for n, kw in specs[1:]]
    likelihood = H.HetLikelihood(liks)
    kern_list = H.latent_functions_prior(Q, lenghtscale=g["lengthscale"], variance=g["variance"], input_dim=P)
    X, Y = [g["Xall_%d" % t] for t in range(T)], [g["Yall_%d" % t] for t in range(T)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = H.HetMOGP(X, Y, g["Z"][:, :P].copy(), kern_list, likelihood, likelihood.generate_metadata(),
                          W_list=[g["W0"][q][:, None].copy() for q in range(Q)])
        model.q_u_means[...] = g["m_u"]
        model.q_u_chols[...] = g["L_flat"]
        model.Z[...] = g["Z"]
        for q in range(Q):
            model.B_list[q].W[...] = g["W"][q][:, None]
        model.parameters_changed()
    assert model.strict_switches >= 1 and model._strict_now
    got = float(liks[0].learnable_params()[0][1].gradient[0])
    prm, prob, Xc, Yc, bs = so.load_case(g)
    grads = {}
    for strict in (True, False):
        e = mc.make_engine(prob, Xc, Yc, strict_qf=strict)
        e.lik_grad_enable(True)
        mc.run(e, prm, bs)
        grads[strict] = float(e.lik_grad(0)[0])
        e.close()
    print("[lik_grad] facade after the auto switch %.17g, strict engine %.17g, default engine %.17g" % (got, grads[True], grads[False]))
    assert abs(got - grads[True]) <= 1e-12 * abs(grads[True])
    assert got == grads[True] or abs(got - grads[True]) < abs(got - grads[False])
