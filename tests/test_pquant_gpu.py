"""GPU: the predictive cdf, survival function and quantiles of DESIGN 9k -- the kernels of csrc/predq.hip against the 50-digit grid
tests/golden/pqgrid.npz and the float64 restatement tests/pquant_ref.py, their block / wave tails and the independence of rows and
probabilities, the ties to the log-predictive-density kernels, the round trip, the engine path (hmogp_predict_cdf /
hmogp_predict_quantile), its refusals, the current likelihood parameters, and the facade.  Every refusal here is a host-side argument
check that returns before a launch."""
import numpy as np
import pytest

import logpred_ref as lr
import pquant_ref as pq

pytestmark = pytest.mark.gpu
EPS = pq.EPS
TAILS = (1, 63, 64, 65, 257)
NPS = (1, 3, 8)
PROBS8 = np.array([0.025, 0.5, 0.975, 1e-12, 0.2, 1.0 - 1e-7, 0.8, 1e-3])
CONT = tuple(f for f in pq.FAMILIES if f not in pq.DISCRETE)


def _E():
    from hetmogp_amd import engine
    return engine


def _lib():
    from hetmogp_amd import _lib
    return _lib


def _csum(name, col=None):
    """(C_KERNEL + C_ORACLE) of the family, the larger of its two classes (rows outside the grid have no class)."""
    t = [max(a[i] for a in pq.c_sum(name).values()) for i in (0, 1)]
    return max(t) if col is None else t[col]


def _assert_quantiles(name, got, m, v, probs, kw, what):
    """The mixed criterion of pquant_ref on every element that can be judged; the others as the restatement has them."""
    got = np.asarray(got, float)
    assert got.shape == (m.shape[0], len(probs))
    if name in pq.DISCRETE:
        want = pq.quantile(name, m, v, probs, **kw)
        ties = pq.discrete_ties(name, m, v, probs, _csum(name), **kw)
        assert not ties.any() and np.array_equal(got, want, equal_nan=True), (what, np.nonzero(got != want))
        return
    ex = pq.quantile_excess(name, got, m, v, probs, _csum(name), **kw)
    judged = pq.in_range(name, got)
    print("[pquant] %-36s worst excess over the quantile criterion (<= 0 passes): %.3g; judged %d of %d" %
          (what, np.nanmax(np.where(judged, ex, -np.inf)), judged.sum(), judged.size))
    assert (ex[judged] <= 0.0).all(), (what, np.nanmax(ex), np.nonzero(judged & ~(ex <= 0.0)))
    if not judged.all():
        want = pq.quantile(name, m, v, probs, **kw)
        assert pq.same_out_of_range(name, got[~judged], want[~judged]).all(), what


def _assert_cdf(name, y, m, v, kw, c, s, what):
    """Kernel against the float64 restatement on rows that have no 50-digit value: each within its own constant of the true value."""
    rc, rs = pq.cdf_sf(name, y, m, v, **kw)
    S = pq.scale(name, y, m, v, **kw)
    for col, (got, ref) in enumerate(((c, rc), (s, rs))):
        fig = pq.figures(got, ref, S[:, col], ones_exact=False)
        print("[pquant] %-36s worst |kernel - float64| / (2^-52 S R): %s %.3g (bound %g)" % (what, ("cdf", "sf")[col], fig.max(), _csum(name, col)))
        assert (fig <= _csum(name, col)).all(), (what, col, fig.max())


# ------------------------------------------------------------------------------------------------ the grid
def test_grid_both_outputs():
    E = _E()
    seen = set()
    for b in pq.load_grid():
        c, s = E.predictive_cdf_rows(b.name, b.y, b.m, b.v, return_sf=True, **b.kw)
        pq.assert_block(c, s, b, pq.c_kernel(b.name), "kernel %s" % b.tag)
        c1 = E.predictive_cdf_rows(b.name, b.y, b.m, b.v, **b.kw)                 # cdf alone: the sf pointer is NULL
        assert np.array_equal(c1, c, equal_nan=True)
        seen.add(b.name)
    assert seen == set(pq.FAMILIES)


@pytest.mark.parametrize("name", pq.FAMILIES)
def test_grid_quantiles(name):
    """Quantiles on the grid's (m, v): bulk rows, v = 0, f at the clips."""
    E = _E()
    for b in pq.load_grid():
        if b.name != name:
            continue
        ok = np.isfinite(b.m).all(1)
        got = E.predictive_quantile_rows(name, b.m[ok], b.v[ok], PROBS8[:5], **b.kw)
        _assert_quantiles(name, got, b.m[ok], b.v[ok], PROBS8[:5], b.kw, "grid %s" % b.tag)
        if name in CONT:
            assert not np.isnan(got).any(), b.tag                                 # nobody ran out of evaluations


# ------------------------------------------------------------------------------------------------ tails, independence
@pytest.mark.parametrize("name,kw", [("Exponential", {}), ("Ordinal", {"K": 4, "sigma": 1.0}), ("Weibull", {})],
                         ids=lambda a: a if isinstance(a, str) else "")
def test_tails_and_independence(name, kw):
    """N = 1, 63, 64, 65, 257 rows and nP = 1, 3, 8 probabilities in one call: the block tail of the lane kernels (256), four rows per
    block of the wave kernels; a row's result depends neither on its neighbours nor on the other probabilities of the call."""
    E = _E()
    y, m, v = pq.bulk_rows(name, max(TAILS), 4343, **kw)
    if name == "Weibull":
        m[:, 1] = np.clip(m[:, 1], -1.0, 3.0)                     # (shapes whose quantiles stay inside the doubles' range)
    full = E.predictive_quantile_rows(name, m, v, PROBS8, **kw)
    _assert_quantiles(name, full, m, v, PROBS8, kw, "%s N = 257, nP = 8" % name)
    cf, sf = E.predictive_cdf_rows(name, y, m, v, return_sf=True, **kw)
    _assert_cdf(name, y, m, v, kw, cf, sf, "%s N = 257" % name)
    for n in TAILS:
        c, s = E.predictive_cdf_rows(name, y[:n], m[:n], v[:n], return_sf=True, **kw)
        assert np.array_equal(c, cf[:n]) and np.array_equal(s, sf[:n]), (name, n)
        for k in NPS:
            q = E.predictive_quantile_rows(name, m[:n], v[:n], PROBS8[:k], **kw)
            assert q.shape == (n, k) and np.array_equal(q, full[:n, :k], equal_nan=True), (name, n, k)
    q = E.predictive_quantile_rows(name, m[100:165][::-1], v[100:165][::-1], PROBS8[::-1], **kw)    # other neighbours, other order
    assert np.array_equal(q, full[100:165][::-1, ::-1], equal_nan=True)
    bad = E.predictive_quantile_rows(name, m[:5], v[:5], [0.5, 0.0, 1.0, -0.5, np.nan, 2.0], **kw)  # a p outside (0, 1): NaN column
    assert np.array_equal(bad[:, 0], full[:5, 1]) and np.isnan(bad[:, 1:]).all()
    many = E.predictive_quantile_rows(name, m[:9], v[:9], np.linspace(0.05, 0.95, 11), **kw)        # more than 8: several calls
    assert many.shape == (9, 11) and (np.diff(many, axis=1) >= 0.0).all()


@pytest.mark.parametrize("name", ("HetGaussian", "Exponential", "Weibull"))
def test_ten_nodes(name):
    E = _E()
    y, m, v = pq.bulk_rows(name, 65, 77)
    m[:, -1] = np.clip(m[:, -1], -1.0, 3.0)
    c, s = E.predictive_cdf_rows(name, y, m, v, gh_T=10, return_sf=True)
    rc, rs = pq.cdf_sf(name, y, m, v, gh_T=10)
    S = pq.scale(name, y, m, v, gh_T=10)
    assert (pq.figures(c, rc, S[:, 0], False) <= _csum(name, 0)).all() and (pq.figures(s, rs, S[:, 1], False) <= _csum(name, 1)).all()
    q = E.predictive_quantile_rows(name, m, v, PROBS8[:3], gh_T=10)
    ex = pq.quantile_excess(name, q, m, v, PROBS8[:3], _csum(name), gh_T=10)
    assert (ex <= 0.0).all(), (name, ex.max())


# ------------------------------------------------------------------------------------------------ ties to kernels that exist
def test_weibull_log_sf_is_the_lpd_of_a_censored_row():
    """The nodes are the same and a censored row scores its survival: log sf(y) = lpd(y, delta = 0), each kernel within its own constant."""
    E = _E()
    y, m, v = pq.bulk_rows("Weibull", 200, 91)
    keep = np.isfinite(y)                                          # (a time drawn at a shape next to its clip of 1e-3 overflows)
    y, m, v = y[keep], m[keep], v[keep]
    _, sf = E.predictive_cdf_rows("Weibull", y, m, v, return_sf=True)
    Y = np.stack([y, np.zeros_like(y)], 1)
    lpd = E.log_predictive_density_rows("Weibull", Y, m, v)
    S_sf = pq.scale("Weibull", y, m, v)[:, 1]
    S_lpd = lr.lpd_scale("Weibull", Y, m, v)
    bound = EPS * (pq.c_kernel("Weibull")[pq.BULK][1] * S_sf + lr.c_kernel("Weibull")[lr.BULK][0] * S_lpd)
    ok = sf > 2.0 ** -1022
    assert ok.mean() > 0.9
    d = np.abs(np.log(sf[ok]) - lpd[ok])
    print("[pquant] Weibull log sf vs lpd(delta = 0): worst |difference| / bound %.3g" % (d / bound[ok]).max())
    assert (d <= bound[ok]).all()


def test_bernoulli_sf_at_zero_is_exp_lpd_of_one():
    E = _E()
    _, m, v = pq.bulk_rows("Bernoulli", 200, 92)
    y0, y1 = np.zeros(200), np.ones(200)
    c, s = E.predictive_cdf_rows("Bernoulli", y0, m, v, return_sf=True)
    l1, l0 = E.log_predictive_density_rows("Bernoulli", y1, m, v), E.log_predictive_density_rows("Bernoulli", y0, m, v)
    for got, lpd, yy in ((s, l1, y1), (c, l0, y0)):
        S = lr.lpd_scale("Bernoulli", yy, m, v)
        bound = EPS * (pq.c_kernel("Bernoulli")[pq.BULK][1] + lr.c_kernel("Bernoulli")[lr.BULK][0] * S)
        assert (np.abs(got - np.exp(lpd)) <= bound * got).all()


def test_gaussian_quantiles_are_the_normal_ones():
    E = _E()
    _, m, v = pq.bulk_rows("Gaussian", 200, 93, sigma=0.5)
    probs = [0.025, 0.5, 0.975]
    for sigma, s in ((0.5, 0.5), (1.7, 1.7), (None, 0.5), (-2.0, 0.5)):
        got = E.predictive_quantile_rows("Gaussian", m, v, probs, sigma=sigma)
        _assert_quantiles("Gaussian", got, m, v, probs, {"sigma": sigma}, "Gaussian sigma = %s" % sigma)
        want = m + np.array([-1.959963984540054, 0.0, 1.959963984540054])[None, :] * np.sqrt(s * s + v)
        assert (np.abs(got - want) <= 8.0 * EPS * (np.abs(m) + 2.0 * np.sqrt(s * s + v))).all(), sigma


@pytest.mark.parametrize("name", CONT)
def test_round_trip(name):
    """cdf(quantile(p)) returns p (sf for p > 1/2): the criterion puts p between F at the 4-ulp neighbours of the quantile (+- tol), and
    the kernel's own value at the quantile lies within its constant of F there."""
    E = _E()
    kw = dict(pq.BULK_KW.get(name, {}))
    _, m, v = pq.bulk_rows(name, 128, 94, **kw)
    m[:, -1] = np.clip(m[:, -1], -1.0, 3.0)
    if name == "Weibull":
        v[:, 1] = np.minimum(v[:, 1], 0.25)
    probs = PROBS8[[0, 1, 2, 5, 7]]
    q = E.predictive_quantile_rows(name, m, v, probs, **kw)
    ok = pq.in_range(name, q).all(1)                               # (Weibull: a shape node at its clip of 1e-3 sends a tail quantile out of range)
    assert ok.mean() > 0.9
    q, m, v = q[ok], m[ok], v[ok]
    for j, p in enumerate(probs):
        col = 1 if p > 0.5 else 0
        tq = 1.0 - p if col else p
        back = E.predictive_cdf_rows(name, q[:, j], m, v, return_sf=True, **kw)[col]
        if name in pq.LOGVAR:
            lo, hi = np.exp(pq.ulps(np.log(q[:, j]), -4)), np.exp(pq.ulps(np.log(q[:, j]), 4))
        else:
            lo, hi = pq.ulps(q[:, j], -4), pq.ulps(q[:, j], 4)
        F = [pq.cdf_sf(name, t, m, v, **kw)[col] for t in (lo, hi)]
        tol = _csum(name, col) * EPS * pq.scale(name, q[:, j], m, v, **kw)[:, col] * tq
        assert (np.abs(back - tq) <= np.abs(F[1] - F[0]) + 2.0 * tol).all(), (name, p, (np.abs(back - tq) / tol).max())


# ------------------------------------------------------------------------------------------------ the engine path
SPECS = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Bernoulli", {}), ("Exponential", {}), ("Ordinal", {"K": 4, "sigma": 1.0}),
         ("Weibull", {})]
EPROBS = [0.025, 0.5, 0.975]


def _engine(specs, M, N=300, Nnew=129, **ekw):
    from hetmogp_amd.engine import Engine
    from hetmogp_amd.synthetic import make_case
    prm, X, Y = make_case(specs, [N] * len(specs), M=M, Q=2, P=1, seed=5)
    _, Xn, Yn = make_case(specs, [Nnew] * len(specs), M=M, Q=2, P=1, seed=6)
    e = Engine(specs, 2, M, 1, **ekw)
    e.set_data(X, Y)
    return e, prm, Xn, Yn


def _cols(specs, t):
    d0 = sum(lr.dim_f(n, **k) for n, k in specs[:t])
    return list(range(d0, d0 + lr.dim_f(specs[t][0], **specs[t][1])))


def _y1(name, Y):
    Y = np.asarray(Y, float)
    return Y[:, 0] if Y.ndim == 2 else Y


@pytest.mark.parametrize("M,ekw", [(128, {}), (16, {}), (128, {"chunk_rows": 48}), (128, {"strict_qf": True})],
                         ids=["regular", "small-model", "chunks-of-48", "strict"])
def test_engine_path_is_the_building_block_on_its_own_qf(M, ekw):
    E = _E()
    e, prm, Xn, Yn = _engine(SPECS, M, **ekw)
    e.elbo_grad(**prm)
    for t, (name, kw) in enumerate(SPECS):
        y = _y1(name, Yn[t])
        cdf, sf = e.predict_cdf(t, Xn[t], y)
        q = e.predict_quantile(t, Xn[t], EPROBS)
        m, v = e.predict_f(Xn[t])
        c = _cols(SPECS, t)
        a, b = E.predictive_cdf_rows(name, y, m[:, c], np.abs(v[:, c]), return_sf=True, **kw)
        qq = E.predictive_quantile_rows(name, m[:, c], np.abs(v[:, c]), EPROBS, **kw)
        assert cdf.shape == (129,) and q.shape == (129, 3) and np.isfinite(cdf).all() and np.isfinite(q).all()
        assert np.array_equal(cdf, a) and np.array_equal(sf, b) and np.array_equal(q, qq), name
    e.close()


def test_engine_path_refusals():
    L = _lib()
    specs = SPECS[:1] + [("Gamma", {})] + SPECS[4:]
    e, prm, Xn, Yn = _engine(specs, 16)
    y0 = _y1("Gaussian", Yn[0])

    def valid():
        c, s = e.predict_cdf(0, Xn[0], y0)
        q = e.predict_quantile(3, Xn[3], EPROBS)
        assert np.isfinite(c).all() and np.isfinite(s).all() and np.isfinite(q).all()

    for call in (lambda: e.predict_cdf(0, Xn[0], y0), lambda: e.predict_quantile(0, Xn[0], EPROBS)):
        with pytest.raises(L.HetMOGPError) as ei:
            call()
        assert ei.value.code == L.E_STATE
    e.elbo_grad(**prm)
    valid()
    p = np.array(EPROBS)
    P = lambda a: a.ctypes.data_as(L.c_double_p)   # noqa: E731
    out = np.zeros((129, 8))
    X0 = np.ascontiguousarray(Xn[0], float)
    refusals = [
        lambda: e.predict_cdf(-1, Xn[0], y0), lambda: e.predict_cdf(len(specs), Xn[0], y0),            # task index
        lambda: e.predict_quantile(-1, Xn[0], EPROBS), lambda: e.predict_quantile(len(specs), Xn[0], EPROBS),
        lambda: e.predict_cdf(1, Xn[1], _y1("Gamma", Yn[1])), lambda: e.predict_quantile(1, Xn[1], EPROBS),   # Gamma: no incomplete gamma function
        lambda: e.predict_cdf(0, Xn[0], y0, gh_T=5), lambda: e.predict_quantile(0, Xn[0], EPROBS, gh_T=30),
        lambda: e.predict_cdf(2, Xn[2], _y1("Ordinal", Yn[2]) + 4.0),                                        # a label outside 1 .. K
        lambda: e.predict_cdf(2, Xn[2], _y1("Ordinal", Yn[2]) + 0.5),
        lambda: L.check(L.lib.hmogp_predict_quantile(e._h, 0, P(X0), 129, 0, P(p), 0, P(out)), e._h),        # nP outside 1 .. 8
        lambda: L.check(L.lib.hmogp_predict_quantile(e._h, 0, P(X0), 129, 9, P(out), 0, P(out)), e._h),
        lambda: L.check(L.lib.hmogp_predict_quantile(e._h, 0, None, 129, 3, P(p), 0, P(out)), e._h),         # NULL pointers with N > 0
        lambda: L.check(L.lib.hmogp_predict_quantile(e._h, 0, P(X0), 129, 3, None, 0, P(out)), e._h),
        lambda: L.check(L.lib.hmogp_predict_quantile(e._h, 0, P(X0), 129, 3, P(p), 0, None), e._h),
        lambda: L.check(L.lib.hmogp_predict_cdf(e._h, 0, None, P(y0), 129, 0, P(out), P(out)), e._h),
        lambda: L.check(L.lib.hmogp_predict_cdf(e._h, 0, P(X0), None, 129, 0, P(out), P(out)), e._h),
        lambda: e.predict_cdf(0, Xn[0], y0[:100]),                                                           # rows of X and y differ
    ]
    for r in refusals:
        with pytest.raises(L.InvalidArgument):
            r()
        valid()                                                                                              # a valid call after each
    with pytest.raises(L.InvalidArgument, match="incomplete gamma"):
        e.predict_cdf(1, Xn[1], _y1("Gamma", Yn[1]))
    e.close()


def test_engine_path_uses_the_current_likelihood_parameters():
    E = _E()
    old = [("Gaussian", {"sigma": 0.5}), ("Ordinal", {"K": 4, "sigma": 1.0})]
    new = [("Gaussian", {"sigma": 0.8}), ("Ordinal", {"bin_edges": [-1.2, 0.1, 0.9], "sigma": 0.6})]
    values = [[0.8], [-1.2, 0.1, 0.9, 0.6]]
    e, prm, Xn, Yn = _engine(old, 16)
    e.elbo_grad(**prm)
    for t in range(2):
        y = _y1(old[t][0], Yn[t])
        before = e.predict_cdf(t, Xn[t], y), e.predict_quantile(t, Xn[t], EPROBS)
        e.set_lik_params(t, values[t])
        after = e.predict_cdf(t, Xn[t], y), e.predict_quantile(t, Xn[t], EPROBS)
        m, v = e.predict_f(Xn[t])
        c = _cols(old, t)
        for spec, (cs, q) in ((new[t], after), (old[t], before)):
            a, b = E.predictive_cdf_rows(spec[0], y, m[:, c], np.abs(v[:, c]), return_sf=True, **spec[1])
            qq = E.predictive_quantile_rows(spec[0], m[:, c], np.abs(v[:, c]), EPROBS, **spec[1])
            assert np.array_equal(cs[0], a) and np.array_equal(cs[1], b) and np.array_equal(q, qq), spec
        assert np.abs(after[0][0] - before[0][0]).max() > 1e-3, old[t][0]
    e.close()


# ------------------------------------------------------------------------------------------------ the facade
def _facade(liks, Ys, M=12):
    import hetmogp_amd as H
    likelihood = H.HetLikelihood(liks)
    rng = np.random.RandomState(1)
    X = [np.sort(rng.rand(len(y), 1), 0) for y in Ys]
    Q = 2
    Df = likelihood.num_output_functions(likelihood.generate_metadata())
    kern_list = H.latent_functions_prior(Q, lenghtscale=np.array([0.1, 0.15]), variance=np.array([1.0, 1.0]), input_dim=1)
    W_list = [0.3 * rng.randn(Df, 1) for _ in range(Q)]
    np.random.seed(0)
    model = H.SVMOGP(X=X, Y=Ys, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood,
                     Y_metadata=likelihood.generate_metadata(), W_list=W_list)
    return model, X


def test_facade():
    import hetmogp_amd as H
    E = _E()
    rng = np.random.RandomState(2)
    Ns = (80, 70, 60, 50)
    t3 = rng.exponential(1.0, Ns[2]) + 0.05
    Ys = [rng.randn(Ns[0], 1), 0.5 * rng.randn(Ns[1], 1), np.stack([t3, (rng.rand(Ns[2]) < 0.7).astype(float)], 1),
          rng.gamma(2.0, 1.0, (Ns[3], 1)) + 1e-3]
    model, X = _facade([H.Gaussian(sigma=0.7, learn_sigma=True), H.HetGaussian(), H.Weibull(), H.Gamma()], Ys)
    Xt = [x[:40] for x in X]
    Yt = [Ys[0][:40, 0], Ys[1][:40, 0], Ys[2][:40, 0], Ys[3][:40, 0]]
    q = model.predict_quantiles(Xt, tasks=[0, 1, 2])                               # GPy's defaults: 2.5 % and 97.5 %
    assert [a.shape for a in q] == [(40, 2)] * 3 and all(np.isfinite(a).all() and (a[:, 0] < a[:, 1]).all() for a in q)
    q3 = model.predict_quantiles(Xt, quantiles=(2.5, 50.0, 97.5), tasks=[2, 0])
    assert np.array_equal(q3[1][:, [0, 2]], q[0]) and np.array_equal(q3[0][:, [0, 2]], q[2]) and (q3[0] > 0.0).all()
    for call in (lambda: model.predict_quantiles(Xt), lambda: model.predict_quantiles(Xt, tasks=None),
                 lambda: model.predictive_cdf(Xt, Yt), lambda: model.predict_quantiles(Xt, tasks=[0, 3], route="reference")):
        with pytest.raises(NotImplementedError, match="Gamma.*incomplete gamma"):
            call()
    # cdf and sf; the survival curve of the Weibull task
    cs = model.predictive_cdf(Xt, Yt, return_sf=True, tasks=[0, 1, 2])
    assert all(c.shape == (40,) and s.shape == (40,) and (np.abs(c + s - 1.0) <= 64.0 * EPS).all() for c, s in cs)
    c_only = model.predictive_cdf(Xt, Yt, tasks=[1])
    assert np.array_equal(c_only[0], cs[1][0])
    times = np.array([0.0, 0.05, 0.3, 1.0, 2.5, 10.0, 1e3])
    S = model.survival_function(2, Xt[2], times)
    assert S.shape == (40, 7) and (S[:, 0] == 1.0).all() and (np.diff(S, axis=1) <= 0.0).all() and (S[:, -1] < S[:, 1]).all()
    for k, tk in enumerate(times):
        col = model.predictive_cdf([None, None, Xt[2]], [None, None, np.full(40, tk)], return_sf=True, tasks=[2])[0][1]
        assert np.array_equal(col, S[:, k]), tk
    med = model.predict_quantiles(Xt, quantiles=(50.0,), tasks=[2])[0][:, 0]        # the median time to event: S(median) = 1/2
    Smed = np.array([model.survival_function(2, Xt[2][i:i + 1], med[i:i + 1])[0, 0] for i in range(0, 40, 8)])
    assert (np.abs(Smed - 0.5) <= 1e-12).all()
    with pytest.raises(ValueError):
        model.survival_function(0, Xt[0], times)
    # the reference route agrees with the building block on _raw_predict_f's q(f), with the likelihoods' current kwargs
    ref_q = model.predict_quantiles(Xt, quantiles=(2.5, 97.5), tasks=[0, 1, 2], route="reference")
    ref_c = model.predictive_cdf(Xt, Yt, return_sf=True, tasks=[0, 1, 2], route="reference")
    for i, t in enumerate((0, 1, 2)):
        l = model.likelihood.likelihoods_list[t]
        m, v = model._predict_route(Xt[t], t, "reference")
        assert np.array_equal(ref_q[i], E.predictive_quantile_rows(l.name, m, v, [0.025, 0.975], **l.kwargs()))
        a, b = E.predictive_cdf_rows(l.name, Yt[t], m, v, return_sf=True, **l.kwargs())
        assert np.array_equal(ref_c[i][0], a) and np.array_equal(ref_c[i][1], b)
    # the likelihood-level entry points
    lik = model.likelihood
    m_F = [model._predict_route(Xt[t], t, "default")[0] for t in range(4)]
    v_F = [model._predict_route(Xt[t], t, "default")[1] for t in range(4)]
    ql = lik.predictive_quantiles(m_F, v_F, [0.025, 0.975], tasks=[0, 1, 2])
    cl = lik.predictive_cdf(Yt, m_F, v_F, return_sf=True, tasks=[0, 1, 2])
    for i in range(3):
        assert np.array_equal(ql[i], q[i]) and np.array_equal(cl[i][0], cs[i][0]) and np.array_equal(cl[i][1], cs[i][1])
    with pytest.raises(NotImplementedError, match="Gamma"):
        lik.predictive_quantiles(m_F, v_F, [0.5])
    with pytest.raises(NotImplementedError, match="Gamma"):
        lik.likelihoods_list[3].predictive_cdf(Yt[3], m_F[3], v_F[3])


# ------------------------------------------------------------------------------------------------ refusals of the building block
def test_building_block_refusals():
    E, L = _E(), _lib()
    y, m, v = pq.bulk_rows("Ordinal", 9, 31, K=4, sigma=1.0)
    kw = {"K": 4, "sigma": 1.0}
    ok = []
    for bad in (dict(gh_T=5), dict(gh_T=30)):
        with pytest.raises(L.InvalidArgument):
            E.predictive_cdf_rows("Ordinal", y, m, v, **bad, **kw)
        with pytest.raises(L.InvalidArgument):
            E.predictive_quantile_rows("Ordinal", m, v, [0.5], **bad, **kw)
        ok.append(E.predictive_cdf_rows("Ordinal", y, m, v, **kw))
    for ybad in (y + 4.0, y - 0.5, np.where(np.arange(9) == 3, np.nan, y)):
        with pytest.raises(L.InvalidArgument):
            E.predictive_cdf_rows("Ordinal", ybad, m, v, **kw)
        ok.append(E.predictive_quantile_rows("Ordinal", m, v, [0.5], **kw))
    for name in pq.REFUSED:
        kw2 = {"K": 3} if name in ("Categorical", "Dirichlet") else {}
        J = lr.dim_f(name, **kw2)
        with pytest.raises(L.InvalidArgument, match="incomplete|no order|multivariate"):
            E.predictive_cdf_rows(name, np.full(4, 0.5), np.zeros((4, J)), np.ones((4, J)), **kw2)
        with pytest.raises(L.InvalidArgument, match="incomplete|no order|multivariate"):
            E.predictive_quantile_rows(name, np.zeros((4, J)), np.ones((4, J)), [0.5], **kw2)
        ok.append(E.predictive_cdf_rows("Gaussian", np.zeros(4), np.zeros((4, 1)), np.ones((4, 1)), sigma=0.5))
    assert all(np.isfinite(a).all() for a in ok)
    assert E.predictive_cdf_rows("Gaussian", np.zeros(0), np.zeros((0, 1)), np.zeros((0, 1))).shape == (0,)
