"""GPU: the joint posterior at new inputs (`hmogp_predict_f_joint` / `hmogp_sample_f_joint`) against the 50-digit grid
tests/golden/jointgrid.npz and the restatements of tests/joint_ref.py -- mean and covariance entry by entry in the default and the strict
mode on the small-model and the regular path, exact symmetry, agreement with predict_f, independence of rows and functions, the factor,
the draws against the returned factor and the restated generator, a singular case, one statistical check, the refusals, the facade.

Criterion (joint_ref's docstring): |got - R| <= C 2^-52 scale, C = max(16, 4 C_ORACLE): 16 for the mean, 512 for the covariance (C_ORACLE 128 is
GPy's cancelling order of the squared distance, which the covariance's scale does not fold in).  Measured on the MI355X, 2026-10-20: mean
0.163, covariance 119.3 (s_N129, where the float64 restatement has 119.3 too; against the restatement itself the device stays within 2.9).
Factor: |L L^T - (cov + jitter I)| <= 16 n 2^-52 max diag (LAPACK 0.786, device 0.786).  Draws: (C_Z + n) 2^-52 sum |L| |z| per entry (worst
entry 0.127 of it).  Every case and figure: DESIGN 9r."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import joint_ref as jr            # noqa: E402

pytestmark = pytest.mark.gpu

GRID = jr.load_grid()
NAMES = [c["name"] for c in jr.CASES]
MODES = [False, True]
SEED, DRAWS = 5, 8
_CACHE = {}


def engine_for(prm, case, strict, P=None):
    from hetmogp_amd.engine import Engine
    X, Y = jr.train_data(dict(case, P=P or case["P"]))
    e = Engine(jr.SPECS, prm["variance"].shape[0], prm["Z"].shape[0], P or case["P"], device=0, strict_qf=strict)
    e.set_data(X, Y)
    out = e.elbo_grad(**prm)
    assert all(r == -1 for r in out["rungs"])          # K_uu of the designed cases factorises without jitter
    return e


def result(name, strict):
    """Everything the tests below share for one (case, mode): computed once, left unchanged."""
    key = (name, strict)
    if key not in _CACHE:
        g = GRID[name]
        d = list(g["case"]["functions"])
        e = engine_for(g["prm"], g["case"], strict)
        mean, cov = e.predict_f_joint(g["Xnew"], d)
        n = mean.size
        m, v = e.predict_f(g["Xnew"])
        F, info = e.sample_f_joint(g["Xnew"], d, size=DRAWS, seed=SEED, return_factor=True)
        _CACHE[key] = dict(engine=e, mean=mean, cov=cov.reshape(n, n), cov4=cov, m=m, v=v, F=F.reshape(DRAWS, n), info=info, d=d, n=n)
    return _CACHE[key]


def ids(strict):
    return "strict" if strict else "default"


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_mean_and_cov_against_the_grid(name, strict):
    r = result(name, strict)
    rm, rc = jr.case_ratios(GRID[name], r["mean"], r["cov"])
    print("%s %s: mean %.3f (C %g), cov %.3f (C %g)" % (name, ids(strict), rm, jr.c_kernel("mean"), rc, jr.c_kernel("cov")))
    assert rm <= jr.c_kernel("mean") and rc <= jr.c_kernel("cov")


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_cov_is_exactly_symmetric(name, strict):
    cov = result(name, strict)["cov"]
    assert np.all(np.isfinite(cov)) and np.array_equal(cov, cov.T)


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_agreement_with_predict_f(name, strict):
    """The mean is predict_f's m, the diagonal predict_f's v before its abs: each within the sum of the two constants of the other, and
    predict_f's own values within the criterion of the grid."""
    r, g = result(name, strict), GRID[name]
    d, n = r["d"], r["n"]
    pm, pv = r["m"][:, d].T.reshape(-1), r["v"][:, d].T.reshape(-1)
    diag = np.arange(n)
    assert np.array_equal(g["ri"][:n] if n > jr.FULL_MAX else g["ri"][diag * n + diag], diag)
    k = diag if n > jr.FULL_MAX else diag * n + diag
    R, Sc = g["cov"][k], g["cov_scale"][k]
    assert np.max(jr.ratios(r["mean"].reshape(-1), pm, g["mean_scale"])) <= 2.0 * jr.c_kernel("mean")
    assert np.max(jr.ratios(np.diag(r["cov"]), pv, Sc)) <= 2.0 * jr.c_kernel("cov")
    assert np.max(jr.ratios(pm, g["mean"], g["mean_scale"])) <= jr.c_kernel("mean")
    assert np.max(jr.ratios(pv, R, Sc)) <= jr.c_kernel("cov")
    assert np.max(jr.ratios(np.diag(r["cov"]), R, Sc)) <= jr.c_kernel("cov")


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", ["s_N64", "s_N129", "r_N64", "r_N65"])
def test_row_and_function_independence(name, strict):
    """An entry depends on its own two rows and two functions only: sub-lists of functions (in another order too) and subsets of rows give
    the same bits."""
    r, g = result(name, strict), GRID[name]
    e, d, cov4 = r["engine"], r["d"], r["cov4"]
    N = g["Xnew"].shape[0]
    sub = [len(d) - 1, 0]                                   # positions in d: a sub-list, reversed
    m2, c2 = e.predict_f_joint(g["Xnew"], [d[j] for j in sub])
    assert np.array_equal(c2, cov4[sub][:, :, sub]) and np.array_equal(m2, r["mean"][sub])
    # 22 .. 44 rows in their order: another tile count.  (Which triangle of G_q an entry is read from follows the ORDER of its two rows, so a
    # permutation of the rows may move last bits; a subset does not.)
    rows = np.unique(np.concatenate([np.arange(0, N, 3), [N - 1]]))
    m3, c3 = e.predict_f_joint(g["Xnew"][rows], d)
    assert np.array_equal(c3, cov4[:, rows][:, :, :, rows])


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_the_factor(name, strict):
    r = result(name, strict)
    L, jit, rung, cov = r["info"]["L"], r["info"]["jitter"], r["info"]["rung"], r["cov"]
    assert np.array_equal(L, np.tril(L)) and np.all(np.isfinite(L)) and np.all(np.diag(L) > 0)
    assert np.array_equal(r["info"]["mean"], r["mean"])
    be = jr.chol_backward(cov, L, jit)
    lapack = jr.chol_backward(cov, *jr.jitchol(cov)[:2])
    print("%s %s: rung %d jitter %.3e backward error %.3f (LAPACK %.3f) n eps max diag" % (name, ids(strict), rung, jit, be, lapack))
    assert lapack <= jr.C_CHOL_LAPACK and be <= jr.C_CHOL_KERNEL
    want = 0.0 if rung < 0 else np.mean(np.diag(cov)) * 1e-6 * 10.0 ** rung
    assert -1 <= rung <= 4 and abs(jit - want) <= 4.0 * cov.shape[0] * jr.EPS * want      # (mean(diag) is a sum of n terms in another order)
    if np.min(np.linalg.eigvalsh(cov)) > 1e-9 * np.max(np.diag(cov)):          # a well-conditioned case: no jitter
        assert rung == -1 and jit == 0.0


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_the_draws(name, strict):
    """F[s] - mean against L z_s, L the returned factor and z the restated generator's; seeds, and the number of draws."""
    r, g = result(name, strict), GRID[name]
    e, d, n, L = r["engine"], r["d"], r["n"], r["info"]["L"]
    z = jr.normals(SEED, n, DRAWS)
    ref = np.stack([L @ zs for zs in z])
    bound = (jr.C_Z + n) * jr.EPS * (np.abs(z) @ np.abs(L).T)
    got = r["F"] - r["mean"].reshape(1, -1)
    # (F is mean + sum: the subtraction above adds at most an ulp of |F| <= |mean| + sum |L| |z|)
    slack = 2.0 * jr.EPS * np.abs(r["mean"]).reshape(1, -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("%s %s: worst draw ratio %.3f of the bound" % (name, ids(strict), np.nanmax(np.abs(got - ref) / (bound + slack))))
    assert np.all(np.abs(got - ref) <= bound + slack)
    for S in (1, 3, 8):
        FS = e.sample_f_joint(g["Xnew"], d, size=S, seed=SEED).reshape(S, n)
        assert np.array_equal(FS, r["F"][:S])               # the same seed gives the same bits; draw s does not depend on S
    other = e.sample_f_joint(g["Xnew"], d, size=3, seed=SEED + 1).reshape(3, n)
    assert not np.array_equal(other, r["F"][:3])


@pytest.mark.parametrize("strict", MODES, ids=ids)
def test_singular_case(strict):
    prm, Xnew, d = jr.singular_case()
    e = engine_for(prm, jr.CASE_BY_NAME["s_N64"], strict)
    mean, cov = e.predict_f_joint(Xnew, d)
    F, info = e.sample_f_joint(Xnew, d, size=jr.SINGULAR_DRAWS, seed=jr.SINGULAR_SEED, return_factor=True)
    assert info["rung"] >= 0 and info["jitter"] > 0.0
    assert all(np.all(np.isfinite(a)) for a in (mean, cov, F, info["L"]))
    gap = max(np.max(np.abs(F[:, :, a] - F[:, :, b])) for a, b in jr.SINGULAR_TWINS)
    print("rung %d jitter %.3e twin gap %.3e bound %.3e" % (info["rung"], info["jitter"], gap, 8.0 * np.sqrt(2.0 * info["jitter"])))
    assert gap <= 8.0 * np.sqrt(2.0 * info["jitter"])
    e.close()


def test_draws_follow_the_law():
    """n = 8, S = 4096: per-coordinate means and every pairwise second moment against (mean, cov), exact laws (joint_ref.stat_zscores),
    overall false-alarm rate 1e-6."""
    prm, Xnew, d = jr.stat_case()
    e = engine_for(prm, jr.CASE_BY_NAME["s_N64"], False)
    F, info = e.sample_f_joint(Xnew, d, size=jr.STAT_DRAWS, seed=jr.STAT_SEED, return_factor=True)
    mean, cov = e.predict_f_joint(Xnew, d)
    n = mean.size
    assert n == 8 and info["rung"] == -1
    zm, zc = jr.stat_zscores(F.reshape(jr.STAT_DRAWS, n), mean.reshape(-1), cov.reshape(n, n))
    t = jr.stat_threshold(n)
    print("max |z|: means %.2f, second moments %.2f, threshold %.2f" % (zm, zc, t))
    assert zm <= t and zc <= t
    e.close()


def test_refusals():
    """Every refusal is followed by a valid call on the same engine."""
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine
    case = jr.CASE_BY_NAME["s_N64"]
    prm, Xnew = jr.make_params(case)
    Xnew = Xnew[:5]
    X, Y = jr.train_data(case)
    e = Engine(jr.SPECS, case["Q"], case["M"], case["P"], device=0)
    e.set_data(X, Y)
    with pytest.raises(_lib.HetMOGPError) as ei:            # before the first evaluation
        e.predict_f_joint(Xnew, [0])
    assert ei.value.code == _lib.E_STATE
    with pytest.raises(_lib.HetMOGPError) as ei:
        e.sample_f_joint(Xnew, [0], size=0)
    assert ei.value.code == _lib.E_STATE
    e.elbo_grad(**prm)
    good = e.predict_f_joint(Xnew, [0, 3])

    def still_fine():
        m, c = e.predict_f_joint(Xnew, [0, 3])
        assert np.array_equal(m, good[0]) and np.array_equal(c, good[1])
        assert np.all(np.isfinite(e.sample_f_joint(Xnew, [0, 3], size=2, seed=1)))

    big = np.zeros((jr.JOINT_MAXDIM // 2 + 1, case["P"]))
    for bad in (dict(functions=[]), dict(functions=[4]), dict(functions=[-1]), dict(functions=[1, 1]), dict(functions=[0, 2, 0])):
        with pytest.raises(_lib.InvalidArgument):
            e.predict_f_joint(Xnew, **bad)
        still_fine()
        with pytest.raises(_lib.InvalidArgument):
            e.sample_f_joint(Xnew, size=2, **bad)
        still_fine()
    with pytest.raises(_lib.InvalidArgument, match="HMOGP_JOINT_MAXDIM"):
        e.predict_f_joint(big, [0, 1])                      # n = 8194
    still_fine()
    with pytest.raises(_lib.InvalidArgument, match="HMOGP_JOINT_MAXDIM"):
        e.sample_f_joint(big, [0, 1], size=1)
    still_fine()
    for S in (0, -3):
        with pytest.raises(_lib.InvalidArgument, match="S must be"):
            e.sample_f_joint(Xnew, [0], size=S)
        still_fine()
    import ctypes as C
    dd = np.zeros(1, dtype=np.int32)
    dp, xp = dd.ctypes.data_as(_lib.c_int32_p), Xnew.ctypes.data_as(_lib.c_double_p)
    buf = np.zeros(25)
    bp = buf.ctypes.data_as(_lib.c_double_p)
    h = e._h
    assert _lib.lib.hmogp_predict_f_joint(h, None, 5, 1, dp, bp, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_predict_f_joint(h, xp, 5, 1, None, bp, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_predict_f_joint(h, xp, 5, 1, dp, None, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_predict_f_joint(h, xp, 5, 1, dp, bp, None) == _lib.E_INVALID
    assert _lib.lib.hmogp_predict_f_joint(h, xp, -1, 1, dp, bp, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_sample_f_joint(h, xp, 5, 1, dp, 1, 0, None, None, None, None, None) == _lib.E_INVALID
    still_fine()
    assert _lib.lib.hmogp_predict_f_joint(h, None, 0, 1, dp, None, None) == 0          # N = 0 returns at once
    jit, rung = C.c_double(7.0), C.c_int32(7)
    assert _lib.lib.hmogp_sample_f_joint(h, None, 0, 1, dp, 1, 0, None, None, None, C.byref(jit), C.byref(rung)) == 0
    assert e.predict_f_joint(np.zeros((0, case["P"])), [0])[1].shape == (1, 0, 1, 0)
    # the optional outputs of the sampler may be left out
    F = np.zeros((2, 5))
    assert _lib.lib.hmogp_sample_f_joint(h, xp, 5, 1, dp, 2, 9, F.ctypes.data_as(_lib.c_double_p), None, None, None, None) == 0
    assert np.array_equal(F, e.sample_f_joint(Xnew, [0], size=2, seed=9).reshape(2, 5))
    still_fine()
    e.close()


# ------------------------------------------------------------------------------------------------------------ the facade
@pytest.fixture(scope="module")
def model():
    import hetmogp_amd as H
    rng = np.random.RandomState(5)
    Q, P, M, n = 2, 1, 12, 40
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.4), H.HetGaussian(), H.Categorical(K=3), H.Poisson()])
    md = likelihood.generate_metadata()
    kern_list = H.latent_functions_prior(Q, lenghtscale=[0.12, 0.2], variance=[1.0, 0.7], input_dim=P)
    X = [np.sort(rng.rand(n, P), 0) for _ in range(4)]
    Y = [rng.randn(n, 1), rng.randn(n, 1), rng.randint(1, 4, (n, 1)).astype(float), rng.poisson(2.0, (n, 1)).astype(float)]
    m = H.SVMOGP(X=X, Y=Y, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood, Y_metadata=md)
    m.q_u_means[...] = 0.6 * rng.randn(M, Q)
    r, c = np.tril_indices(M)
    m.q_u_chols[...] = np.stack([(0.5 * np.eye(M) + 0.05 * np.tril(rng.randn(M, M), -1))[r, c] for _ in range(Q)], 1)
    m.parameters_changed()
    return m


def facade_prm(m):
    Q = len(m.kern_list)
    return dict(Z=np.array(m.Z.values), m_u=np.array(m.q_u_means.values), L_flat=np.array(m.q_u_chols.values),
                variance=np.array([float(k.variance[0]) for k in m.kern_list]), lengthscale=np.array([float(k.lengthscale[0]) for k in m.kern_list]),
                W=np.stack([np.ravel(m.B_list[q].W.values) for q in range(Q)]), kappa=np.stack([np.ravel(m.B_list[q].kappa.values) for q in range(Q)]))


def test_facade_predict_f_full_cov(model):
    X = np.linspace(0.05, 0.95, 7)[:, None]
    Df = model.num_output_funcs
    assert Df == 6                                          # 1 + 2 + 2 + 1
    m0, v0 = model.predict_f(X)
    m1, v1 = model._engine.predict_f(np.asarray(X, dtype=float).reshape(-1, model.Xdim))      # the parent's code path
    assert np.array_equal(m0, m1) and np.array_equal(v0, v1) and m0.shape == (7, Df)
    mean, cov = model.predict_f(X, full_cov=True)
    assert mean.shape == (7, Df) and cov.shape == (Df, 7, Df, 7)
    assert np.array_equal(mean, m0)
    c2 = cov.reshape(Df * 7, Df * 7)
    assert np.array_equal(c2, c2.T)
    _, _, _, sc = jr.joint(facade_prm(model), X, range(Df), return_scale=True)
    assert np.max(jr.ratios(np.diag(c2), v0.T.reshape(-1), np.diag(sc))) <= 2.0 * jr.c_kernel("cov")
    ms, cs = model.predict_f(X, full_cov=True, functions=[3, 4])
    assert ms.shape == (7, 2) and cs.shape == (2, 7, 2, 7) and np.array_equal(cs, cov[3:5][:, :, 3:5]) and np.array_equal(ms, m0[:, 3:5])
    with pytest.raises(ValueError):
        model.predict_f(X, functions=[0])


def test_facade_posterior_samples(model):
    X = np.linspace(0.05, 0.95, 6)[:, None]
    F = model.posterior_samples_f(X, size=5, seed=3)
    assert F.shape == (5, 6, 6) and np.all(np.isfinite(F))
    assert np.array_equal(F, model.posterior_samples_f(X, size=5, seed=3))
    assert np.array_equal(F[:2], model.posterior_samples_f(X, size=2, seed=3))
    assert not np.array_equal(F, model.posterior_samples_f(X, size=5, seed=4))
    assert model.posterior_samples_f(X, size=4, functions=[1, 2], seed=3).shape == (4, 6, 2)
    np.random.seed(12)
    a = model.posterior_samples_f(X, size=2)                # seed=None: from NumPy's global generator
    np.random.seed(12)
    assert np.array_equal(a, model.posterior_samples_f(X, size=2))
    counts = model.posterior_samples(X, 3, size=9, seed=1)
    assert counts.shape == (9, 6) and np.all(counts >= 0) and np.array_equal(counts, np.floor(counts))
    assert np.array_equal(counts, model.posterior_samples(X, 3, size=9, seed=1))
    labels = model.posterior_samples(X, 2, size=9, seed=1)
    assert labels.shape == (9, 6) and set(np.unique(labels)) <= {1.0, 2.0, 3.0}
    assert model.posterior_samples(X, 1, size=4, seed=1).shape == (4, 6)


def test_facade_gaussian_draws_have_the_predictive_variance(model):
    """y = f + sigma eps at one input, S = 2000 draws: sum (y - mean)^2 / (cov_ii + sigma^2) is chi-square with S degrees of freedom."""
    from scipy import stats
    X = np.array([[0.31], [0.77]])
    S = 2000
    y = model.posterior_samples(X, 0, size=S, seed=21)
    mean, cov = model.predict_f(X, full_cov=True, functions=[0])
    sigma = model.likelihood.likelihoods_list[0].sigma
    for i in range(2):
        stat = np.sum((y[:, i] - mean[i, 0]) ** 2) / (cov[0, i, 0, i] + sigma ** 2)
        lo, hi = stats.chi2.ppf(2.5e-7, S), stats.chi2.isf(2.5e-7, S)       # 1e-6 over the two inputs, two-sided
        print("input %d: chi-square statistic %.1f in [%.1f, %.1f]" % (i, stat, lo, hi))
        assert lo <= stat <= hi
