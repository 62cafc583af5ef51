"""GPU: pathwise (Matheron) posterior samples (`hmogp_paths_create` / `_eval` / `_state` / `_free`) against the 50-digit grid
tests/golden/pathsgrid.npz and the restatements of tests/paths_ref.py / tests/paths_ref_mp.py -- draws, state and evaluation entry by entry
from a default-mode and a strict-mode evaluation on the small-model and the regular path, one set of bits in both modes, independence of rows,
chunks, S and the list of functions, the snapshot, interpolation at the inducing inputs, the exact law given the frequencies, the feature
error against the exact posterior, a call beyond the joint route's bound, the facade, the refusals.

Criteria (paths_ref's docstring): |got - R| <= C 2^-52 scale.  Draws: C_Z = 16 ulps of the normal.  State: u 16, v 4096 = max(16, 4 C_ORACLE) with
C_ORACLE 1024 (GPy's cancelling order of K_uu at l = 1 / 127, which scale_v does not fold in).  Evaluation, against the 50-digit evaluation
from the device's OWN state: 16.  Every figure measured on the MI355X: DESIGN 9v."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import joint_ref as jr            # noqa: E402
import paths_ref as pr            # noqa: E402

pytestmark = pytest.mark.gpu

GRID = pr.load_grid()
NAMES = [c["name"] for c in pr.CASES]
MODES = [False, True]
N_EVAL = 24                        # entries per case the evaluation is held to 50 digits on (seconds of mpmath per case otherwise)
_ENG, _RES, _REF = {}, {}, {}


def ids(strict):
    return "strict" if strict else "default"


def engine(name, strict=False, **kw):
    """One engine per (case, mode, options), with the case's parameters evaluated once."""
    key = (name, strict, tuple(sorted(kw.items())))
    if key not in _ENG:
        from hetmogp_amd.engine import Engine
        case = pr.CASE_BY_NAME[name]
        prm, _ = pr.make_params(case)
        X, Y = pr.train_data(case)
        e = Engine(pr.SPECS, case["Q"], case["M"], case["P"], device=0, strict_qf=strict, **kw)
        e.set_data(X, Y)
        out = e.elbo_grad(**prm)
        assert all(r == -1 for r in out["rungs"])
        _ENG[key] = e
    return _ENG[key]


def result(name, strict):
    """The designed path set of one (case, mode): state and evaluation, computed once, left unchanged."""
    key = (name, strict)
    if key not in _RES:
        c, g = pr.CASE_BY_NAME[name], GRID[name]
        e = engine(name, strict)
        sid = e.paths_create(c["functions"], size=c["S"], num_features=c["Lf"], seed=pr.GRID_SEED)
        _RES[key] = dict(engine=e, sid=sid, state=e.paths_state(sid), F=e.paths_eval(sid, g["Xnew"]))
    return _RES[key]


def reference_eval(name):
    """(indices, R, scale): the 50-digit evaluation from the device's own state (the default mode's; the strict one's is the same bits)."""
    if name not in _REF:
        import paths_ref_mp as pm
        g, c = GRID[name], pr.CASE_BY_NAME[name]
        idx = g["i_F"][::max(1, len(g["i_F"]) // N_EVAL)][:N_EVAL]
        R, sc = pm.evaluate(result(name, False)["state"], g["prm"], c["P"], g["Xnew"], idx)
        _REF[name] = (idx, R, sc)
    return _REF[name]


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", NAMES)
def test_draws_and_state_against_the_grid(name, strict):
    r, g = result(name, strict), GRID[name]
    rz, rt = pr.draw_ratios(g, r["state"])
    rs = pr.state_ratios(g, r["state"])
    print("%s %s: zeta %.3f theta %.3f (C %g) u %.3f (C %g) v %.3f (C %g)" % (name, ids(strict), rz, rt, pr.C_Z, rs["u"], pr.c_kernel("u"), rs["v"],
                                                                              pr.c_kernel("v")))
    assert rz <= pr.C_Z and rt <= pr.C_Z
    assert rs["u"] <= pr.c_kernel("u") and rs["v"] <= pr.c_kernel("v")
    assert all(np.all(np.isfinite(a)) for a in r["state"].values())


@pytest.mark.parametrize("name", NAMES)
def test_evaluation_against_50_digits_from_the_own_state(name):
    idx, R, sc = reference_eval(name)
    for strict in MODES:
        ratio = float(np.max(pr.ratios(pr.pick(result(name, strict)["F"], idx), R, sc)))
        print("%s %s: F %.3f (C %g) on %d entries" % (name, ids(strict), ratio, pr.c_kernel("F"), len(idx)))
        assert ratio <= pr.c_kernel("F")
    # ... and every entry against the float64 restatement from the same state: each within its own constant of the 50-digit value
    g, c = GRID[name], pr.CASE_BY_NAME[name]
    F64, s64 = pr.evaluate(result(name, False)["state"], g["prm"], c["P"], g["Xnew"], return_scale=True)
    assert np.max(pr.ratios(result(name, False)["F"], F64, s64)) <= pr.c_kernel("F") + pr.c_oracle("F")


@pytest.mark.parametrize("name", NAMES)
def test_one_set_of_bits_in_both_modes(name):
    a, b = result(name, False), result(name, True)
    for k in ("omega", "theta", "v", "u"):
        assert np.array_equal(a["state"][k], b["state"][k]), k
    assert np.array_equal(a["F"], b["F"]) and np.all(np.isfinite(a["F"]))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["s_N64", "r_N65"])
def test_row_independence(name, N):
    """The rows of a call equal the same rows evaluated alone, in two halves, and in a second call."""
    c = pr.CASE_BY_NAME[name]
    r = result(name, False)
    e, sid = r["engine"], r["sid"]
    X = np.random.RandomState(100 + N).rand(N, c["P"])
    F = e.paths_eval(sid, X)
    assert F.shape == (c["S"], len(c["functions"]), N) and np.all(np.isfinite(F))
    assert np.array_equal(F, e.paths_eval(sid, X))
    for i in sorted({0, N // 2, N - 1}):
        assert np.array_equal(F[:, :, i:i + 1], e.paths_eval(sid, X[i:i + 1]))
    h = (N + 1) // 2
    assert np.array_equal(F[:, :, :h], e.paths_eval(sid, X[:h])) and np.array_equal(F[:, :, h:], e.paths_eval(sid, X[h:]))


@pytest.mark.parametrize("name", ["s_N129", "r_N129"])
def test_forced_chunks_give_the_same_bits(name):
    """Chunks of 48 rows over 129 against the unchunked call."""
    c, g = pr.CASE_BY_NAME[name], GRID[name]
    e48 = engine(name, False, chunk_rows=48)
    sid = e48.paths_create(c["functions"], size=c["S"], num_features=c["Lf"], seed=pr.GRID_SEED)
    assert np.array_equal(e48.paths_eval(sid, g["Xnew"]), result(name, False)["F"])
    e48.paths_free(sid)


@pytest.mark.parametrize("strict", MODES, ids=ids)
@pytest.mark.parametrize("name", ["s_N64", "r_N65"])
def test_samples_functions_and_seeds(name, strict):
    c, g = pr.CASE_BY_NAME[name], GRID[name]
    e = engine(name, strict)
    d = list(c["functions"])
    X = g["Xnew"]
    sets = {S: e.paths_create(d, size=S, num_features=c["Lf"], seed=3) for S in (1, 3, 8)}
    F = {S: e.paths_eval(sid, X) for S, sid in sets.items()}
    st = {S: e.paths_state(sid) for S, sid in sets.items()}
    for S in (1, 3):                                        # sample s does not depend on S
        assert np.array_equal(F[S], F[8][:S])
        assert np.array_equal(st[S]["theta"], st[8]["theta"][:, :, :S]) and np.array_equal(st[S]["v"], st[8]["v"][:, :, :S])
        assert np.array_equal(st[S]["u"], st[8]["u"][:, :S]) and np.array_equal(st[S]["omega"], st[8]["omega"])
    sub = [len(d) - 1, 0]                                   # positions in d: a sub-list, in another order
    sid = e.paths_create([d[j] for j in sub], size=8, num_features=c["Lf"], seed=3)
    assert np.array_equal(e.paths_eval(sid, X), F[8][:, sub])
    assert np.array_equal(e.paths_state(sid)["theta"], st[8]["theta"][..., sub])
    e.paths_free(sid)
    sid = e.paths_create(d, size=3, num_features=c["Lf"], seed=4)
    other = e.paths_eval(sid, X)
    assert other.shape == F[3].shape and not np.any(other == F[3])
    for s in list(sets.values()) + [sid]:
        e.paths_free(s)


def test_a_set_is_a_snapshot():
    name = "s_N63"
    c, g = pr.CASE_BY_NAME[name], GRID[name]
    from hetmogp_amd.engine import Engine
    X, Y = pr.train_data(c)
    e = Engine(pr.SPECS, c["Q"], c["M"], c["P"], device=0)
    e.set_data(X, Y)
    e.elbo_grad(**g["prm"])
    old = e.paths_create(c["functions"], size=3, num_features=8, seed=1)
    F0, s0 = e.paths_eval(old, g["Xnew"]), e.paths_state(old)
    prm2 = dict(g["prm"], m_u=g["prm"]["m_u"] + 0.1, lengthscale=g["prm"]["lengthscale"] * 1.1, variance=g["prm"]["variance"] * 0.9,
                W=g["prm"]["W"] * 1.2, Z=g["prm"]["Z"] + 0.001)
    e.elbo_grad(**prm2)
    assert np.array_equal(e.paths_eval(old, g["Xnew"]), F0)
    assert all(np.array_equal(v, s0[k]) for k, v in e.paths_state(old).items())
    new = e.paths_create(c["functions"], size=3, num_features=8, seed=1)
    assert new != old and not np.any(e.paths_eval(new, g["Xnew"]) == F0)
    e.close()


@pytest.mark.parametrize("Lf", [1, 64])
@pytest.mark.parametrize("name", ["s_N129", "r_N129"])
def test_interpolation_at_the_inducing_inputs(name, Lf):
    """Q = 1, Xnew = Z: the paths minus the kappa part (recomputed on the host from the state's frequencies and the restated normals) equal
    w u -- also at Lf = 1, where the prior features alone are useless: the update is wired to the right latent, sample and sign."""
    c = pr.CASE_BY_NAME[name]
    assert c["Q"] == 1
    prm, _ = pr.make_params(c)
    e = engine(name)
    d, S, seed = [0, 2], 3, 9
    sid = e.paths_create(d, size=S, num_features=Lf, seed=seed)
    st = e.paths_state(sid)
    Z = prm["Z"][:, :c["P"]]
    F = e.paths_eval(sid, Z)
    e.paths_free(sid)
    _, sF = pr.evaluate(st, prm, c["P"], Z, return_scale=True)
    _, sc = pr.state(prm, c["P"], d, S, Lf, seed, return_scale=True)
    dr = pr.draws(seed, 1, c["P"], c["M"], S, Lf, d)
    lt = pr.latent_q(prm, 0, c["P"])
    PhiZ, at = pr.features(st["omega"][0], np.sqrt(lt["var"] / Lf), Z)
    grow = 1.0 + np.pi * np.concatenate([at, at], 1)
    worst = 0.0
    for j, dj in enumerate(d):
        w, sk = prm["W"][0, dj], np.sqrt(prm["kappa"][0, dj])
        for s in range(S):
            kpart = sk * (PhiZ @ dr["thetak"][j, 0, s])
            resid = F[s, j] - kpart - w * st["u"][0, s]
            # (the kappa part is recomputed from the RESTATED normals: the device's and the restated one are each within C_Z ulps of the
            #  50-digit normal -- the restated one within 4 --, hence 2 C_Z on that term)
            bound = pr.EPS * (pr.c_kernel("F") * sF[s, j] + pr.c_kernel("v") * (np.abs(lt["K"]) @ sc["v"][0, :, s, j])
                              + 2.0 * pr.C_Z * sk * ((np.abs(PhiZ) * grow) @ np.abs(dr["thetak"][j, 0, s])))
            worst = max(worst, float(np.max(np.abs(resid) / bound)))
            assert np.all(np.abs(resid) <= bound)
            # (the bound above carries v's constant 4096; these two cases need far less: K_q carries 2 / l^2 <= 352 ulps, the condition
            #  estimate is <= 50, so the update's error is ~ 50 x 352 x 2^-52 = 4e-12 of |w u|: 1e-9 says these ARE the values w u)
            assert np.max(np.abs(resid)) <= 1e-9 * np.max(np.abs(w * st["u"][0, s]))
    print("%s Lf %d: worst residual %.3e of the bound" % (name, Lf, worst))


def test_paths_follow_the_law_given_the_frequencies():
    """n = 8 (two functions at four inputs), S = 4096, Lf = 64: given the stored frequencies the paths are exactly Gaussian, so 9r's exact-law
    statistics apply with predict_f's mean and the conditional covariance from the state.  nD S = 8192 exceeds HMOGP_PATHS_MAXCOLS, so the two
    functions are drawn as two single-function sets of one seed -- the same bits as one two-function set, by the sub-list property."""
    prm, Xnew, d = pr.stat_case()
    name = "s_N64"
    assert all(np.array_equal(prm[k], GRID[name]["prm"][k]) for k in prm)
    e = engine(name)
    sids = [e.paths_create([dj], size=pr.STAT_DRAWS, num_features=pr.STAT_FEATURES, seed=pr.STAT_SEED) for dj in d]
    F = np.concatenate([e.paths_eval(s, Xnew) for s in sids], 1).reshape(pr.STAT_DRAWS, -1)
    omega = e.paths_state(sids[0])["omega"]
    assert np.array_equal(omega, e.paths_state(sids[1])["omega"])
    for s in sids:
        e.paths_free(s)
    pair = e.paths_create(list(d), size=16, num_features=pr.STAT_FEATURES, seed=pr.STAT_SEED)
    assert np.array_equal(e.paths_eval(pair, Xnew).reshape(16, -1), F[:16])
    e.paths_free(pair)
    mean = e.predict_f(Xnew)[0][:, list(d)].T.reshape(-1)
    cov = pr.cond_cov(omega, prm, Xnew.shape[1], d, Xnew)
    assert F.shape[1] == 8
    zm, zc = pr.stat_zscores(F, mean, cov)
    t = pr.stat_threshold(8)
    print("max |z|: means %.2f, second moments %.2f, threshold %.2f" % (zm, zc, t))
    assert zm <= t and zc <= t


def test_feature_error_against_the_exact_posterior():
    """Lf = 4096, n = 8: the conditional covariance from the state against predict_f(full_cov=True), each entry a mean of Lf i.i.d. per-frequency
    terms: a z-test with the terms' sample standard deviation.  The one place the approximation is measured, not pinned."""
    prm, Xnew, d = pr.stat_case()
    e = engine("s_N64")
    sid = e.paths_create(list(d), size=1, num_features=pr.FEAT_FEATURES, seed=pr.FEAT_SEED)
    omega = e.paths_state(sid)["omega"]
    e.paths_free(sid)
    exact = e.predict_f_joint(Xnew, list(d))[1].reshape(8, 8)
    z, err, count = pr.feature_error_z(omega, prm, Xnew.shape[1], d, Xnew, exact)
    t = pr.z_threshold(count)
    print("worst |z| %.2f (threshold %.2f), worst |error| %.3e, max diag %.3e" % (z, t, err, np.max(np.diag(exact))))
    assert count == 36 and z <= t


def test_beyond_the_joint_bound():
    name = "s_N64"
    c = pr.CASE_BY_NAME[name]
    e = engine(name)
    X = np.random.RandomState(8).rand(10000, c["P"])
    sid = e.paths_create([0], size=2, num_features=16, seed=2)
    F = e.paths_eval(sid, X)
    assert F.shape == (2, 1, 10000) and np.all(np.isfinite(F))
    for r0 in range(0, 10000, 1000):
        assert np.array_equal(F[:, :, r0:r0 + 1000], e.paths_eval(sid, X[r0:r0 + 1000]))
    e.paths_free(sid)
    from hetmogp_amd import _lib
    with pytest.raises(_lib.InvalidArgument, match="HMOGP_JOINT_MAXDIM"):
        e.sample_f_joint(X, [0], size=2, seed=2)


def test_refusals():
    """Every refusal is HMOGP_E_INVALID (HMOGP_E_STATE before the first evaluation) and is followed by a valid call on the same engine."""
    import ctypes as C
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine
    case = pr.CASE_BY_NAME["s_N64"]
    prm, Xnew = pr.make_params(case)
    Xnew = Xnew[:5]
    X, Y = pr.train_data(case)
    e = Engine(pr.SPECS, case["Q"], case["M"], case["P"], device=0)
    e.set_data(X, Y)
    h = e._h
    sid = C.c_int32(-1)
    dd = np.array([0, 3], dtype=np.int32)
    dp, xp = dd.ctypes.data_as(_lib.c_int32_p), Xnew.ctypes.data_as(_lib.c_double_p)
    buf = np.zeros(64)
    bp = buf.ctypes.data_as(_lib.c_double_p)
    assert _lib.lib.hmogp_paths_create(h, 2, dp, 2, 8, 1, C.byref(sid)) == _lib.E_STATE            # before the first evaluation
    assert _lib.lib.hmogp_paths_eval(h, 0, xp, 5, bp) == _lib.E_STATE
    assert _lib.lib.hmogp_paths_state(h, 0, None, None, None, None) == _lib.E_STATE
    assert _lib.lib.hmogp_paths_free(h, 0) == _lib.E_STATE
    e.elbo_grad(**prm)
    good_id = e.paths_create([0, 3], size=2, num_features=8, seed=1)
    good = e.paths_eval(good_id, Xnew)

    def still_fine():
        assert np.array_equal(e.paths_eval(good_id, Xnew), good)
        s = e.paths_create([3], size=1, num_features=2, seed=1)
        assert np.all(np.isfinite(e.paths_eval(s, Xnew)))
        e.paths_free(s)

    for bad in (dict(functions=[]), dict(functions=[4]), dict(functions=[-1]), dict(functions=[1, 1]), dict(functions=[0, 2, 0]), dict(size=0),
                dict(size=-2), dict(num_features=0), dict(num_features=_lib.PATHS_MAXFEAT + 1), dict(functions=[0, 1], size=_lib.PATHS_MAXCOLS // 2 + 1)):
        with pytest.raises(_lib.InvalidArgument):
            e.paths_create(**dict(dict(functions=[0], size=1, num_features=4, seed=0), **bad))
        still_fine()
    assert _lib.lib.hmogp_paths_create(h, 2, None, 2, 8, 1, C.byref(sid)) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_create(h, 2, dp, 2, 8, 1, None) == _lib.E_INVALID
    still_fine()
    for bad_id in (-1, _lib.PATHS_MAXSETS, good_id + 1):                                          # unknown ids
        assert _lib.lib.hmogp_paths_eval(h, bad_id, xp, 5, bp) == _lib.E_INVALID
        assert _lib.lib.hmogp_paths_state(h, bad_id, None, None, None, None) == _lib.E_INVALID
        assert _lib.lib.hmogp_paths_free(h, bad_id) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_eval(h, good_id, xp, -1, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_eval(h, good_id, None, 5, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_eval(h, good_id, xp, 5, None) == _lib.E_INVALID
    still_fine()
    assert _lib.lib.hmogp_paths_eval(h, good_id, None, 0, None) == 0                              # Nnew = 0 returns at once
    assert e.paths_eval(good_id, np.zeros((0, case["P"]))).shape == (2, 2, 0)
    assert _lib.lib.hmogp_paths_state(h, good_id, None, None, None, None) == 0                    # every output of the state may be left out
    # the 17th live set is refused; after a free a new one succeeds
    more = [e.paths_create([0], size=1, num_features=1, seed=k) for k in range(_lib.PATHS_MAXSETS - 1)]
    with pytest.raises(_lib.InvalidArgument, match="no free slot"):
        e.paths_create([0], size=1, num_features=1, seed=99)
    assert np.array_equal(e.paths_eval(good_id, Xnew), good)
    e.paths_free(more.pop())
    more.append(e.paths_create([0], size=1, num_features=1, seed=99))
    for s in more:
        e.paths_free(s)
    with pytest.raises(_lib.InvalidArgument, match="unknown or freed"):                           # a freed id
        e.paths_eval(more[0], Xnew)
    still_fine()
    e.paths_free(good_id)
    with pytest.raises(_lib.InvalidArgument):
        e.paths_free(good_id)
    still_sid = e.paths_create([0, 3], size=2, num_features=8, seed=1)
    assert np.array_equal(e.paths_eval(still_sid, Xnew), good)
    e.close()


# ------------------------------------------------------------------------------------------------------------ the facade
@pytest.fixture(scope="module")
def model():
    import hetmogp_amd as H
    rng = np.random.RandomState(5)
    Q, P, M, n = 2, 1, 12, 40
    likelihood = H.HetLikelihood([H.Gaussian(sigma=0.4), H.HetGaussian(), H.Poisson()])
    md = likelihood.generate_metadata()
    kern_list = H.latent_functions_prior(Q, lenghtscale=[0.12, 0.2], variance=[1.0, 0.7], input_dim=P)
    X = [np.sort(rng.rand(n, P), 0) for _ in range(3)]
    Y = [rng.randn(n, 1), rng.randn(n, 1), rng.poisson(2.0, (n, 1)).astype(float)]
    m = H.SVMOGP(X=X, Y=Y, Z=np.linspace(0, 1, M)[:, None], kern_list=kern_list, likelihood=likelihood, Y_metadata=md)
    m.q_u_means[...] = 0.6 * rng.randn(M, Q)
    r, c = np.tril_indices(M)
    m.q_u_chols[...] = np.stack([(0.5 * np.eye(M) + 0.05 * np.tril(rng.randn(M, M), -1))[r, c] for _ in range(Q)], 1)
    m.parameters_changed()
    return m


def test_facade_sample_paths(model):
    from hetmogp_amd import _lib
    X = np.linspace(0.05, 0.95, 6)[:, None]
    Df = model.num_output_funcs
    assert Df == 4
    paths = model.sample_paths(size=5, num_features=32, seed=3)
    assert (paths.functions, paths.size, paths.num_features, paths.seed) == ([0, 1, 2, 3], 5, 32, 3)
    F = paths(X)
    assert F.shape == (5, 6, Df) and np.all(np.isfinite(F)) and np.array_equal(F, paths(X))
    assert np.array_equal(paths(X[2:4]), F[:, 2:4])
    st = paths.state()
    assert st["omega"].shape == (2, 32, 1) and st["theta"].shape == (2, 64, 5, Df) and st["v"].shape == (2, 12, 5, Df) and st["u"].shape == (2, 5, 12)
    with model.sample_paths(size=2, functions=[2, 1], num_features=32, seed=3) as sub:
        assert sub.functions == [2, 1] and np.array_equal(sub(X), F[:2][:, :, [2, 1]])
    with pytest.raises(ValueError):
        sub(X)                                              # closed by the context manager
    paths.close()
    paths.close()                                           # (a second close is nothing)
    with pytest.raises(ValueError):
        paths(X)
    with pytest.raises(ValueError):
        paths.state()
    np.random.seed(12)
    a = model.sample_paths(size=2, num_features=8)          # seed=None: from NumPy's global generator
    np.random.seed(12)
    b = model.sample_paths(size=2, num_features=8)
    assert a.seed == b.seed and np.array_equal(a(X), b(X))
    a.close(), b.close()
    # the 17th live set is refused; after a close a new one succeeds
    live = [model.sample_paths(size=1, functions=[0], num_features=1, seed=k) for k in range(_lib.PATHS_MAXSETS)]
    with pytest.raises(_lib.InvalidArgument, match="no free slot"):
        model.sample_paths(size=1, functions=[0], num_features=1, seed=0)
    live.pop().close()
    live.append(model.sample_paths(size=1, functions=[0], num_features=1, seed=0))
    assert np.all(np.isfinite(live[-1](X)))
    for p in live:
        p.close()
    for bad in (dict(size=0), dict(num_features=0), dict(functions=[7]), dict(functions=[1, 1])):
        with pytest.raises(_lib.InvalidArgument):
            model.sample_paths(**dict(dict(size=1, seed=0), **bad))
        with model.sample_paths(size=1, num_features=4, seed=0) as ok:
            assert ok(X).shape == (1, 6, Df)


def test_facade_pathwise_methods(model):
    X = np.linspace(0.05, 0.95, 6)[:, None]
    F = model.posterior_samples_f(X, size=4, functions=[1, 2], seed=3, method="pathwise", num_features=64)
    with model.sample_paths(size=4, functions=[1, 2], num_features=64, seed=3) as paths:
        assert np.array_equal(F, paths(X))
    J = model.posterior_samples_f(X, size=4, functions=[1, 2], seed=3)
    assert F.shape == J.shape and F.dtype == J.dtype and not np.array_equal(F, J)
    assert np.array_equal(J, model.posterior_samples_f(X, size=4, functions=[1, 2], seed=3, method="joint"))
    for task in (0, 1, 2):
        yj = model.posterior_samples(X, task, size=9, seed=1)
        yp = model.posterior_samples(X, task, size=9, seed=1, method="pathwise", num_features=64)
        assert yp.shape == yj.shape and yp.dtype == yj.dtype and np.all(np.isfinite(yp))
        assert np.array_equal(yp, model.posterior_samples(X, task, size=9, seed=1, method="pathwise", num_features=64))
    counts = model.posterior_samples(X, 2, size=9, seed=1, method="pathwise")
    assert np.all(counts >= 0) and np.array_equal(counts, np.floor(counts))
    big = np.linspace(0, 1, 10000)[:, None]                 # beyond the joint route's bound
    assert model.posterior_samples_f(big, size=2, functions=[0], seed=1, method="pathwise", num_features=16).shape == (2, 10000, 1)
    with pytest.raises(ValueError):
        model.posterior_samples_f(big, size=2, functions=[0], seed=1)
    with pytest.raises(ValueError):
        model.posterior_samples_f(X, method="exact")
