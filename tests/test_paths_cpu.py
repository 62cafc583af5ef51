"""Pathwise (Matheron) posterior samples, CPU side: the float64 restatement (tests/paths_ref.py) against the 50-digit grid
tests/golden/pathsgrid.npz, the grid's regeneration, the scales in both arithmetics, the criteria's sensitivity, the separation of the
generator's streams, the interpolation identity, the law of the paths given their frequencies (two forms of the covariance; the statistical
case on the restatement's own paths) and the four new C-ABI symbols.  The device is held to the same grid in tests/test_paths_gpu.py."""
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
import paths_ref as pr            # noqa: E402

GRID = pr.load_grid()
NAMES = [c["name"] for c in pr.CASES]


@pytest.fixture(scope="module")
def restated():
    """(state, scales) of every case, computed once."""
    out = {}
    for n in NAMES:
        c = GRID[n]["case"]
        out[n] = pr.state(GRID[n]["prm"], c["P"], c["functions"], c["S"], c["Lf"], pr.GRID_SEED, return_scale=True)
    return out


def test_cases_cover_the_designed_shapes():
    C = pr.CASES
    assert len(GRID) == len(C)
    assert {c["N"] for c in C} == {1, 63, 64, 65, 129} and {c["M"] for c in C} == {16, 128}
    assert {c["P"] for c in C} == {1, 2, 4} and {c["Q"] for c in C} == {1, 3}
    assert {len(c["functions"]) for c in C} == {1, 2, 3} and {c["S"] for c in C} == {1, 3, 8} and {c["Lf"] for c in C} == {1, 8, 50, 64}
    tasks = [{pr.TASK_OF[d] for d in c["functions"]} for c in C]
    assert any(len(t) == len(c["functions"]) > 1 for t, c in zip(tasks, C))          # functions of different tasks
    assert any(len(t) < len(c["functions"]) for t, c in zip(tasks, C))               # two functions of one task
    assert any(list(c["functions"]) != sorted(c["functions"]) for c in C)            # out of order
    assert all(2 * c["Lf"] + c["M"] <= 2 * 64 + 128 for c in C)                      # the contraction lengths C_ORACLE absorbs
    for c in C:
        prm, _ = pr.make_params(c)
        assert max(jr.cond_estimates(prm, c["P"])) <= 50.0
        jc = jr.CASE_BY_NAME[c["name"]]
        assert all(c[k] == jc[k] for k in ("M", "Q", "P", "N", "functions", "seed"))   # the model set-up of DESIGN 9r's grid
    assert os.path.getsize(pr.GRID) < 400 * 1024


def test_restatement_against_the_grid(restated):
    worst = {"zeta": 0.0, "theta": 0.0, "u": 0.0, "v": 0.0, "F": 0.0}
    for n in NAMES:
        e, c = GRID[n], GRID[n]["case"]
        st = restated[n][0]
        r = pr.state_ratios(e, st)
        r["zeta"], r["theta"] = pr.draw_ratios(e, st)
        F = pr.evaluate(pr.synthetic_state(c, e["prm"]), e["prm"], c["P"], e["Xnew"])
        r["F"] = float(np.max(pr.ratios(pr.pick(F, e["i_F"]), e["F"], e["F_scale"])))
        print("%-7s " % n + "  ".join("%s %.3f" % (k, r[k]) for k in sorted(r)))
        for k in worst:
            worst[k] = max(worst[k], r[k])
    assert worst["zeta"] <= pr.C_Z and worst["theta"] <= pr.C_Z
    for what in ("u", "v", "F"):
        assert worst[what] <= pr.c_oracle(what), (what, worst[what])
        assert worst[what] > pr.c_oracle(what) / 64.0 or pr.c_oracle(what) == 1.0, "C_ORACLE is not the measured figure any more"


def test_grid_regenerates_bit_for_bit():
    import make_paths_grid as mk
    for n in pr.REGEN_CASES:
        e = GRID[n]
        ref = mk.build_case(e["case"])
        for k, v in ref.items():
            assert np.array_equal(v, e[k]), (n, k)


def test_float64_scales_equal_the_50_digit_scales(restated):
    for n in NAMES:
        e, c = GRID[n], GRID[n]["case"]
        sc = restated[n][1]
        for k in ("theta", "u", "v"):
            assert np.allclose(pr.pick(sc[k], e["i_" + k]), e[k + "_scale"], rtol=1e-9, atol=0.0), (n, k)
        _, sF = pr.evaluate(pr.synthetic_state(c, e["prm"]), e["prm"], c["P"], e["Xnew"], return_scale=True)
        assert np.allclose(pr.pick(sF, e["i_F"]), e["F_scale"], rtol=1e-9, atol=0.0), n


def test_a_moved_result_is_caught():
    """An entry off by 2 C 2^-52 scale fails the device's criterion, whichever array it is in."""
    for n in ("s_N1", "s_N64", "r_N65"):
        e = GRID[n]
        for k in ("theta", "u", "v", "F"):
            C_ = pr.C_Z if k == "theta" else pr.c_kernel(k)
            j = len(e[k]) // 2
            moved = e[k].copy()
            assert np.max(pr.ratios(moved, e[k], e[k + "_scale"])) == 0.0
            moved[j] += 2.0 * C_ * pr.EPS * e[k + "_scale"][j]
            assert np.max(pr.ratios(moved, e[k], e[k + "_scale"])) > C_, (n, k)
        bad = e["F"].copy()
        bad[0] = np.nan
        assert np.isinf(np.max(pr.ratios(bad, e["F"], e["F_scale"])))


def test_stream_separation():
    """No (n, s, pair) triple is used twice within a set.  The four tags separate the streams; within a tag the triples are the full product
    of an n-axis and an s-axis, so they are distinct iff each axis is -- enumerated at small shapes, and axis by axis at the caps."""
    for (Q, P, M, S, Lf, d) in ((1, 1, 3, 1, 1, (0,)), (3, 4, 16, 3, 8, (3, 0, 2)), (2, 2, 5, 8, 50, (1, 2))):
        t = pr.used_triples(Q, P, M, S, Lf, d)
        assert len(np.unique(t, axis=0)) == len(t) == Q * Lf * P + S * Q * (2 * Lf + M) + len(d) * S * Q * 2 * Lf
    Q, P, M, Lf = 8, 4, 1024, pr.MAXFEAT
    for d in ((0,), (3, 1), tuple(range(8))):
        S = pr.MAXCOLS // len(d)
        q, s = np.arange(Q), np.arange(S)
        sq = (s[None, :] * Q + q[:, None]).reshape(-1)
        axes = {pr.TAG_FREQ: (np.arange(Lf), (q[:, None] * 4 + np.arange(P)[None, :]).reshape(-1)), pr.TAG_PRIOR: (np.arange(2 * Lf), sq),
                pr.TAG_QU: (np.arange(M), sq), pr.TAG_KAPPA: ((np.asarray(d)[:, None] * 2 * Lf + np.arange(2 * Lf)[None, :]).reshape(-1), sq)}
        for tag, (na, sa) in axes.items():
            assert 0 < tag < 256 and len(np.unique(na)) == len(na) and len(np.unique(sa)) == len(sa)
            assert na.min() >= 0 and sa.min() >= 0 and int(sa.max()) < 2 ** 55            # (s << 8 stays inside 64 bits)
    assert len({pr.TAG_FREQ, pr.TAG_PRIOR, pr.TAG_QU, pr.TAG_KAPPA, 0}) == 5              # pair 0 is the joint sampler's


@pytest.mark.parametrize("Lf", [1, 64])
def test_update_cancels_the_feature_error_at_the_inducing_inputs(Lf):
    """Phi(Z) theta + K v = u whatever Lf is, within the state criterion: w (Phi_Z theta) + K v~ = w u."""
    c = pr.CASE_BY_NAME["s_N64"]
    prm, _ = pr.make_params(c)
    d, S = (0, 3), 3
    st, sc = pr.state(prm, c["P"], d, S, Lf, seed=5, return_scale=True)
    dr = pr.draws(5, c["Q"], c["P"], c["M"], S, Lf, d)
    for q in range(c["Q"]):
        lt = pr.latent_q(prm, q, c["P"])
        PhiZ = pr.features(st["omega"][q], np.sqrt(lt["var"] / Lf), lt["Zq"])[0]
        for j, dj in enumerate(d):
            w = prm["W"][q, dj]
            for s in range(S):
                prior = PhiZ @ dr["theta"][q, s]
                resid = w * prior + lt["K"] @ st["v"][q, :, s, j] - w * st["u"][q, s]
                bound = pr.EPS * (pr.c_oracle("v") * (np.abs(lt["K"]) @ sc["v"][q, :, s, j])
                                  + 4.0 * (abs(w) * (np.abs(PhiZ) @ np.abs(dr["theta"][q, s]) + np.abs(st["u"][q, s])) + np.abs(lt["K"]) @ np.abs(st["v"][q, :, s, j])))
                assert np.all(np.abs(resid) <= bound), (Lf, q, j, s, np.max(np.abs(resid) / bound))
    if Lf == 1:      # the prior features alone are useless here: the update carries the path
        assert np.max(np.abs(PhiZ @ dr["theta"][q, 0] - st["u"][q, 0])) > 0.1


@pytest.mark.parametrize("name", ["s_N63", "s_N64", "r_N65"])
def test_conditional_covariance_in_both_forms(restated, name):
    """Given the frequencies: the covariance from the paths' own linear form equals 9r's formula with k_q replaced by phi^T phi (and the
    feature-error term at the inducing inputs), and is symmetric positive semi-definite."""
    e, c = GRID[name], GRID[name]["case"]
    X = e["Xnew"][:7]
    om = restated[name][0]["omega"]
    a = pr.cond_cov(om, e["prm"], c["P"], c["functions"], X)
    b = pr.cond_cov_formula(om, e["prm"], c["P"], c["functions"], X)
    scale = np.sqrt(np.outer(np.diag(a), np.diag(a)))
    assert np.max(np.abs(a - b) / scale) <= 1e-9
    assert np.max(np.abs(a - a.T) / scale) <= 1e-13 and np.min(np.linalg.eigvalsh(0.5 * (a + a.T))) >= -1e-10 * np.max(np.diag(a))
    const, T = pr.freq_terms(om, e["prm"], c["P"], c["functions"], X)
    assert np.max(np.abs(const + T.mean(0) - a) / scale) <= 1e-9


def test_statistical_thresholds_hold_for_the_restatement():
    """The statistical case of the GPU suite on the restatement's own paths (same seed): given the stored frequencies the paths are exactly
    Gaussian with predict_f's mean and the conditional covariance, so 9r's exact-law statistics apply unchanged."""
    prm, Xnew, d = pr.stat_case()
    P = Xnew.shape[1]
    st = pr.state(prm, P, d, pr.STAT_DRAWS, pr.STAT_FEATURES, pr.STAT_SEED)
    F = pr.evaluate(st, prm, P, Xnew).reshape(pr.STAT_DRAWS, -1)
    mean = jr.predict_f(prm, Xnew)[0][:, list(d)].T.reshape(-1)
    cov = pr.cond_cov(st["omega"], prm, P, d, Xnew)
    assert F.shape[1] == 8
    zm, zc = pr.stat_zscores(F, mean, cov)
    t = pr.stat_threshold(8)
    print("max |z| mean %.2f cov %.2f threshold %.2f" % (zm, zc, t))
    assert zm <= t and zc <= t
    # ... and a wrong law is told apart: a covariance 30 % too large, a mean off by a fifth of a standard deviation
    assert pr.stat_zscores(F, mean, 1.3 * cov)[1] > t and pr.stat_zscores(F, mean + 0.2 * np.sqrt(np.diag(cov)), cov)[0] > t


def test_feature_error_statistic_on_the_restatement():
    prm, Xnew, d = pr.stat_case()
    P = Xnew.shape[1]
    Q = prm["variance"].shape[0]
    Lf = 512
    dr = pr.draws(pr.FEAT_SEED, Q, P, 1, 1, Lf, d)
    omega = dr["zeta"] / (np.pi * prm["lengthscale"][:, None, None])
    z, err, count = pr.feature_error_z(omega, prm, P, d, Xnew, jr.joint(prm, Xnew, d, strict=True)[1])
    print("worst |z| %.2f, worst |error| %.3e over %d entries, threshold %.2f" % (z, err, count, pr.z_threshold(count)))
    assert count == 36 and z <= pr.z_threshold(count)


def test_abi_symbols_and_refusals_without_a_device():
    """The four symbols exist, the ABI version stays 8, a NULL handle is refused on the host with a message, and without a device the engine
    itself is refused with HMOGP_E_NO_DEVICE (the refusals that need an engine: tests/test_paths_gpu.py::test_refusals)."""
    import torch
    from hetmogp_amd import _lib, engine
    assert _lib.ABI_VERSION == 8 and _lib.lib.hmogp_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "hetmogp_hip.h")).read()
    for sym in ("hmogp_paths_create", "hmogp_paths_eval", "hmogp_paths_state", "hmogp_paths_free"):
        assert sym in _lib.EXPORTS and sym + "(" in header
    for line in ("#define HMOGP_PATHS_MAXFEAT 8192", "#define HMOGP_PATHS_MAXCOLS 4096", "#define HMOGP_PATHS_MAXSETS 16", "#define HMOGP_ABI_VERSION 8"):
        assert line in header
    assert (_lib.PATHS_MAXFEAT, _lib.PATHS_MAXCOLS, _lib.PATHS_MAXSETS) == (pr.MAXFEAT, pr.MAXCOLS, pr.MAXSETS) == (8192, 4096, 16)
    import ctypes as C
    d = np.zeros(1, dtype=np.int32)
    buf = np.zeros(4)
    sid = C.c_int32(-1)
    dp, bp = d.ctypes.data_as(_lib.c_int32_p), buf.ctypes.data_as(_lib.c_double_p)
    assert _lib.lib.hmogp_paths_create(None, 1, dp, 1, 1, 0, C.byref(sid)) == _lib.E_INVALID and sid.value == -1
    assert b"handle is NULL" in _lib.lib.hmogp_last_error(None)
    assert _lib.lib.hmogp_paths_eval(None, 0, bp, 1, bp) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_state(None, 0, None, None, None, None) == _lib.E_INVALID
    assert _lib.lib.hmogp_paths_free(None, 0) == _lib.E_INVALID
    # A thin guard only, not a proof of control flow: without a device there is no engine to refuse anything, so the refusals themselves are
    # exercised in tests/test_paths_gpu.py::test_refusals (each followed by a valid call).  Here: every entry point checks the engine's
    # state before it first names the device, and paths_create asks about memory before it allocates.
    src = open(os.path.join(ROOT, "hetmogp_amd", "csrc", "engine_optim.hip")).read()
    for fn in ("paths_create", "paths_eval", "paths_state", "paths_free"):
        body = src[src.index("void hmogp_engine::%s(" % fn):]
        assert 0 <= body.index("HMOGP_E_STATE") < body.index("hipSetDevice"), fn
    create = src[src.index("void hmogp_engine::paths_create("):]
    assert create.index("hipMemGetInfo") < create.index(".ensure(")
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HetMOGPError) as ei:
            engine.Engine(pr.SPECS, 1, 16, 1, device=0)
        assert ei.value.code == _lib.E_NO_DEVICE
