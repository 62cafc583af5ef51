"""The joint posterior at new inputs, CPU side: the float64 restatement (tests/joint_ref.py) against the 50-digit grid
tests/golden/jointgrid.npz, the grid's regeneration, the criterion's sensitivity, the properties of the restated covariance, and the two
new C-ABI symbols.  The device is held to the same grid in tests/test_joint_gpu.py."""
import ctypes as C
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

GRID = jr.load_grid()
NAMES = [c["name"] for c in jr.CASES]


@pytest.fixture(scope="module")
def restated():
    """(mean, cov) of every case in both forms, computed once."""
    return {(n, s): jr.joint(GRID[n]["prm"], GRID[n]["Xnew"], GRID[n]["case"]["functions"], strict=s) for n in NAMES for s in (False, True)}


def test_cases_cover_the_issue():
    assert {c["N"] for c in jr.CASES} == {1, 63, 64, 65, 129}
    assert {len(c["functions"]) for c in jr.CASES} == {1, 2, 3}
    assert {c["P"] for c in jr.CASES} == {1, 2, 4} and {c["Q"] for c in jr.CASES} == {1, 3} and {c["M"] for c in jr.CASES} == {16, 128}
    tasks = [{jr.TASK_OF[d] for d in c["functions"]} for c in jr.CASES]
    assert any(len(t) == len(c["functions"]) > 1 for t, c in zip(tasks, jr.CASES))         # functions of different tasks
    assert any(len(t) < len(c["functions"]) for t, c in zip(tasks, jr.CASES))              # two functions of one task
    for c in jr.CASES:
        prm, _ = jr.make_params(c)
        assert max(jr.cond_estimates(prm, c["P"])) < jr.COND_FLAG


def test_grid_holds_the_designed_parameters():
    for c in jr.CASES:
        prm, Xnew = jr.make_params(c)
        e = GRID[c["name"]]
        for k, v in prm.items():
            assert np.array_equal(v, e["prm"][k]), (c["name"], k)
        assert np.array_equal(Xnew, e["Xnew"])
        ri, ci = jr.stored_entries(c)
        assert np.array_equal(ri, e["ri"]) and np.array_equal(ci, e["ci"])
        n = len(c["functions"]) * c["N"]
        assert e["mean"].shape == (n,) and np.all(e["mean_scale"] > 0) and np.all(e["cov_scale"] > 0)
        assert (len(ri) == n * n) == (n <= jr.FULL_MAX)
    assert os.path.getsize(jr.GRID) < 1024 * 1024


@pytest.mark.parametrize("strict", [False, True], ids=["default", "strict"])
def test_restatement_against_the_grid(restated, strict):
    worst = {"mean": 0.0, "cov": 0.0}
    for n in NAMES:
        rm, rc = jr.case_ratios(GRID[n], *restated[(n, strict)])
        print("%-7s mean %.3f cov %.3f" % (n, rm, rc))
        worst["mean"], worst["cov"] = max(worst["mean"], rm), max(worst["cov"], rc)
    for what in ("mean", "cov"):
        assert worst[what] <= jr.c_oracle(what), (what, worst[what])
        assert worst[what] > jr.c_oracle(what) / 64.0 or jr.c_oracle(what) == 1.0, "C_ORACLE is not the measured figure any more"


def test_grid_regenerates_on_a_subset():
    import joint_ref_mp as jm
    rng = np.random.RandomState(3)
    for n in jr.REGEN_CASES:
        e = GRID[n]
        pick = rng.choice(len(e["ri"]), min(12, len(e["ri"])), replace=False)
        ref = jm.reference(e["prm"], e["Xnew"], e["case"]["functions"], e["ri"][pick], e["ci"][pick])
        assert np.array_equal(ref["mean"], e["mean"]) and np.array_equal(ref["mean_scale"], e["mean_scale"]), n
        assert np.array_equal(ref["cov"], e["cov"][pick]) and np.array_equal(ref["cov_scale"], e["cov_scale"][pick]), n


def test_a_moved_result_is_caught(restated):
    """An entry off by 2 C 2^-52 scale fails the device's criterion, whichever entry it is."""
    for n in ("s_N1", "s_N63", "r_N65"):
        e = GRID[n]
        mean, cov = restated[(n, False)]
        for what, C_ in (("mean", jr.c_kernel("mean")), ("cov", jr.c_kernel("cov"))):
            rm0, rc0 = jr.case_ratios(e, mean, cov)
            assert (rm0 if what == "mean" else rc0) <= C_
            k = len(e[what]) // 2
            if what == "mean":
                moved = e["mean"].copy()
                moved[k] += 2.0 * C_ * jr.EPS * e["mean_scale"][k]
                assert np.max(jr.ratios(moved, e["mean"], e["mean_scale"])) > C_
            else:
                moved = np.array(cov)
                moved[e["ri"][k], e["ci"][k]] = e["cov"][k] + 2.0 * C_ * jr.EPS * e["cov_scale"][k]
                assert jr.case_ratios(e, mean, moved)[1] > C_
    bad = np.array(GRID["s_N1"]["mean"])
    bad[0] = np.nan
    assert np.isinf(np.max(jr.ratios(bad, GRID["s_N1"]["mean"], GRID["s_N1"]["mean_scale"])))


@pytest.mark.parametrize("name", NAMES)
def test_covariance_properties(restated, name):
    e = GRID[name]
    d = list(e["case"]["functions"])
    for strict in (False, True):
        mean, cov = restated[(name, strict)]
        assert np.array_equal(cov, cov.T)
        m, v = jr.predict_f(e["prm"], e["Xnew"])
        _, _, sm, sc = jr.joint(e["prm"], e["Xnew"], d, strict=strict, return_scale=True)
        # the diagonal is q(f)'s variance (before any abs), the mean q(f)'s mean: two float64 evaluations of one formula
        assert np.max(jr.ratios(np.diag(cov), v[:, d].T.ravel(), np.diag(sc))) <= 2.0 * jr.c_oracle("cov")
        assert np.max(jr.ratios(mean, m[:, d].T, sm)) <= 2.0 * jr.c_oracle("mean")
        L, jit, rung = jr.jitchol(cov)
        assert rung >= -1 and np.all(np.isfinite(L)) and np.all(np.diag(L) > 0)
        assert np.min(np.linalg.eigvalsh(cov + jit * np.eye(cov.shape[0]))) > 0.0
        assert jr.chol_backward(cov, L, jit) <= jr.C_CHOL_LAPACK


def test_sampler_restatement():
    e = GRID["s_N65"]
    mean, cov = jr.joint(e["prm"], e["Xnew"], e["case"]["functions"])
    F8, L, jit, rung = jr.sample(mean.ravel(), cov, 8, seed=3)
    F3 = jr.sample(mean.ravel(), cov, 3, seed=3)[0]
    assert np.array_equal(F8[:3], F3)                       # draw s does not depend on how many draws were asked for
    assert not np.array_equal(jr.sample(mean.ravel(), cov, 3, seed=4)[0], F3)
    z = jr.normals(3, cov.shape[0], 8)
    import mclp_ref as mr
    assert z[5, 17] == mr.normal_pair(3, 17, 5, 0)[0]


def test_singular_case_on_the_cpu():
    """Two identical rows: the ladder is taken, and the restatement's twin coordinates stay within 8 sqrt(2 jitter) for the seed the GPU test fixes."""
    prm, Xnew, d = jr.singular_case()
    mean, cov = jr.joint(prm, Xnew, d)
    F, L, jit, rung = jr.sample(mean.ravel(), cov, jr.SINGULAR_DRAWS, jr.SINGULAR_SEED)
    assert rung >= 0 and jit > 0.0 and np.all(np.isfinite(F))
    N = Xnew.shape[0]
    F = F.reshape(jr.SINGULAR_DRAWS, len(d), N)
    gap = max(np.max(np.abs(F[:, :, a] - F[:, :, b])) for a, b in jr.SINGULAR_TWINS)
    print("twin gap %.3e, bound %.3e" % (gap, 8.0 * np.sqrt(2.0 * jit)))
    assert gap <= 8.0 * np.sqrt(2.0 * jit)


def test_statistical_thresholds_hold_for_the_restatement():
    """The thresholds of the GPU suite's statistical check, applied to the restatement's own draws (same seed)."""
    prm, Xnew, d = jr.stat_case()
    mean, cov = jr.joint(prm, Xnew, d)
    F = jr.sample(mean.ravel(), cov, jr.STAT_DRAWS, jr.STAT_SEED)[0]
    zm, zc = jr.stat_zscores(F, mean.ravel(), cov)
    t = jr.stat_threshold(cov.shape[0])
    print("max |z| mean %.2f cov %.2f threshold %.2f" % (zm, zc, t))
    assert zm <= t and zc <= t


def test_abi_symbols_and_refusals_without_a_device():
    """The two symbols exist, the ABI version stays 8, and a NULL handle is refused on the host: no device is asked for."""
    from hetmogp_amd import _lib
    assert _lib.ABI_VERSION == 8 and _lib.lib.hmogp_abi_version() == 8
    assert "hmogp_predict_f_joint" in _lib.EXPORTS and "hmogp_sample_f_joint" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "hetmogp_hip.h")).read()
    assert "hmogp_predict_f_joint(" in header and "hmogp_sample_f_joint(" in header and "#define HMOGP_JOINT_MAXDIM 8192" in header
    assert "#define HMOGP_ABI_VERSION 8" in header and _lib.JOINT_MAXDIM == 8192
    X = np.zeros((2, 1))
    d = np.zeros(1, dtype=np.int32)
    mean, cov, F = np.zeros(2), np.zeros((2, 2)), np.zeros((1, 2))
    p = lambda a: a.ctypes.data_as(_lib.c_double_p)
    dp = d.ctypes.data_as(_lib.c_int32_p)
    assert _lib.lib.hmogp_predict_f_joint(None, p(X), 2, 1, dp, p(mean), p(cov)) == _lib.E_INVALID
    jit, rung = C.c_double(0.0), C.c_int32(0)
    assert _lib.lib.hmogp_sample_f_joint(None, p(X), 2, 1, dp, 1, 0, p(F), None, None, C.byref(jit), C.byref(rung)) == _lib.E_INVALID
    # the refusals sit in front of the first device call: in the source, every throw of hmogp_engine::joint's checks precedes hipSetDevice
    src = open(os.path.join(ROOT, "hetmogp_amd", "csrc", "engine_optim.hip")).read()
    body = src[src.index("void hmogp_engine::joint("):]
    first_device = body.index("hipSetDevice")
    for msg in ("no evaluation to predict from", "nD must be >= 1", "out of range", "repeated", "exceeds HMOGP_JOINT_MAXDIM", "S must be >= 1",
                "bad predict arguments"):
        assert 0 <= body.index(msg) < first_device, msg
    assert body.index("if (Nnew == 0) return;") < first_device
