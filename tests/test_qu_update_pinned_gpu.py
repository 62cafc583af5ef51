"""GPU: the two updates that WRITE the resident q(u) on the device, pinned.

Natural-gradient step (`hmogp_natgrad_step`, `hmogp_qu_natgrad`, `hmogp_qu_natgrad_async`: `natgrad_prec_kernel` reversed, `gemv_kernel`,
`natgrad_theta1_kernel`, potrf and trtri on J Lambda J, `antitranspose_kernel`, `gemv_t_kernel`, `pack_tril_kernel`, `scatter_mq_kernel`,
`commit_if_ok_kernel`): element by element against the extended-precision restatement of tests/natgrad_ref.py,

    |quantity| <= 2^-52 (C_KERNEL[kind] S + B)      kinds ng_chol, ng_mean, and the condition ng_diag,

on the tail-only shapes of tests/tail_cases.py with an injected dense bundle, on the small-model shapes end to end on both paths, and
on T65 with the rows of L graded by powers of two (cond(Lambda) >= 1e6).  The reference is fed what the evaluation exported (dL_dS,
g_m_u): byte copies of what the step reads.  The three entry points agree bit for bit at ragged M and Q = 2; a step that would leave the
cone in ONE latent commits nothing in either; the grid-stride loops of `commit_if_ok_kernel` and `adadelta_kernel` run at M = 1024.

Adadelta (`hmogp_qu_adadelta`: `adadelta_kernel`): after every phase 0 the resident q(u) has the bits of the NumPy restatement
(natgrad_ref.adadelta_phase) fed the gradients each evaluation exported.

Every accepted step prints its worst ratios as `[natgrad] <case> <kind> ...`."""
import ctypes as C

import numpy as np
import pytest

import natgrad_ref as nr
import rowpass_cases as rc
import tail_cases as tc
from test_tail_pinned_gpu import make_engine, params

pytestmark = pytest.mark.gpu

ADADELTA = dict(rate=1.0, decay=0.9, offset=1e-4)          # DeviceAdadelta's defaults
OUTPUTS = ("elbo", "kl", "g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z")


@pytest.fixture(scope="module")
def refs():
    return tc.references()


def evaluate(e, case, want_dL_dS=False, resident=False, **kw):
    """hmogp_elbo_grad with g_m_u and g_L_u exported also when q(u) is resident (m_u = L_flat = NULL): `Engine.elbo_grad` leaves them
    in HBM then, the C ABI copies them out wherever it is given the arrays."""
    from hetmogp_amd._lib import check, lib
    args = params(case, **kw)
    if resident:
        args.update(m_u=None, L_flat=None)
    p, keep = e._params(**args)
    c, o = e._outputs(want_dL_dS, skip_qu=False)
    check(lib.hmogp_elbo_grad(e._h, C.byref(p), C.byref(c)), e._h)
    out = e._wrap(o)
    assert out["rungs"] == case[4]
    return out


def inject(e, case, bundle, resident=False):
    """hmogp_step_begin -> the dense bundle in place of the row pass's -> hmogp_step_finish with dL_dS (test_tail_pinned_gpu.split_step)."""
    e.step_begin(**(params(case, m_u=None, L_flat=None) if resident else params(case)))
    e.stats_write(np.asarray(bundle, dtype=np.float64))
    out = e.step_finish(want_dL_dS=True)
    assert out["rungs"] == case[4]
    return out


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def big_case():
    """M = 1024, Q = 2, one 17-row Gaussian task: the recipe of the tail-only shapes.  Mtri Q = 1 049 600 > 4096 * 256 elements
    (`adadelta_kernel`'s grid) and M Q + Mtri Q > 2048 * 256 (`commit_if_ok_kernel`'s)."""
    from model_cases import synth
    M = 1024
    prm, prob, X, Y = synth(50 + M, rc.SPECS[:1], [17], M, 2, 1, (16.0, 100.0))
    assert prob["specs"][0][0] == "Gaussian"
    prm["m_u"] = 0.1 * prm["m_u"]
    return prm, prob, X, Y, [rc.RUNG] * 2


# ================================================================================================ natural-gradient step
def pinned_steps(e, case, what, evaluation):
    """For each gamma: evaluation + step twice (same bits), then the element criterion against the reference of what was exported."""
    prm = case[0]
    base, first = None, None
    for gamma in nr.GAMMAS if what != "graded" else (nr.GRADED_GAMMA,):
        runs = []
        for _ in range(2):
            out = evaluation()
            runs.append((np.array(out["dL_dS"], copy=True), np.array(out["g_m_u"], copy=True)) + e.natgrad_step(gamma))
        assert same(runs[0], runs[1]), (what, gamma, "a second identical evaluation and step gives other bits")
        if base is None:
            first, base = runs[0], nr.base(prm["m_u"], prm["L_flat"], runs[0][0], runs[0][1])
        assert same(first[:2], runs[0][:2])
        ref = nr.at_gamma(base, gamma)
        assert all(u["lam_min"] > 0 for u in ref)
        nr.check("%s gamma=%g" % (what, gamma), ref, runs[0][2], runs[0][3], nr.c_kernel())
        yield gamma, runs[0][2:]


@pytest.mark.parametrize("tag", nr.REGULAR)
def test_step_on_the_regular_path(refs, tag):
    o, case = refs[tag]["default"], refs[tag]["case"]
    e = make_engine(case)
    try:
        assert len(list(pinned_steps(e, case, tag, lambda: inject(e, case, o["bundle"])))) == len(nr.GAMMAS)
    finally:
        e.close()


def test_step_with_graded_factor(refs):
    """T65 with the rows of L scaled by 2^e, e in [-10, 0]: cond(Lambda) >= 1e6 (asserted on the CPU), the same constants."""
    o, case = refs[nr.GRADED]["default"], refs[nr.GRADED]["case"]
    Lf, _ = nr.graded_L_flat(case[0]["L_flat"], case[1]["M"])
    case = (dict(case[0], L_flat=Lf),) + tuple(case[1:])
    e = make_engine(case)
    try:
        assert len(list(pinned_steps(e, case, "graded", lambda: inject(e, case, o["bundle"])))) == 1
    finally:
        e.close()


@pytest.mark.parametrize("small_path", [True, False])
@pytest.mark.parametrize("tag", nr.SMALL)
def test_step_on_small_model_shapes(refs, tag, small_path):
    """M = 33, 50, 64 end to end through hmogp_elbo_grad, on the fused small-model kernels (witness: only that path captures a
    hipGraph) and on the regular ones.  The step taken from a REPLAYED evaluation has the bits of the step taken from the evaluation
    that exported dL_dS (which is never captured)."""
    case = refs[tag]["case"]
    e = make_engine(case, small_path=small_path)
    try:
        for _ in range(3):
            e.elbo_grad(**params(case))
        stats = e.graph_stats()
        assert (stats[0] >= 1) if small_path else (stats == (0, 0)), stats
        replayed = e.natgrad_step(nr.GAMMAS[0])
        what = "%s small_path=%s" % (tag, small_path)
        steps = dict(pinned_steps(e, case, what, lambda: e.elbo_grad(want_dL_dS=True, **params(case))))
        assert same(replayed, steps[nr.GAMMAS[0]])
    finally:
        e.close()


# ================================================================================================ the three entry points
@pytest.mark.parametrize("tag", ["T65", "S50"])
def test_entry_points_agree_bit_for_bit(refs, tag):
    case = refs[tag]["case"]
    prm, gamma = case[0], 0.1
    host, sync, asyn, fresh = es = [make_engine(case) for _ in range(4)]
    try:
        out0 = host.elbo_grad(**params(case))
        m1, L1 = host.natgrad_step(gamma)
        assert not np.array_equal(m1, prm["m_u"]) and not np.array_equal(L1, prm["L_flat"])
        for e in (sync, asyn):
            e.qu_load(prm["m_u"], prm["L_flat"])
            assert e.elbo_grad(**params(case, m_u=None, L_flat=None))["elbo"] == out0["elbo"]
        sync.qu_natgrad(gamma)
        assert same(sync.qu_read(), (m1, L1))
        asyn.qu_natgrad_async(gamma)
        assert asyn.qu_natgrad_status() is True
        assert same(asyn.qu_read(), (m1, L1))
        want = evaluate(fresh, case, m_u=m1, L_flat=L1)
        for e in (sync, asyn):
            got = evaluate(e, case, resident=True)
            for k in OUTPUTS:
                assert np.array_equal(got[k], want[k]), (tag, k)
    finally:
        for e in es:
            e.close()


def test_refusal_is_all_or_nothing(refs):
    """T33 at gamma = 1: latent 0 stays positive definite (cond about 245), latent 1 does not (lambda_min about -0.51; both asserted on the
    CPU).  Nothing is committed for EITHER latent.  hmogp_natgrad_step and hmogp_qu_natgrad retry at gamma = 0.1 without a new
    evaluation; the asynchronous entry point gives its evaluation up when it is enqueued (include/hetmogp_hip.h), so its retry follows
    the same evaluation run again."""
    tag, gamma = nr.REFUSED
    o, case = refs[tag]["default"], refs[tag]["case"]
    prm = case[0]
    host, sync, asyn = es = [make_engine(case) for _ in range(3)]
    try:
        out = inject(host, case, o["bundle"])
        ref = nr.reference(prm["m_u"], prm["L_flat"], out["dL_dS"], out["g_m_u"], gamma)
        assert ref[0]["lam_min"] > 0 > ref[1]["lam_min"], [u["lam_min"] for u in ref]
        with pytest.raises(np.linalg.LinAlgError):
            host.natgrad_step(gamma)
        m1, L1 = host.natgrad_step(0.1)
        ref = nr.reference(prm["m_u"], prm["L_flat"], out["dL_dS"], out["g_m_u"], 0.1)
        nr.check("T33 natgrad_step after a refusal", ref, m1, L1, nr.c_kernel())

        for e in (sync, asyn):
            e.qu_load(prm["m_u"], prm["L_flat"])
            assert np.array_equal(inject(e, case, o["bundle"], resident=True)["dL_dS"], out["dL_dS"])
        with pytest.raises(np.linalg.LinAlgError):
            sync.qu_natgrad(gamma)
        assert same(sync.qu_read(), (prm["m_u"], prm["L_flat"]))
        sync.qu_natgrad(0.1)
        got = sync.qu_read()
        nr.check("T33 qu_natgrad after a refusal", ref, got[0], got[1], nr.c_kernel())
        assert same(got, (m1, L1))

        asyn.qu_natgrad_async(gamma)
        assert asyn.qu_natgrad_status() is False
        assert same(asyn.qu_read(), (prm["m_u"], prm["L_flat"]))
        inject(asyn, case, o["bundle"], resident=True)
        asyn.qu_natgrad_async(0.1)
        assert asyn.qu_natgrad_status() is True
        got = asyn.qu_read()
        nr.check("T33 qu_natgrad_async after a refusal", ref, got[0], got[1], nr.c_kernel())
        assert same(got, (m1, L1))
    finally:
        for e in es:
            e.close()


# ================================================================================================ grid-stride loops, M = 1024
@pytest.fixture(scope="module")
def big():
    return big_case()


def test_async_commit_at_M1024_equals_the_synchronous_step(big):
    prm = big[0]
    sync, asyn = es = [make_engine(big) for _ in range(2)]
    try:
        for e in es:
            e.qu_load(prm["m_u"], prm["L_flat"])
            e.elbo_grad(**params(big, m_u=None, L_flat=None))
        sync.qu_natgrad(0.1)
        asyn.qu_natgrad_async(0.1)
        assert asyn.qu_natgrad_status() is True
        a, b = sync.qu_read(), asyn.qu_read()
        assert same(a, b)
        assert not np.any(a[0] == prm["m_u"]) and np.mean(a[1] == prm["L_flat"]) < 0.01       # (every part of both arrays moved)
        assert nr.diag_ok(a[1], 1024)
    finally:
        for e in es:
            e.close()


# ================================================================================================ Adadelta
def adadelta_iterations(e, case, momentum, n, hyper_at=None):
    """n iterations of phase 0 -> evaluation on the resident q(u) -> phase 1, then one more phase 0 (the closing half-step), on the
    engine and on the restatement; the resident q(u) is compared after every phase 0.  Returns the n + 1 reads."""
    from hetmogp_amd import _lib
    prm = case[0]
    rate, decay, offset = ADADELTA["rate"], ADADELTA["decay"], ADADELTA["offset"]
    args = (rate, momentum, decay, float(1 - decay), offset)
    e.qu_load(prm["m_u"], prm["L_flat"])
    sm, sL = nr.adadelta_state(prm["m_u"]), nr.adadelta_state(prm["L_flat"])
    reads = []

    def phase0(i):
        e.qu_adadelta(0, rate, momentum, decay, offset)
        nr.adadelta_phase(sm, 0, None, *args), nr.adadelta_phase(sL, 0, None, *args)
        m, L = e.qu_read()
        assert np.array_equal(m.reshape(-1), sm["x"]), ("m_u after phase 0 of iteration", i)
        assert np.array_equal(L.reshape(-1), sL["x"]), ("L_flat after phase 0 of iteration", i)
        reads.append((m, L))

    for i in range(n):
        phase0(i)
        hyper = i == hyper_at
        out = evaluate(e, case, resident=True, group_mask=_lib.GROUP_HYPER if hyper else _lib.GROUP_ALL)
        if hyper:
            assert not out["g_m_u"].any() and not out["g_L_u"].any()
        else:
            assert out["g_m_u"].all() and out["g_L_u"].any()
        e.qu_adadelta(1, rate, momentum, decay, offset)
        nr.adadelta_phase(sm, 1, None if hyper else out["g_m_u"], *args)
        nr.adadelta_phase(sL, 1, None if hyper else out["g_L_u"], *args)
    phase0(n)
    return reads


def _adadelta(case, small_path, momentum):
    e = make_engine(case, small_path=small_path)
    try:
        reads = adadelta_iterations(e, case, momentum, 5, hyper_at=2)
        assert same(reads[0], (case[0]["m_u"], case[0]["L_flat"]))          # (the first phase 0 has nothing pending and no momentum yet)
        for i in range(5):
            # x moves with every iteration, except that a withheld gradient moves it by step1 = momentum * step only
            still = i == 2 and momentum == 0.0
            assert np.array_equal(reads[i + 1][0], reads[i][0]) == still and np.array_equal(reads[i + 1][1], reads[i][1]) == still, i
        again = adadelta_iterations(e, case, momentum, 1)          # hmogp_qu_load resets the accumulators
        assert same(again[0], reads[0]) and same(again[1], reads[1])
    finally:
        e.close()


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("tag,small_path", [("T65", True), ("S50", True), ("S50", False)])
def test_adadelta_is_the_restated_recurrence(refs, tag, small_path, momentum):
    _adadelta(refs[tag]["case"], small_path, momentum)


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_adadelta_at_M1024(big, momentum):
    _adadelta(big, True, momentum)
