"""CPU: the extended-precision criterion of the natural-gradient step (tests/natgrad_ref.py) against its plain float64
restatement, and the NumPy restatement of `adadelta_kernel` against the host optimiser.
  (a) every step the GPU test accepts has lambda_min(Lambda) > 0 in the longdouble reference (the same list, natgrad_ref.CASES), the
      refused step has one latent on each side of the cone, and the graded case reaches cond(Lambda) >= 1e6;
  (b) `step_f64` stays within C_ORACLE on every case, the graded one included, no element is held only by the floor, and C_ORACLE is
      the re-measured maximum;
  (c) the criterion rejects seven corruptions of the restatement's own output, each what an indexing or sign error in a kernel of the
      step would leave behind (arithmetic on arrays: nothing is run wrongly);
  (d) the Adadelta restatement gives the bits of `hetmogp_amd.util.Adadelta`."""
import numpy as np
import pytest

import natgrad_ref as nr
import tail_cases as tc


@pytest.fixture(scope="module")
def refs():
    return tc.references()


_BASE, _STEP = {}, {}


def _reference(refs, tag, gamma):
    if tag not in _BASE:
        inp = nr.cpu_inputs(refs, tag)
        _BASE[tag] = (inp, nr.base(*inp))
    inp, b = _BASE[tag]
    return inp, nr.at_gamma(b, gamma)


def _measure(refs, tag, gamma):
    """(inputs, reference, (m_new, L_flat_new) of `step_f64`, worst ratios with B = 0)."""
    if (tag, gamma) not in _STEP:
        inp, ref = _reference(refs, tag, gamma)
        got = nr.step_f64(*inp, gamma)
        _STEP[(tag, gamma)] = (inp, ref, got, nr.worst_ratios(ref, got[0], got[1], nr.C_ORACLE, with_B=False))
    return _STEP[(tag, gamma)]


# ================================================================================================ (a) the cases
@pytest.mark.parametrize("tag,gamma", nr.CASES)
def test_accepted_steps_stay_inside_the_cone(refs, tag, gamma):
    _, ref = _reference(refs, tag, gamma)
    print("[natgrad] %-7s gamma = %-5g lambda_min(Lambda) = %s   cond(Lambda) = %s" % (
        tag, gamma, " ".join("%.4g" % u["lam_min"] for u in ref), " ".join("%.4g" % u["cond"] for u in ref)))
    assert all(u["lam_min"] > 0 for u in ref), [u["lam_min"] for u in ref]
    if tag == "graded":
        assert all(u["cond"] >= 1e6 for u in ref), [u["cond"] for u in ref]


def test_refused_step_has_one_latent_on_each_side(refs):
    tag, gamma = nr.REFUSED
    inp, ref = _reference(refs, tag, gamma)
    print("[natgrad] refused %s gamma = %g: lambda_min = %s, cond = %s" % (tag, gamma, [u["lam_min"] for u in ref], [u["cond"] for u in ref]))
    assert ref[0]["lam_min"] > 0 and 100 < ref[0]["cond"] < 1000
    assert -1.0 < ref[1]["lam_min"] < -0.1
    with pytest.raises(np.linalg.LinAlgError):
        nr.step_f64(*inp, gamma)


# ================================================================================================ (b) the constants
@pytest.mark.parametrize("tag,gamma", nr.CASES)
def test_restatement_within_c_oracle(refs, tag, gamma):
    inp, ref, (m1, L1), _ = _measure(refs, tag, gamma)
    nr.check("f64 %s gamma=%g" % (tag, gamma), ref, m1, L1, nr.C_ORACLE, with_B=False)
    nr.check("f64 %s gamma=%g (with B)" % (tag, gamma), ref, m1, L1, nr.c_kernel())
    nr.assert_scales_dense("%s gamma=%g" % (tag, gamma), ref, m1, L1)


def test_c_oracle_is_the_remeasured_maximum(refs):
    worst = {k: 0.0 for k in nr.KINDS}
    for tag, gamma in nr.CASES:
        w = _measure(refs, tag, gamma)[3]
        print("[natgrad] f64 %-7s gamma = %-5g %s" % (tag, gamma, " ".join("%s %.3g" % (k, w[k][0]) for k in nr.KINDS)))
        for k in nr.KINDS:
            worst[k] = max(worst[k], w[k][0])
    measured = {k: nr.next_pow2(worst[k]) for k in nr.KINDS}
    print("[natgrad] C_ORACLE re-measured:", measured)
    ck = nr.c_kernel()
    for k in nr.KINDS:
        assert measured[k] <= nr.C_ORACLE[k] <= 2.0 * measured[k], (k, worst[k], nr.C_ORACLE[k])      # (never below the measurement)
        assert ck[k] == max(16.0, 4.0 * nr.C_ORACLE[k])


# ================================================================================================ (c) sharpness
def _ratios(ref, m1, L1):
    return {k: w[0] for k, w in nr.worst_ratios(ref, m1, L1, nr.c_kernel()).items()}


def test_criterion_rejects_corruptions(refs):
    """Each corruption pushes some element of the kind it is listed with beyond C_KERNEL (and `check` raises); the uncorrupted output
    of the same case passes."""
    CK = nr.c_kernel()
    seen = []

    def judge(what, tag, gamma, m1, L1, kinds):
        _, ref = _reference(refs, tag, gamma)
        r = _ratios(ref, m1, L1)
        seen.append((what, tag, kinds, r))
        for k in kinds:
            assert r[k] > CK[k], (what, k, r[k])
        with pytest.raises(AssertionError):
            nr.check("corrupted: " + what, ref, m1, L1, CK)

    tag, gamma = "T65", 0.1
    inp, ref, (m1, L1), _ = _measure(refs, tag, gamma)
    M = ref[0]["M"]
    nr.check("uncorrupted %s" % tag, ref, m1, L1, CK)

    bad = nr.step_f64(*inp, gamma, reversed_route=False)
    judge("1 un-reversed route: the inverse of the factor of Lambda itself, no anti-transpose", tag, gamma, bad[0], bad[1], ("ng_chol",))

    judge("2a the two latents' columns of L_flat_new swapped", tag, gamma, m1, L1[:, ::-1], ("ng_chol",))
    judge("2b the two latents' columns of m_new swapped", tag, gamma, m1[:, ::-1], L1, ("ng_mean",))

    Ls = nr.unpack(L1, M)
    Ls[1][M - 1, :] = 0.0
    Ls[1][:, M - 1] = 0.0
    judge("3 last row and last column of L^ of latent 1 left at zero", tag, gamma, m1, nr.pack(Ls), ("ng_chol",))
    assert not nr.diag_ok(nr.pack(Ls), M)

    gi, gref, (gm1, gL1), _ = _measure(refs, "graded", nr.GRADED_GAMMA)
    Ls = nr.unpack(gL1, M)
    row = int(np.argmin(np.abs(Ls[0]).max(1)))
    col = int(np.argmax(np.abs(Ls[0][row])))
    assert np.abs(Ls[0][row]).max() <= 2.0 ** -8 * np.abs(Ls[0]).max()
    Ls[0][row, col] *= 1.0 + 1e-3
    rel = abs(Ls[0][row, col]) * 1e-3 / np.abs(Ls[0]).max()
    print("[natgrad] corruption 4 moves L^[%d, %d] by %.3g of max|L^|: below 1e-5 of the array norm" % (row, col, rel))
    assert rel < 1e-5
    judge("4 one element of a small-magnitude row off by 1e-3 relative", "graded", nr.GRADED_GAMMA, gm1, nr.pack(Ls), ("ng_chol",))

    bad = nr.step_f64(*inp, gamma, theta_dlds=False)
    assert np.array_equal(bad[1], L1)
    judge("5 theta1 without - 2 dL_dS m", tag, gamma, bad[0], bad[1], ("ng_mean",))

    bad = nr.step_f64(*inp, gamma, lam_factor=1.0)
    judge("6 gamma for 2 gamma in Lambda", tag, gamma, bad[0], bad[1], ("ng_chol",))

    for t in ("T65", "T33"):
        i2, r2, (a1, b1), _ = _measure(refs, t, gamma)
        Mt = r2[0]["M"]
        bad = nr.step_f64(*i2, gamma, gemv_t_rows=16 * (Mt // 16))
        assert np.array_equal(bad[1], b1)
        judge("7 gemv_t without the rows i >= 16 floor(M / 16)", t, gamma, bad[0], bad[1], ("ng_mean",))

    for what, tag, kinds, r in seen:
        print("[natgrad] corruption %-82s %-7s %s" % (what, tag, " ".join("%s %.3g = %.3g x C_KERNEL" % (k, r[k], r[k] / CK[k]) for k in kinds)))


# ================================================================================================ (d) Adadelta
def _grad(w, it):
    """A fixed seeded function of wrt (and of the iteration, so that no two evaluations agree)."""
    return np.sin(3.0 * w + 0.1 * it) * _SCALE + 0.25 * w


N_ADA = 70000
_SCALE = np.exp(np.random.RandomState(11).randn(N_ADA))


@pytest.mark.parametrize("momentum", [0.9, 0.0])
def test_adadelta_restatement_is_the_host_optimiser(momentum):
    """Five iterations on n = 70 000 (more than one cache block of util.Adadelta) + the evaluation point of a sixth: bit-identical at
    every evaluation point and at the end, after the closing half-step.  Iteration 2 withholds its gradient (grad=None; the host
    optimiser is handed zeros): it moves x by step1 only."""
    from hetmogp_amd.util import Adadelta
    assert N_ADA > Adadelta._BLOCK
    rate, decay, offset, withheld = 1.0, 0.9, 1e-4, 2
    x0 = np.random.RandomState(12).randn(N_ADA)
    points, grads = [], []

    def fprime(w):
        it = len(points)
        points.append(w.copy())
        g = None if it == withheld else _grad(w, it)
        grads.append(g)
        return np.zeros_like(w) if g is None else -g          # (the optimiser descends along fprime; the engine hands over +grad)

    wrt = x0.copy()
    opt = Adadelta(wrt, fprime, step_rate=rate, decay=decay, momentum=momentum, offset=offset)
    it = iter(opt)
    ends = []
    for _ in range(6):
        next(it)
        ends.append(wrt.copy())

    s = nr.adadelta_state(x0)
    args = (rate, momentum, decay, float(1 - decay), offset)
    for i in range(6):
        before = s["x"].copy()
        pend, step = s["pend"].copy(), s["step"].copy()
        nr.adadelta_phase(s, 0, None, *args)
        assert np.array_equal(s["x"], points[i]), ("evaluation point", i)
        assert not s["pend"].any()
        if i == withheld + 1:
            assert not pend.any() and np.array_equal(s["x"], before - step * momentum), "a withheld gradient moves x by step1 only"
        nr.adadelta_phase(s, 1, grads[i], *args)
        assert np.array_equal(s["x"], points[i]), "phase 1 leaves x at the evaluation point"
        assert np.array_equal(s["x"] - s["pend"], ends[i]), ("after the closing half-step", i)
    assert np.array_equal(s["gms"], opt.gms) and np.array_equal(s["sms"], opt.sms) and np.array_equal(s["step"], opt.step)
    assert len({p.tobytes() for p in points}) == (6 if momentum else 5)      # (without momentum the withheld iteration stands still)
