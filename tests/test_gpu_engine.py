"""GPU: parity of the whole hot path (hmogp_elbo_grad through the C ABI) against
  * the golden vectors captured from the reference's own Python (tests/golden/inf_*.npz, model_*.npz), and
  * the NumPy oracle on seeded inputs at sizes it finishes in seconds,
plus size-independent properties at larger sizes (row-chunk invariance, shard additivity, gating).
Tolerance: BASELINE.json's north-star states 1e-5 relative for ELBO and gradients; these tests hold the engine
to 1e-8 (relative to the largest magnitude of each array) on the well-conditioned fixtures."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, elementwise_excess, rel_norm as rel
from model_cases import KEYS, make_engine, run, synth

pytestmark = pytest.mark.gpu

TOL = 1e-8


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "model_*.npz"))), ids=os.path.basename)
def test_engine_vs_reference_parameters_changed(path):
    """model_*.npz: outputs of the reference's SVMOGP.parameters_changed (svmogp.py:85-166), incl. SVI gating
    (E-step / M-step) and the stale-W chain factors (quirk Q3)."""
    from oracle import svmogp_oracle as so
    from hetmogp_amd import _lib
    g = np.load(path)
    prm, prob, X, Y, bs = so.load_case(g)
    mask = _lib.GROUP_ALL
    if bool(g["stochastic"]):
        mask = _lib.GROUP_QU if bool(g["vem_step"]) else (_lib.GROUP_HYPER | _lib.GROUP_Z)
    e = make_engine(prob, X, Y)
    out = run(e, prm, bs, group_mask=mask)
    assert out["rungs"] == [-1] * prob["Q"]
    for k in KEYS:
        assert rel(out[k], g[k]) < TOL, k
        assert elementwise_excess(out[k], g[k]) <= 1.0, (k, "element-wise 1e-5")


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "inf_*.npz"))), ids=os.path.basename)
def test_engine_vs_reference_inference(path):
    """inf_*.npz: ELBO / raw gradients of the reference's SVMOGPInf.inference (svmogp_inf.py:23-109); the raw dict is
    reduced to parameter gradients by the oracle's literal assembly (pinned by the model_* fixtures)."""
    from oracle import svmogp_oracle as so
    g = np.load(path)
    prm, prob, X, Y, bs = so.load_case(g)
    e = make_engine(prob, X, Y)
    out = run(e, prm, bs)
    assert rel(out["elbo"], g["elbo"]) < TOL
    assert rel(out["KL"], g["KL"]) < TOL          # calculate_KL on its own (svmogp_inf.py:227-250), not only through the ELBO
    Q, Df = prob["Q"], prob["Df"]
    assert rel(out["g_m_u"], np.hstack([g["dL_dmu_u_%d" % q] for q in range(Q)])) < TOL
    assert rel(out["g_L_u"], np.hstack([g["dL_dL_u_%d" % q] for q in range(Q)])) < TOL
    grads = dict(dL_dmu_u=[g["dL_dmu_u_%d" % q] for q in range(Q)], dL_dL_u=[g["dL_dL_u_%d" % q] for q in range(Q)],
                 dL_dKmm=[g["dL_dKmm_%d" % q] for q in range(Q)],
                 dL_dKmn=[[g["dL_dKmn_%d_%d" % (q, d)] for d in range(Df)] for q in range(Q)],
                 dL_dKdiag=[[g["dL_dKdiag_%d_%d" % (q, d)] for d in range(Df)] for q in range(Q)])
    want = so.assemble_literal(prm, prob, X, grads)
    for k in KEYS[1:]:
        assert rel(out[k], want[k]) < TOL, k
        assert elementwise_excess(out[k], want[k]) <= 1.0, (k, "element-wise 1e-5")
    # q(f) through the prediction entry point at the training inputs (svmogp_inf.py:212-218)
    for t in range(prob["T"]):
        m, v = e.predict_f(X[t])
        for d in range(Df):
            if prob["f_index"][d] == t:
                assert rel(m[:, d], g["m_fd_%d" % d][:, 0]) < TOL
                assert rel(v[:, d], g["v_fd_%d" % d][:, 0]) < TOL
                assert elementwise_excess(m[:, d], g["m_fd_%d" % d][:, 0]) <= 1.0
                assert elementwise_excess(v[:, d], g["v_fd_%d" % d][:, 0]) <= 1.0


def test_engine_vs_oracle_multitile():
    """M = 300 (3 x 3 GEMM tiles, ragged), several row chunks, all eight likelihoods, batch scales."""
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {}), ("HetGaussian", {}),
             ("Beta", {}), ("Exponential", {}), ("Categorical", {"K": 3})]
    Ns = [700, 513, 400, 333, 256, 300, 129, 257]
    prm, prob, X, Y = synth(11, specs, Ns, 300, 3, 1, (0.8, 1.0, 1.3))
    bs = [1.0 + 0.5 * t for t in range(len(specs))]
    want = so.elbo_grad_fused(prm, prob, X, Y, bs)
    assert want["rungs"] == [-1, -1, -1]
    e = make_engine(prob, X, Y, chunk_rows=256)
    out = run(e, prm, bs)
    assert out["rungs"] == want["rungs"]
    for k in KEYS:
        assert rel(out[k], want[k]) < TOL, k
    wv, wi = e.posterior_u()
    u = so.u_algebra(prm, prob)
    for q in range(3):
        assert rel(wv[q], u["a"][q]) < TOL and rel(wi[q], -u["C"][q]) < TOL


def test_engine_2d_inputs_vs_oracle():
    from oracle import svmogp_oracle as so
    specs = [("Categorical", {"K": 4}), ("Gaussian", {"sigma": 0.5})]
    prm, prob, X, Y = synth(12, specs, [500, 777], 144, 2, 2, (0.9, 1.2))
    want = so.elbo_grad_fused(prm, prob, X, Y)
    out = run(make_engine(prob, X, Y), prm)
    for k in KEYS:
        assert rel(out[k], want[k]) < TOL, k


def test_forced_jitter_rung_matches_oracle():
    """Ill-conditioned K_uu (lengthscale = 4 spacings): CPU and GPU compared at the SAME rung."""
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {})]
    prm, prob, X, Y = synth(13, specs, [300, 200], 24, 2, 1, (4.0, 5.0))
    prm["Z"] = np.tile(np.linspace(0, 1, 24)[:, None], (1, 2))
    want = so.elbo_grad_fused(prm, prob, X, Y)
    assert min(want["rungs"]) >= 0            # LAPACK takes the ladder here
    e = make_engine(prob, X, Y)
    free = run(e, prm)
    assert free["rungs"] == want["rungs"]     # the GPU ladder lands on the same rung
    out = run(e, prm, forced_rung=want["rungs"])
    # cond(K_uu + jitter) ~ 1e7 and |C| ~ 1e12: agreement is conditioning-limited.  The yardstick is the distance
    # between the oracle's own two restatements (explicit-inverse vs solve-based forms of the same reference
    # mathematics, both float64 LAPACK): the engine must sit within 10x of it (and within 1e-5 where that is smaller).
    lit = so.elbo_grad_literal(prm, prob, X, Y, forced_rungs=want["rungs"])
    for k in KEYS:
        assert rel(out[k], want[k]) < max(1e-5, 10.0 * rel(want[k], lit[k])), k


def test_row_shards_are_additive_and_chunk_invariant():
    """The multi-GPU contract: stats(rows A) + stats(rows B) -> finish == one pass over all rows; and the result does
    not depend on the row-chunk size."""
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    Ns = [3000, 2500, 2000, 1500]
    prm, prob, X, Y = synth(14, specs, Ns, 128, 3, 1, (0.8, 1.0, 1.3))
    bs = [2.0, 1.0, 3.0, 1.5]
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"], batch_scale=bs)
    e = make_engine(prob, X, Y)
    full = e.elbo_grad(**args)
    e2 = make_engine(prob, X, Y, chunk_rows=700)
    chunked = e2.elbo_grad(**args)
    for k in KEYS:
        assert rel(chunked[k], full[k]) < 1e-9, k     # summation order only
    cut = [n // 3 for n in Ns]
    e.step_begin(row_begin=[0] * 4, row_end=cut, **args)
    s1 = e.stats_read()
    e.step_begin(row_begin=cut, row_end=Ns, **args)
    s2 = e.stats_read()
    e.stats_write(s1 + s2)
    both = e.step_finish()
    for k in KEYS:
        assert rel(both[k], full[k]) < 1e-9, k


def test_minibatch_rows_match_oracle_on_slices():
    """SVI: contiguous row slices + batch_scale = N_all / N_batch (svmogp.py:89-90, util.py:52-72)."""
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 1.0}), ("Bernoulli", {})]
    Ns = [600, 500]
    prm, prob, X, Y = synth(15, specs, Ns, 32, 2, 1, (1.0, 1.3))
    e = make_engine(prob, X, Y)
    b0, b1 = [128, 100], [256, 200]
    bs = [Ns[t] / float(b1[t] - b0[t]) for t in range(2)]
    out = run(e, prm, bs, row_begin=b0, row_end=b1)
    want = so.elbo_grad_fused(prm, prob, [X[t][b0[t]:b1[t]] for t in range(2)], [Y[t][b0[t]:b1[t]] for t in range(2)], bs)
    for k in KEYS:
        assert rel(out[k], want[k]) < TOL, k


def test_empty_task_and_v_negative_flag():
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {})]
    prm, prob, X, Y = synth(16, specs, [200, 150], 16, 2, 1, (1.0, 1.2))
    e = make_engine(prob, X, Y)
    out = run(e, prm, row_begin=[0, 0], row_end=[200, 0])           # task 1 contributes no rows
    want = so.elbo_grad_fused(prm, prob, [X[0], X[1][:0]], [Y[0], Y[1][:0]])
    for k in KEYS:
        assert rel(out[k], want[k]) < TOL, k
    assert out["v_negative"] is False
    bad = dict(prm)
    bad["L_flat"] = prm["L_flat"] * 1e-3                             # S << Kuu  ->  v_fd = B s2 + w^2 c can go negative
    bad["kappa"] = -0.9 * prm["W"] ** 2
    out = run(e, bad)
    assert out["v_negative"] is True                                  # the reference prints 'v negative!' (svmogp_inf.py:221)


def test_kuu_cache_is_invisible():
    """HMOGP_CFG_CACHE_KUU (opt-in, used by the SVMOGP facade): K_uu / L_uu / K_uu^-1 are reused while Z and the kernel
    hyper-parameters are bit-identical; results equal the uncached engine bit for bit through a sequence that moves
    q(u) only (cache hit), then a lengthscale (miss), then Z (miss), then back (miss, then hit)."""
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {})]
    prm, prob, X, Y = synth(23, specs, [300, 200, 250], 40, 2, 1, (1.0, 1.3))
    plain, cached = make_engine(prob, X, Y), make_engine(prob, X, Y, cache_kuu=True)
    rng = np.random.RandomState(0)
    seq = [dict(prm)]
    a = dict(prm); a["m_u"] = prm["m_u"] + 0.1 * rng.randn(*prm["m_u"].shape); seq.append(a)
    b = dict(a); b["L_flat"] = a["L_flat"] * 1.1; seq.append(b)
    c = dict(b); c["lengthscale"] = np.asarray(b["lengthscale"]) * 1.05; seq.append(c)
    d = dict(c); d["Z"] = c["Z"] + 1e-3; seq.append(d)
    seq += [b, b, prm]
    for i, p in enumerate(seq):
        o1, o2 = run(plain, p), run(cached, p)
        assert o1["rungs"] == o2["rungs"]
        for k in KEYS:
            assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), (i, k)
    # a forced jitter rung is part of the key
    o1, o2 = run(plain, prm, forced_rung=[1, -1]), run(cached, prm, forced_rung=[1, -1])
    assert o1["rungs"] == o2["rungs"] == [1, -1]
    for k in KEYS:
        assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), k


def test_q_u_only_evaluation_uses_triangular_fold_and_matches_full():
    """E-steps (group_mask = QU) take the forward contraction with T = tril(C) + tril(C^T,-1) (half the products); the
    ELBO and the q(u) gradients must equal those of the full evaluation (ragged multi-tile M, two latents), and so must
    predict_f, which uses the same fold."""
    from oracle import svmogp_oracle as so
    from hetmogp_amd import _lib
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Gamma", {})]
    prm, prob, X, Y = synth(31, specs, [700, 500, 600], 300, 2, 1, (1.0, 1.3))
    e = make_engine(prob, X, Y)
    full = run(e, prm)
    qu = run(e, prm, group_mask=_lib.GROUP_QU)
    for k in ("elbo", "g_m_u", "g_L_u"):
        assert rel(qu[k], full[k]) < 1e-12, k
    for k in ("g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"):
        assert not np.any(qu[k])
    want = so.elbo_grad_fused(prm, prob, X, Y)
    for k in ("elbo", "g_m_u", "g_L_u"):
        assert rel(qu[k], want[k]) < TOL, k


@pytest.mark.parametrize("case", [
    dict(specs=[("Poisson", {})], Ns=[37], M=1, Q=1, P=1, cs=(1.0,)),                       # a single inducing point
    dict(specs=[("Gaussian", {"sigma": 0.3})], Ns=[1], M=5, Q=2, P=1, cs=(1.0, 2.0)),       # a single data row
    dict(specs=[("Bernoulli", {}), ("Exponential", {})], Ns=[129, 127], M=33, Q=8, P=1, cs=(1.0,) * 8),   # Q = HMOGP_MAXQ
    dict(specs=[("HetGaussian", {}), ("Beta", {})], Ns=[65, 200], M=27, Q=2, P=3, cs=(1.0, 1.5)),        # 3-D inputs
    dict(specs=[("Categorical", {"K": 3}), ("Gamma", {})], Ns=[90, 0], M=16, Q=1, P=4, cs=(1.2,)),      # 4-D, empty task
    dict(specs=[("Gaussian", {"sigma": 1.0})] * 6, Ns=[50, 60, 70, 80, 90, 100], M=64, Q=3, P=2, cs=(1.0, 1.2, 0.9)),
], ids=["M1", "N1", "Q8", "P3", "P4_empty", "T6_2d"])
def test_odd_shapes_vs_oracle(case):
    """Corner shapes against the NumPy oracle: M = 1, N = 1, Q = 8 latents, 3-D / 4-D inputs, an empty task, six tasks;
    every one also through row pools smaller than a task (chunk_rows = 48), which must not change anything, and a third time with
    small_path=False: at M <= 64 the first two legs take the fused small-model kernels, the third the regular row-pass kernels."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = synth(41, case["specs"], case["Ns"], case["M"], case["Q"], case["P"], case["cs"])
    want = so.elbo_grad_fused(prm, prob, X, Y)
    for kw in ({}, {"chunk_rows": 48}, {"small_path": False}):
        out = run(make_engine(prob, X, Y, **kw), prm)
        for k in KEYS:
            assert rel(out[k], want[k]) < TOL, (k, kw)


def test_repeated_evaluations_are_bit_identical():
    """No floating-point atomics anywhere (two-level deterministic reductions, fixed stream joins): the same parameters
    give the same bits every time, on the same engine and on a fresh one."""
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    prm, prob, X, Y = synth(43, specs, [900, 700, 800, 600], 260, 3, 1, (1.0, 1.2, 0.9))
    e = make_engine(prob, X, Y)
    first = run(e, prm)
    for i in range(4):
        again = run(e if i < 3 else make_engine(prob, X, Y), prm)
        for k in KEYS:
            assert np.array_equal(np.asarray(first[k]), np.asarray(again[k])), (i, k)


def test_pinned_parameters_and_reused_outputs():
    """hmogp_host_alloc: parameters in page-locked arrays and gradients returned in engine-owned page-locked arrays
    (reuse_outputs=True) give the same bits as the default pageable path; the reused arrays are overwritten by the
    next evaluation."""
    from hetmogp_amd.engine import pinned_empty
    specs = [("Gaussian", {"sigma": 0.5}), ("Poisson", {})]
    prm, prob, X, Y = synth(29, specs, [300, 250], 48, 2, 1, (1.0, 1.2))
    plain, fast = make_engine(prob, X, Y), make_engine(prob, X, Y, reuse_outputs=True)
    pp = dict(prm)
    for k in ("Z", "m_u", "L_flat"):
        a = pinned_empty(np.shape(prm[k]))
        a[...] = prm[k]
        pp[k] = a
    o1, o2 = run(plain, prm), run(fast, pp)
    for k in KEYS:
        assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), k
    gL = o2["g_L_u"]
    keep = gL.copy()
    pp["m_u"][...] = prm["m_u"] * 1.5
    o3 = run(fast, pp)
    assert o3["g_L_u"] is gL or np.shares_memory(o3["g_L_u"], gL)
    assert not np.array_equal(keep, gL)                       # overwritten in place by the second evaluation
    big = pinned_empty((1000, 7))
    big[...] = 3.0
    assert big.sum() == 21000.0 and big.flags["C_CONTIGUOUS"]


@pytest.mark.slow
def test_headline_size_properties():
    """BASELINE.json headline shape (N=200k/task would take the oracle hours): N_t = 50k, M = 1024, Q = 3 through
    size-independent properties -- chunk invariance and shard additivity of the ELBO and every gradient."""
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    Ns = [50000] * 4
    prm, prob, X, Y = synth(17, specs, Ns, 1024, 3, 1, (0.8, 1.0, 1.3))
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"])
    e = make_engine(prob, X, Y)
    full = e.elbo_grad(**args)
    assert np.isfinite(full["elbo"]) and full["rungs"] == [-1, -1, -1]
    e.step_begin(row_begin=[0] * 4, row_end=[20000] * 4, **args)
    s1 = e.stats_read()
    e.step_begin(row_begin=[20000] * 4, row_end=Ns, **args)
    s2 = e.stats_read()
    e.stats_write(s1 + s2)
    both = e.step_finish()
    for k in KEYS:
        assert rel(both[k], full[k]) < 1e-9, k


def test_natural_gradient_step():
    """f3 (no reference oracle: property tests).  With Gaussian likelihoods and ONE latent GP the model is conjugate: one
    natural-gradient step of size 1 lands on the optimum of q(u) (gradients vanish) -- with Q > 1 the factors q(u_q) are
    coupled through the mixing and a simultaneous step is only a Jacobi sweep.  The device update equals the same formulas
    in NumPy from the exported dL/dm, dL/dS; small steps increase the ELBO for non-conjugate likelihoods."""
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 0.5}), ("Gaussian", {"sigma": 1.0})]
    prm, prob, X, Y = synth(21, specs, [400, 300], 24, 1, 1, (1.0,))
    e = make_engine(prob, X, Y)
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"])
    out0 = e.elbo_grad(want_dL_dS=True, **args)
    m1, L1 = e.natgrad_step(1.0)
    # NumPy restatement of the update from the exported gradients
    M, Q = 24, 1
    for q in range(Q):
        L = so.flat_to_tril(prm["L_flat"][:, q], M)
        Si = np.linalg.inv(L @ L.T)
        dS = 0.5 * (out0["dL_dS"][q] + out0["dL_dS"][q].T)
        Lam = Si - 2.0 * dS
        th1 = Si @ prm["m_u"][:, q] + (out0["g_m_u"][:, q] - 2.0 * dS @ prm["m_u"][:, q])
        Snew = np.linalg.inv(Lam)
        assert rel(m1[:, q], Snew @ th1) < 1e-8
        Ln = so.flat_to_tril(L1[:, q], M)
        assert rel(Ln @ Ln.T, Snew) < 1e-8
    a1 = dict(args, m_u=m1, L_flat=L1)
    out1 = e.elbo_grad(**a1)
    assert out1["elbo"] > out0["elbo"]
    scale = max(np.max(np.abs(out0["g_m_u"])), np.max(np.abs(out0["g_L_u"])))
    assert np.max(np.abs(out1["g_m_u"])) < 1e-7 * scale and np.max(np.abs(out1["g_L_u"])) < 1e-7 * scale
    # non-conjugate likelihood, small step: monotone
    specs2 = [("Bernoulli", {}), ("Poisson", {})]
    prm2, prob2, X2, Y2 = synth(22, specs2, [400, 300], 24, 2, 1, (1.0, 1.3))
    e2 = make_engine(prob2, X2, Y2)
    a2 = dict(Z=prm2["Z"], m_u=prm2["m_u"], L_flat=prm2["L_flat"], variance=prm2["variance"],
              lengthscale=prm2["lengthscale"], W=prm2["W"], kappa=prm2["kappa"])
    prev = e2.elbo_grad(**a2)["elbo"]
    for _ in range(3):
        m_new, L_new = e2.natgrad_step(0.1)
        a2 = dict(a2, m_u=m_new, L_flat=L_new)
        cur = e2.elbo_grad(**a2)["elbo"]
        assert cur > prev
        prev = cur


def test_exact_zero_windows_equal_dense():
    """Opt-in exact-zero windows (HMOGP_CFG_EXACT_ZERO_WINDOWS): sorted 1-D inputs make K_uf banded and most tiles are
    skipped; every skipped term is a product with an exact 0.0, so the result must equal the dense path (to summation
    order of the row-range split) and the oracle.  Shuffled rows are not banded: the device falls back to dense ranges."""
    from oracle import svmogp_oracle as so
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    Ns = [3000, 2500, 1111, 700]
    prm, prob, X, Y = synth(31, specs, Ns, 300, 3, 1, (0.8, 1.0, 1.3))
    bs = [1.0, 2.0, 1.5, 3.0]
    dense = run(make_engine(prob, X, Y), prm, bs)
    win = run(make_engine(prob, X, Y, exact_zero_windows=True), prm, bs)
    want = so.elbo_grad_fused(prm, prob, X, Y, bs)
    for k in KEYS:
        assert rel(win[k], dense[k]) < 1e-10, k
        assert rel(win[k], want[k]) < TOL, k
    # chunked + windows
    winc = run(make_engine(prob, X, Y, exact_zero_windows=True, chunk_rows=512), prm, bs)
    for k in KEYS:
        assert rel(winc[k], dense[k]) < 1e-9, k
    # not banded (rows shuffled): dense fallback
    rng = np.random.RandomState(0)
    perm = [rng.permutation(n) for n in Ns]
    Xs, Ys = [x[p] for x, p in zip(X, perm)], [y[p] for y, p in zip(Y, perm)]
    ws = run(make_engine(prob, Xs, Ys, exact_zero_windows=True), prm, bs)
    for k in KEYS:
        assert rel(ws[k], dense[k]) < 1e-9, k
    # E-step mask (P~ never stored) and long lengthscale (no exact zeros at all)
    from hetmogp_amd import _lib
    d2 = run(make_engine(prob, X, Y), prm, bs, group_mask=_lib.GROUP_QU)
    w2 = run(make_engine(prob, X, Y, exact_zero_windows=True), prm, bs, group_mask=_lib.GROUP_QU)
    for k in ("elbo", "g_m_u", "g_L_u"):
        assert rel(w2[k], d2[k]) < 1e-11, k


@pytest.mark.slow
def test_exact_zero_windows_headline_shape():
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    Ns = [50000] * 4
    prm, prob, X, Y = synth(32, specs, Ns, 1024, 3, 1, (0.8, 1.0, 1.3))
    dense = run(make_engine(prob, X, Y), prm)
    e = make_engine(prob, X, Y, exact_zero_windows=True)
    win = run(e, prm)
    for k in KEYS:
        assert rel(win[k], dense[k]) < 1e-10, k


@pytest.mark.slow
def test_config5_like_2d_M2048_vs_oracle():
    """BASELINE config 5 shape: P = 2, M = 2048 (16 x 16 GEMM tiles), Q = 2, [Categorical(4), Gaussian], plus prediction
    on a grid (predict_f = predictive_new) and the per-likelihood predictive moments."""
    from oracle import svmogp_oracle as so
    from oracle import likelihoods_oracle as lo
    from hetmogp_amd import engine as E
    specs = [("Categorical", {"K": 4}), ("Gaussian", {"sigma": 0.5})]
    prm, prob, X, Y = synth(41, specs, [1500, 2000], 2048, 2, 2, (0.9, 1.1))
    want = so.elbo_grad_fused(prm, prob, X, Y)
    assert want["rungs"] == [-1, -1]
    e = make_engine(prob, X, Y)
    out = run(e, prm)
    lit = so.elbo_grad_literal(prm, prob, X, Y)       # yardstick: the oracle's literal (solve-based) restatement
    for k in KEYS:
        assert rel(out[k], want[k]) < min(1e-7, max(1e-8, 10.0 * rel(want[k], lit[k]))), (k, rel(want[k], lit[k]))
    g = np.stack(np.meshgrid(np.linspace(0, 1, 24), np.linspace(0, 1, 24), indexing="ij"), -1).reshape(-1, 2)
    m, v = e.predict_f(g)
    u = so.u_algebra(prm, prob)
    for d in range(prob["Df"]):
        md, vd = np.zeros(len(g)), np.zeros(len(g))
        for q in range(2):
            K = so.rbf_K(g, prm["Z"][:, 2 * q:2 * q + 2], prm["variance"][q], prm["lengthscale"][q])
            w = prm["W"][q, d]
            md += w * (K @ u["a"][q])
            vd += (w * w + prm["kappa"][q, d]) * prm["variance"][q] + w * w * np.sum((K @ u["C"][q]) * K, 1)
        assert rel(m[:, d], md) < 1e-7 and rel(v[:, d], vd) < 1e-7
    mp, vp = E.predictive("Categorical", m[:, :3], np.abs(v[:, :3]), K=4)
    wm, wv = lo.predictive("Categorical", m[:, :3], np.abs(v[:, :3]), K=4)
    assert rel(mp, wm) < 1e-9 and np.allclose(mp.sum(1), 1.0)


@pytest.mark.slow
def test_config4_like_eight_likelihoods_Q4_vs_oracle():
    """BASELINE config 4 mix: T = 8 [HetGaussian, Categorical(5), Beta, Exponential, Gaussian, Bernoulli, Poisson, Gamma],
    Df = 14, Q = 4, two row shards combined through the statistic bundle."""
    from oracle import svmogp_oracle as so
    specs = [("HetGaussian", {}), ("Categorical", {"K": 5}), ("Beta", {}), ("Exponential", {}), ("Gaussian", {"sigma": 0.5}),
             ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
    Ns = [400, 150, 300, 250, 500, 350, 300, 200]
    prm, prob, X, Y = synth(42, specs, Ns, 160, 4, 1, (0.8, 1.0, 1.3, 1.1))
    assert prob["Df"] == 14
    want = so.elbo_grad_fused(prm, prob, X, Y)
    e = make_engine(prob, X, Y)
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"])
    cut = [n // 2 for n in Ns]
    e.step_begin(row_begin=[0] * 8, row_end=cut, **args)
    s1 = e.stats_read()
    e.step_begin(row_begin=cut, row_end=Ns, **args)
    e.stats_write(s1 + e.stats_read())
    out = e.step_finish()
    for k in KEYS:
        assert rel(out[k], want[k]) < TOL, k


def test_error_conventions():
    """Status codes surface as the reference's exception types: bad arguments -> ValueError, call-order
    violations -> HetMOGPError(E_STATE), a non-PD K_uu after five jitter rungs -> LinAlgError (GPy jitchol, util.py:198)."""
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine
    with pytest.raises(ValueError):
        Engine([("Gaussian", {})], Q=9, M=8, P=1)                      # more latent GPs than HMOGP_MAXQ
    with pytest.raises(ValueError):
        Engine([("Categorical", {"K": 11})], Q=1, M=8, P=1)            # dim_f above HMOGP_MAXJ
    with pytest.raises(ValueError):
        Engine([("Gaussian", {})], Q=1, M=8, P=7)                      # input dimension above 4
    specs = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {})]
    prm, prob, X, Y = synth(51, specs, [50, 40], 8, 2, 1, (1.0, 1.2))
    e = make_engine(prob, X, Y)
    with pytest.raises(_lib.HetMOGPError) as ei:
        e.step_finish()                                                # finish without begin
    assert ei.value.code == _lib.E_STATE
    with pytest.raises(ValueError):
        run(e, prm, row_begin=[0, 0], row_end=[51, 40])                # row range outside the task's data
    bad = dict(prm)
    bad["lengthscale"] = np.array([0.0, 1.0])
    with pytest.raises(ValueError):
        run(e, bad)
    bad = dict(prm)
    bad["variance"] = np.array([-1.0, 0.5])                            # K_uu = -I-like: not PD, non-positive diagonal
    with pytest.raises(np.linalg.LinAlgError):
        run(e, bad)
    ok = run(e, prm)                                                   # the handle stays usable after errors
    assert np.isfinite(ok["elbo"])
