"""GPU: the BASELINE.json configurations at their FULL sizes (H: 4 x 200 000 rows, M = 1024; C2: the same at M = 512; the
per-rank share of C4: 8 x 125 000 rows, Q = 4, Df = 14 -- 4.1e9-element K^ / P~ workspaces), where the oracle cannot run
the whole evaluation, through size-independent properties:

  * shard additivity   the statistic bundles of two row shards add up to the bundle of all rows (what the multi-GPU
                       exchange relies on) -- gradients after `finish` agree with the single evaluation;
  * chunk invariance   streaming the rows in several pools gives the same results as one pool;
  * repeatability      two evaluations are bit-identical (deterministic reductions, no floating-point atomics);
  * oracle parity      on a window of rows taken from the END of every task (row_begin close to N_t: the offsets into the
                       row workspaces are exercised at their largest values) against the NumPy oracle on exactly those rows;
  * dense == exact-zero windows (1-D sorted inputs): the opt-in mode drops only products with exact zeros.
"""
import numpy as np
import pytest

from conftest import elementwise_excess, rel_norm as rel

pytestmark = pytest.mark.gpu

KEYS = ["elbo", "g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"]
H_SPECS = [("Gaussian", {"sigma": 0.5}), ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]
C4_SPECS = [("HetGaussian", {}), ("Categorical", {"K": 5}), ("Beta", {}), ("Exponential", {}), ("Gaussian", {"sigma": 0.5}),
            ("Bernoulli", {}), ("Poisson", {}), ("Gamma", {})]


def check_config(specs, N, M, Q, window, seed, pools, exact_zero=True, oracle_tol=1e-8, P=1, calibrate=False):
    from hetmogp_amd.engine import Engine
    from hetmogp_amd.synthetic import make_case
    from oracle import svmogp_oracle as so
    T = len(specs)
    prm, X, Y = make_case(specs, [N] * T, M=M, Q=Q, P=P, seed=seed)
    e = Engine(specs, Q, M, P)
    e.set_data(X, Y)
    full = e.elbo_grad(**prm)
    assert np.isfinite(full["elbo"]) and not full["v_negative"] and full["rungs"] == [-1] * Q
    # repeatability: same bits
    again = e.elbo_grad(**prm)
    for k in KEYS:
        assert np.array_equal(np.asarray(full[k]), np.asarray(again[k])), k
    # shard additivity (uneven split, different per task)
    cut = [N // 3 + 1000 * t for t in range(T)]
    e.step_begin(row_begin=[0] * T, row_end=cut, **prm)
    s1 = e.stats_read()
    e.step_begin(row_begin=cut, row_end=[N] * T, **prm)
    s2 = e.stats_read()
    e.stats_write(s1 + s2)
    both = e.step_finish()
    for k in KEYS:
        assert rel(both[k], full[k]) < 1e-9, ("shards", k, rel(both[k], full[k]))
    # oracle parity on the LAST `window` rows of every task
    prob = so.make_problem(specs, Q, M, P)
    Xw, Yw = [x[N - window:] for x in X], [y[N - window:] for y in Y]
    want = so.elbo_grad_fused(prm, prob, Xw, Yw)
    lit = so.elbo_grad_literal(prm, prob, Xw, Yw) if calibrate else None
    got = e.elbo_grad(row_begin=[N - window] * T, row_end=[N] * T, **prm)
    for k in KEYS:
        tol = oracle_tol
        if calibrate:      # conditioning-limited shapes (2-D, M = 2048): the yardstick is the distance between the oracle's own
            tol = min(1e-7, max(oracle_tol, 10.0 * rel(want[k], lit[k])))      # literal (solve-based) and fused restatements
        assert rel(got[k], want[k]) < tol, ("oracle window", k, rel(got[k], want[k]))
        assert elementwise_excess(got[k], want[k]) <= 1.0, ("oracle window, element-wise 1e-5", k)
    e.close()
    # chunk invariance: `pools` pools instead of one
    total = N * T
    e2 = Engine(specs, Q, M, P, chunk_rows=(total + pools - 1) // pools + 17)
    e2.set_data(X, Y)
    chunked = e2.elbo_grad(**prm)
    for k in KEYS:
        assert rel(chunked[k], full[k]) < 1e-9, ("pools", k, rel(chunked[k], full[k]))
    e2.close()
    if exact_zero:
        e3 = Engine(specs, Q, M, P, exact_zero_windows=True)
        e3.set_data(X, Y)
        ez = e3.elbo_grad(**prm)
        for k in KEYS:
            assert rel(ez[k], full[k]) < 1e-9, ("exact-zero windows", k, rel(ez[k], full[k]))
        e3.close()


@pytest.mark.timeout(600)
def test_headline_H_full_size():
    """H: T=4 [Gaussian, Bernoulli, Poisson, Gamma], N_t = 200 000, M = 1024, Q = 3 (the bench workload)."""
    check_config(H_SPECS, 200000, 1024, 3, window=2000, seed=20260929, pools=3)


@pytest.mark.timeout(600)
def test_C2_full_size():
    """C2: the same mix at M = 512 (the Gram's lower tiles are 4 diagonal + 6 off-diagonal: the diagonal path weighs most)."""
    check_config(H_SPECS, 200000, 512, 3, window=2000, seed=20260931, pools=2)


@pytest.mark.timeout(900)
def test_C4_rank_share_full_size():
    """One rank's share of C4: 8 tasks x 125 000 rows, Q = 4, Df = 14 (HetGaussian, Categorical(5), Beta, ...): the K^ / P~
    workspaces hold 4 x 1e6 x 1024 = 4.1e9 elements each -- element indices beyond 2^32."""
    check_config(C4_SPECS, 125000, 1024, 4, window=1000, seed=20260933, pools=2, exact_zero=False)


@pytest.mark.timeout(1200)
def test_C4_full_size_pools():
    """BASELINE config 4 at its FULL size on ONE GPU: 8 tasks x 1 000 000 rows, M = 1024, Q = 4, Df = 14, streamed through pools
    of 2^20 rows that cross task boundaries.  The evaluation equals the sum of the eight rank-share bundles (what the 8-GPU
    exchange would all-reduce: `dist.shard_ranges` row ranges, stats_read / stats_write), is bit-repeatable, and matches the
    oracle on a window of rows at the END of every task."""
    from hetmogp_amd.engine import Engine
    from hetmogp_amd.synthetic import make_case
    from hetmogp_amd.dist import shard_ranges
    from oracle import svmogp_oracle as so
    N, M, Q, P, T, world = 1000000, 1024, 4, 1, len(C4_SPECS), 8
    prm, X, Y = make_case(C4_SPECS, [N] * T, M=M, Q=Q, P=P, seed=20260933)
    e = Engine(C4_SPECS, Q, M, P)
    e.set_data(X, Y)
    full = e.elbo_grad(**prm)
    assert np.isfinite(full["elbo"]) and not full["v_negative"] and full["rungs"] == [-1] * Q
    again = e.elbo_grad(**prm)
    for k in KEYS:
        assert np.array_equal(np.asarray(full[k]), np.asarray(again[k])), k
    total = None
    for rank in range(world):
        rb, re = shard_ranges([0] * T, [N] * T, rank, world)
        e.step_begin(row_begin=rb, row_end=re, **prm)
        s = e.stats_read()
        total = s if total is None else total + s
    e.stats_write(total)
    summed = e.step_finish()
    for k in KEYS:
        # (1e-7, not the 1e-9 of the smaller configurations: g_variance / g_lengthscale are differences of sums over 8e6 rows that
        #  are 10-100x their result, and eight shards add those sums in another order than eight pools -- measured 1.1e-8)
        assert rel(summed[k], full[k]) < 1e-7, ("sum of 8 rank shares", k, rel(summed[k], full[k]))
        assert elementwise_excess(summed[k], full[k]) <= 1.0, ("sum of 8 rank shares, element-wise 1e-5", k)
    window = 4000      # (4 inducing spacings of inputs: a window inside ONE spacing makes H_q nearly rank one and the comparison
    prob = so.make_problem(C4_SPECS, Q, M, P)      #  conditioning-limited -- 4e-8 in g_Z with 500 rows)
    want = so.elbo_grad_fused(prm, prob, [x[N - window:] for x in X], [y[N - window:] for y in Y])
    lit = so.elbo_grad_literal(prm, prob, [x[N - window:] for x in X], [y[N - window:] for y in Y])
    got = e.elbo_grad(row_begin=[N - window] * T, row_end=[N] * T, **prm)
    for k in KEYS:
        # (rows from the END of the input range: the last inducing points see data on one side only and their g_Z entries are
        #  differences of terms ~1e3 x larger; as in check_config(calibrate=True) the yardstick is the distance between the
        #  oracle's own literal (solve-based) and fused restatements, capped at 1e-7)
        tol = min(1e-7, max(1e-8, 10.0 * rel(want[k], lit[k])))
        if k == "g_Z":     # quirk Q10 (GPy gradients_X drops entries whose computed distance is exactly 0): with 1e6 rows per task one
            tol = 1e-7     # row lies within 1.5e-8 of the inducing point at 1.0; the oracle drops its term like the reference, the
                           # engine's default mode keeps it (strict mode drops it): 4.3e-8 of that inducing point's entry
        print("C4 full, oracle window:", k, "engine-fused %.2e" % rel(got[k], want[k]), "fused-literal %.2e" % rel(want[k], lit[k]))
        assert rel(got[k], want[k]) < tol, ("oracle window", k, rel(got[k], want[k]), tol)
        assert elementwise_excess(got[k], want[k]) <= 1.0, ("oracle window, element-wise 1e-5", k)
    e.close()


@pytest.mark.timeout(900)
def test_C5_full_size():
    """C5: T=2 [Categorical(4), Gaussian], 2-D inputs, N_t = 50 000, M = 2048 (46 x 46 grid cut to 2048), Q = 2 -- 16 x 16 GEMM
    tiles, 64 factorisation panels, the P = 2 variants of rbf / colstats.  Oracle parity on the last 1500 rows of both tasks."""
    check_config([("Categorical", {"K": 4}), ("Gaussian", {"sigma": 0.5})], 50000, 2048, 2, window=1500, seed=20260934,
                 pools=2, exact_zero=False, P=2, calibrate=True)


@pytest.mark.timeout(900)
def test_C3_full_size_minibatches_of_resident_million():
    """C3: N_all = 1 000 000 rows per task RESIDENT (hmogp_set_task_data once), SVI minibatches = contiguous row ranges of it
    (util.py:52-72), batch_scale = N_all / N_batch (svmogp.py:89-90).  Minibatches near the END of the resident arrays (offsets
    ~990 000, different per task, and the short last slice) against the NumPy oracle on exactly those rows; the same rows
    uploaded alone to a second engine give the same numbers; E-step (q(u) group only) and M-step gating; repeatability."""
    from hetmogp_amd import _lib
    from hetmogp_amd.engine import Engine
    from hetmogp_amd.synthetic import make_case
    from oracle import svmogp_oracle as so
    T, N, M, Q, B = 4, 1000000, 1024, 3, 8192
    prm, X, Y = make_case(H_SPECS, [N] * T, M=M, Q=Q, P=1, seed=20260932)
    prob = so.make_problem(H_SPECS, Q, M, 1)
    e = Engine(H_SPECS, Q, M, 1)
    e.set_data(X, Y)
    for rb, re_ in (([990000 - 1000 * t for t in range(T)], [990000 - 1000 * t + B for t in range(T)]),
                    ([N - 5632] * T, [N] * T)):                      # 1e6 = 122 * 8192 + 576: also a short ragged slice
        bs = [N / float(b - a) for a, b in zip(rb, re_)]
        Xb, Yb = [x[a:b] for x, a, b in zip(X, rb, re_)], [y[a:b] for y, a, b in zip(Y, rb, re_)]
        want = so.elbo_grad_fused(prm, prob, Xb, Yb, bs)
        got = e.elbo_grad(row_begin=rb, row_end=re_, batch_scale=bs, **prm)
        assert got["rungs"] == [-1] * Q and not got["v_negative"]
        for k in KEYS:
            assert rel(got[k], want[k]) < 1e-8, ("minibatch vs oracle", k, rel(got[k], want[k]))
            assert elementwise_excess(got[k], want[k]) <= 1.0, ("minibatch vs oracle, element-wise 1e-5", k)
        again = e.elbo_grad(row_begin=rb, row_end=re_, batch_scale=bs, **prm)
        for k in KEYS:
            assert np.array_equal(np.asarray(got[k]), np.asarray(again[k])), k
        e2 = Engine(H_SPECS, Q, M, 1)
        e2.set_data(Xb, Yb)
        alone = e2.elbo_grad(batch_scale=bs, **prm)
        for k in KEYS:
            assert rel(alone[k], got[k]) < 1e-11, ("resident slice vs own upload", k)
        e2.close()
        est = e.elbo_grad(row_begin=rb, row_end=re_, batch_scale=bs, group_mask=_lib.GROUP_QU, **prm)
        mst = e.elbo_grad(row_begin=rb, row_end=re_, batch_scale=bs, group_mask=_lib.GROUP_HYPER | _lib.GROUP_Z, **prm)
        for k in ("elbo", "g_m_u", "g_L_u"):
            assert rel(est[k], got[k]) < 1e-9, ("E-step", k)      # (the E-step's forward runs against the triangular fold of C)
        for k in ("elbo", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"):
            assert rel(mst[k], got[k]) < 1e-9, ("M-step", k)
        assert not np.any(est["g_Z"]) and not np.any(mst["g_m_u"])
    e.close()
