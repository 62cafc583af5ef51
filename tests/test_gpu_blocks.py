"""GPU: parity of the building-block kernels, called through the C ABI (hetmogp_amd.engine -> libhetmogp_hip.so),
against the NumPy oracle / LAPACK and the golden vectors of the reference.  Tolerances: fp64, relative to the
largest magnitude of each array (1e-12 for GEMM / RBF, 1e-9 for factorisations and quadratures)."""
import glob
import json
import os

import numpy as np
import pytest
import scipy.linalg

from conftest import GOLDEN, rel_norm as rel
import likgrid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    from hetmogp_amd import engine
    return engine


@pytest.mark.parametrize("tA,tB", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(128, 128, 64), (130, 70, 37), (5, 5, 5), (300, 257, 129), (1, 1, 1), (64, 512, 1030),
                                   (257, 3, 16)])
def test_gemm_f64_all_layouts(E, tA, tB, shape):
    """Asymmetric operands so a transposed fragment map cannot pass (cdna guide rule 16)."""
    M, N, K = shape
    rng = np.random.RandomState(M * 7 + N * 3 + K + tA * 2 + tB)
    A = rng.randn(K, M) if tA else rng.randn(M, K)
    B = rng.randn(N, K) if tB else rng.randn(K, N)
    A += np.arange(A.shape[1])[None, :] * 0.01
    C0 = rng.randn(M, N)
    want = 0.7 * (A.T if tA else A) @ (B.T if tB else B) - 1.3 * C0
    got = E.gemm(A, B, transA=bool(tA), transB=bool(tB), alpha=0.7, beta=-1.3, C0=C0)
    assert rel(got, want) < 1e-13


@pytest.mark.parametrize("tA,tB", [(0, 0), (1, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize("shape", [(256, 256, 256), (320, 64, 48), (256, 192, 1024), (1024, 1024, 1024)])
def test_gemm_f64_small_tiles(E, tA, tB, shape):
    """beta = 0, extents that are multiples of 64 and fewer than 512 tiles of 128 x 128: launch_gemm_f64 takes the
    64 x 64-tile kernel (gemm_small.hip).  C starts as NaN: it must be overwritten, never read."""
    M, N, K = shape
    rng = np.random.RandomState(M + 3 * N + 7 * K + tA * 2 + tB)
    A = rng.randn(K, M) if tA else rng.randn(M, K)
    B = rng.randn(N, K) if tB else rng.randn(K, N)
    A += np.arange(A.shape[1])[None, :] * 0.01
    want = -0.3 * (A.T if tA else A) @ (B.T if tB else B)
    got = E.gemm(A, B, transA=bool(tA), transB=bool(tB), alpha=-0.3, beta=0.0, C0=np.full((M, N), np.nan))
    assert rel(got, want) < 1e-13


@pytest.mark.parametrize("P,N,M", [(1, 100, 37), (1, 257, 64), (2, 65, 50), (3, 33, 16), (1, 5, 1030)])
def test_rbf_cross_cov(E, P, N, M):
    from oracle import svmogp_oracle as so
    rng = np.random.RandomState(P * 100 + N + M)
    X, Z = rng.rand(N, P), rng.rand(M, P)
    ell = 0.9 * M ** (-1.0 / P)
    got = E.rbf_cross_cov(X, Z, 0.7, ell)
    want = so.rbf_K(X, Z, 0.7, ell)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "cov_*.npz"))), ids=os.path.basename)
def test_jitchol_ladder_and_inverse_golden(E, path):
    """Golden Kuu -> (Luu, Kuui, rung) from the reference's util.latent_funs_cov (util.py:181-200)."""
    g = np.load(path)
    L, Ai, rungs = E.jitchol_inv(g["Kuu"])
    assert rungs == [int(r) for r in g["rung"]]
    if max(rungs) < 0:     # well-conditioned: factor and inverse agree tightly
        assert rel(L, g["Luu"]) < 1e-10
        assert rel(Ai, g["Kuui"]) < 1e-8
    else:                  # singular + jitter: cond ~ 1e6, compare through the defining identities instead
        for q in range(L.shape[0]):
            jit = np.diag(g["Kuu"][q]).mean() * 1e-6 * 10.0 ** rungs[q]
            Aj = g["Kuu"][q] + jit * np.eye(L.shape[1])
            assert rel(L[q] @ L[q].T, Aj) < 1e-12
            assert rel(Ai[q] @ Aj, np.eye(L.shape[1])) < 1e-6


@pytest.mark.parametrize("M", [1, 31, 32, 33, 50, 64, 200, 256, 320, 513, 576, 1024])
def test_potrf_potri_vs_lapack(E, M):
    rng = np.random.RandomState(M)
    Q = 2
    B = rng.randn(Q, M, M)
    A = B @ B.transpose(0, 2, 1) + M * np.eye(M)[None]
    L, Ai, rungs = E.jitchol_inv(A)
    assert rungs == [-1] * Q
    for q in range(Q):
        Lr = scipy.linalg.cholesky(A[q], lower=True)
        assert rel(L[q], Lr) < 1e-12
        assert np.all(np.triu(L[q], 1) == 0.0)
        assert rel(Ai[q], np.linalg.inv(A[q])) < 1e-10
    Lv = np.tril(rng.randn(Q, M, M)) * 0.1 + np.eye(M)[None]
    Si = E.potri(Lv)
    for q in range(Q):
        assert rel(Si[q], np.linalg.inv(Lv[q] @ Lv[q].T)) < 1e-9


def test_jitchol_not_pd_raises(E):
    A = -np.eye(8)[None]
    with pytest.raises(np.linalg.LinAlgError):
        E.jitchol_inv(A)


@pytest.mark.parametrize("path", likgrid.reference_fixtures(), ids=os.path.basename)
def test_var_exp_golden(E, path):
    """Per-likelihood E_q[log p], d/dm, d/dv against the reference's own likelihoods/*.py outputs (incl. clip rows), element by
    element: |kernel - reference| <= (C + C_oracle) * 2^-52 * S with each element's condition scale S
    (tests/golden/lik_scales.npz) and the constants of DESIGN 9a (two float64 evaluations: the kernel's and the oracle's add).  The earlier array-maximum form is kept beside it: no element is held to less than before."""
    g = np.load(path)
    name, kw, y, m, v, want, S, kind, cls = likgrid.fixture_want_and_scale(path)
    ve, dm, dv = E.var_exp(name, y, m, v, **kw)
    likgrid.assert_rows(likgrid.pack(ve, dm, dv, want.shape[0]), want, S, np.zeros(want.shape, np.uint8), kind, cls,
                        likgrid.c_kernel_vs_float64(name), os.path.basename(path) + " kernel vs reference")
    for got, want in ((ve[:, None], g["var_exp"]), (dm, g["var_exp_dm"]), (dv, g["var_exp_dv"])):
        np.testing.assert_allclose(got, want, rtol=2e-9, atol=1e-11 * np.max(np.abs(want)))


def test_var_exp_large_random_vs_oracle(E):
    """3000 seeded rows per family (m in [-2, 2], v in [e^-5, e]) against the NumPy oracle, element by element under the bulk
    constants of DESIGN 9a with each element's condition scale; the earlier array-maximum form is kept beside it."""
    from oracle import likelihoods_oracle as lo
    scales = likgrid.load_scales()
    for name, kw, y, m, v in likgrid.large_random_cases():
        n, J = m.shape
        assert J == E.lik_dim_f(name, **kw)
        got = E.var_exp(name, y, m, v, **kw)
        want = lo.var_exp_all(name, y[:, None], m, v, **kw)
        C = likgrid.c_kernel_vs_float64(name)           # two float64 evaluations: the two constants add
        likgrid.assert_rows(likgrid.pack(*got, n), likgrid.pack(*want, n), scales["random__%s__S" % name].astype(float),
                            np.zeros((n, 1 + 2 * J), np.uint8), np.array([0] + [1] * J + [2] * J), np.zeros(n, int), C,
                            "3000 random rows, " + name)
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b.reshape(a.shape), rtol=1e-9, atol=1e-11 * np.max(np.abs(b)))


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "pred_*.npz"))), ids=os.path.basename)
def test_predictive_golden(E, path):
    """f2: predictive mean / variance of y against the reference's own `<likelihood>.predictive` outputs."""
    g = np.load(path)
    name, kw = json.loads(str(g["spec"]))
    mp, vp = E.predictive(name, g["m"], g["v"], gh_T=int(g["gh_T"]), **kw)
    np.testing.assert_allclose(mp, g["mean_pred"], rtol=1e-10, atol=1e-13 * np.max(np.abs(g["mean_pred"])))
    np.testing.assert_allclose(vp, g["var_pred"], rtol=1e-8, atol=1e-12 * max(1.0, np.max(np.abs(g["var_pred"]))))


def test_log_predictive_monte_carlo_vs_quadrature(E):
    """f4: the Monte-Carlo log predictive is stochastic (own counter-based generator), so it is checked statistically:
    for 1-D likelihoods log E_q[p(y|f)] is also a Gauss-Hermite integral (T = 20, the oracle), and the MC estimate with
    S = 16384 samples must agree per row within 0.05 nats and within 0.01 on average; HetGaussian / Categorical are
    checked against NumPy Monte-Carlo with the same number of samples."""
    from oracle import likelihoods_oracle as lo
    rng = np.random.RandomState(9)
    n = 64
    x, w = lo.gh_rule(20)
    for name, y in (("Gaussian", rng.randn(n)), ("Bernoulli", (rng.rand(n) < 0.5).astype(float)),
                    ("Poisson", rng.poisson(3.0, n).astype(float)), ("Exponential", rng.gamma(2.0, 1.0, n))):
        m, v = rng.uniform(-1, 1, (n, 1)), np.exp(rng.uniform(-3, 0, (n, 1)))
        f = x[None, :] * np.sqrt(2 * v) + m
        if name == "Gaussian":
            lp = -0.5 * np.log(2 * np.pi) - 0.5 * (y[:, None] - f) ** 2          # sigma ignored (quirk Q6)
        elif name == "Bernoulli":
            p = np.clip(1 / (1 + np.exp(-f)), 1e-9, 1 - 1e-9)
            lp = y[:, None] * np.log(p) + (1 - y[:, None]) * np.log(1 - p)
        elif name == "Poisson":
            from scipy.special import gammaln
            lp = -np.exp(f) + y[:, None] * f - gammaln(y[:, None] + 1)
        else:
            b = np.clip(np.exp(-f), 1e-9, 1e9)
            lp = -np.log(b) - y[:, None] / b
        want = np.log(np.exp(lp) @ w)
        got = E.log_predictive_rows(name, y, m, v, num_samples=16384, seed=123)
        assert np.max(np.abs(got - want)) < 0.05 and abs(np.mean(got - want)) < 0.01, name
        assert np.array_equal(got, E.log_predictive_rows(name, y, m, v, num_samples=16384, seed=123))   # reproducible
    # multi-function likelihoods: NumPy Monte-Carlo
    S = 16384
    for name, kw, J in (("HetGaussian", {}, 2), ("Categorical", {"K": 4}, 3)):
        m, v = rng.uniform(-1, 1, (n, J)), np.exp(rng.uniform(-3, 0, (n, J)))
        y = rng.randn(n) if name == "HetGaussian" else rng.randint(1, 5, n).astype(float)
        F = m[:, :, None] + np.sqrt(v)[:, :, None] * rng.randn(n, J, S)
        if name == "HetGaussian":
            lp = -0.5 * np.log(2 * np.pi) - 0.5 * F[:, 1] - 0.5 * (y[:, None] - F[:, 0]) ** 2 / np.exp(F[:, 1])
        else:
            e = np.exp(F)
            den = 1 + e.sum(1, keepdims=True)
            p = np.clip(np.concatenate([e / den, 1 / den], 1), 1e-9, 1 - 1e-9)
            p = p / p.sum(1, keepdims=True)
            lp = np.log(p[np.arange(n), (y - 1).astype(int)])
        want = np.log(np.mean(np.exp(lp), 1))
        got = E.log_predictive_rows(name, y, m, v, num_samples=S, seed=7, **kw)
        assert np.max(np.abs(got - want)) < 0.1 and abs(np.mean(got - want)) < 0.02, name
