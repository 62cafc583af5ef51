"""GPU: every (family, function count) a launcher can choose reaches the kernel instantiation of that count (csrc/lik_dispatch.h,
visit_family): Categorical K = 2 .. 9 (1 .. 8 functions) and Dirichlet K = 2 .. 4, in closed form -- no grid, no oracle (the oracle's
10^(K-1)-node tensor does not fit in memory from K = 7 on).

Inputs: N = 5 rows -- not a multiple of the 4 rows per block of the wave-per-row kernels, so the last block is partial -- with m seeded in
[-2, 2] and v = 0.  No block refuses or clips v = 0: every quadrature node and every Monte-Carlo draw is then f = m, the normalised
weights sum to 1, and each block returns the family's log density at f = m:
  * Categorical, labels 1 .. K cycling over the rows, class K the reference: `var_exp`'s ve, `log_predictive_density_rows` (10 nodes)
    and `log_predictive_rows(num_samples=8)` equal log softmax_y([m, 0]) (m in [-2, 2], K <= 9: every probability is above 2e-3, far
    from the reference's clip at 1e-9).  `predictive`'s mean, (N, K - 1), equals the softmax probabilities of the K - 1 classes that have a
    function, as the reference returns them: renormalised over those K - 1 columns (categorical.py:89-91).
  * Dirichlet, seeded compositions: the same three blocks equal lgamma(sum a) - sum lgamma(a_k) + sum (a_k - 1) log y_k, a = exp(m).
A wrong function count reads the wrong number of functions per row and misses by O(1).  Tolerance: the array-maximum form of
tests/test_gpu_blocks.py for kernel against NumPy, rtol = 1e-9, atol = 1e-11 max|want| (the rule at v = 0 returns the closed form to a
few 1e-16)."""
import numpy as np
import pytest
from scipy.special import gammaln

pytestmark = pytest.mark.gpu

N = 5


@pytest.fixture(scope="module")
def E():
    from hetmogp_amd import engine
    return engine


def close(got, want, what):
    got, want = np.asarray(got, float), np.asarray(want, float).reshape(np.shape(got))
    print("[dispatch] %-44s max|got - want| = %.3g (max|want| = %.3g)" % (what, np.max(np.abs(got - want)), np.max(np.abs(want))))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-11 * np.max(np.abs(want)), err_msg=what)


@pytest.mark.parametrize("K", range(2, 10))
def test_categorical_every_function_count(E, K):
    D = K - 1
    m = np.random.RandomState(100 + K).uniform(-2.0, 2.0, (N, D))
    v = np.zeros((N, D))
    y = (np.arange(N) % K + 1).astype(float)
    f = np.concatenate([m, np.zeros((N, 1))], axis=1)              # class K is the reference class: f_K = 0
    logp = f - np.log(np.sum(np.exp(f), axis=1, keepdims=True))
    want = logp[np.arange(N), y.astype(int) - 1]
    close(E.var_exp("Categorical", y, m, v, K=K)[0], want, "Categorical K=%d var_exp" % K)
    close(E.log_predictive_density_rows("Categorical", y, m, v, gh_T=10, K=K), want, "Categorical K=%d log_predictive_density" % K)
    close(E.log_predictive_rows("Categorical", y, m, v, num_samples=8, seed=K, K=K), want, "Categorical K=%d log_predictive (8 draws)" % K)
    p = np.exp(logp[:, :D])
    close(E.predictive("Categorical", m, v, K=K)[0], p / p.sum(axis=1, keepdims=True), "Categorical K=%d predictive mean" % K)


@pytest.mark.parametrize("K", range(2, 5))
def test_dirichlet_every_function_count(E, K):
    rng = np.random.RandomState(200 + K)
    m = rng.uniform(-2.0, 2.0, (N, K))
    v = np.zeros((N, K))
    y = rng.dirichlet(np.full(K, 2.0), N)
    a = np.exp(m)
    want = gammaln(a.sum(axis=1)) - gammaln(a).sum(axis=1) + ((a - 1.0) * np.log(y)).sum(axis=1)
    close(E.var_exp("Dirichlet", y, m, v, K=K)[0], want, "Dirichlet K=%d var_exp" % K)
    close(E.log_predictive_density_rows("Dirichlet", y, m, v, gh_T=10, K=K), want, "Dirichlet K=%d log_predictive_density" % K)
    close(E.log_predictive_rows("Dirichlet", y, m, v, num_samples=8, seed=K, K=K), want, "Dirichlet K=%d log_predictive (8 draws)" % K)
