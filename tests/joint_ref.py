"""float64 NumPy restatement of the joint posterior at new inputs (`hmogp_predict_f_joint` / `hmogp_sample_f_joint`; csrc/joint.hip and
`hmogp_engine::joint` of csrc/engine_optim.hip), the designed cases, the loader / criterion of their grid
tests/golden/jointgrid.npz (tools/make_joint_grid.py; 50-digit values from tests/joint_ref_mp.py).

From the raw parameters Z [M, Q P], variance [Q], lengthscale [Q], m_u [M, Q], L_flat [M (M + 1) / 2, Q], W [Q, Df], kappa [Q, Df]:
  K_q = k_q(Z_q, Z_q),  S_q = L_q L_q^T,  A_q = k_q(Xnew, Z_q),  C_q = K_q^-1 S_q K_q^-1 - K_q^-1,  G_q = A_q C_q A_q^T
  mean[j, i]            = sum_q w_jq A_q[i] K_q^-1 m_q
  cov[(j, i), (j', i')] = sum_q (w_jq w_j'q + kap_jq [j == j']) k_q(x_i, x_i') + w_jq w_j'q G_q[i, i']
  F[s]                  = mean + L z_s,  L = chol(cov + jitter I) on GPy's ladder (plain first: rung -1; then mean(diag) 1e-6 10^k, k = 0..4),
                          z_s[i] = z0 of mclp_ref.normal_pair(seed, i, s, 0)
k_q in GPy's rounding order (r2 = -2 x.z + (|x|^2 + |z|^2), clipped; r = sqrt(r2) / l; k = s2 exp(-r r / 2)).  strict=True forms G_q through
solves against the Cholesky factor of K_q -- R = A K^-1, G = (R L_q)(R L_q)^T - R A^T -- as the strict mode does.

Criterion: |got - R| <= C 2^-52 scale per entry, R the 50-digit value rounded to double and, as the issue of DESIGN 9r states it,
  scale_cov  = sum_q |coef_k| k_q(x_i, x_i') (1 + r2 / 2) + |coef_g| sum_mm' |A_im| |C_mm'| |A_i'm'|     (r2 already divided by l^2)
  scale_mean = sum_q |w_jq| sum_mm' |A_im| (1 + r2_im / 2 + c_im / 2) |K_q^-1_mm'| |m_q,m'|,   c_im = sum_p (|x_ip| + |z_mp|)^2 / l^2
(every term of the sums in absolute value; the factor 1 + r2 / 2 is the rounding of the exponential's argument; c_im, in the mean's scale
only -- the covariance's is the issue's --, is what GPy's order -2 x.z + (|x|^2 + |z|^2) cancels r2 from: 1 / l^2 = 16 000 at M = 128, P = 1).

C_ORACLE: the largest ratio of THIS file against the grid, rounded up to the next power of two (measured on the CPU with NumPy / LAPACK;
`python tools/make_joint_grid.py --measure` prints the raw figures, tests/test_joint_cpu.py re-measures them).  The device gets
C_KERNEL = max(16, 4 C_ORACLE), the convention of DESIGN 9k."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

EPS = 2.0 ** -52
GRID = os.path.join(HERE, "golden", "jointgrid.npz")
JOINT_MAXDIM = 8192
COND_FLAG = 5e2                    # the engine's ill-conditioning flag threshold: every designed case stays below it
FULL_MAX = 48                      # joint dimension up to which the grid stores the full covariance
N_SUBSET = 400                     # off-diagonal entries stored beyond it (all diagonal entries are always stored)

# Three tasks, four functions: 0 (Gaussian) | 1, 2 (HetGaussian: mean and log-variance) | 3 (Poisson)
SPECS = [("Gaussian", {"sigma": 0.5}), ("HetGaussian", {}), ("Poisson", {})]
DF = 4
TASK_OF = (0, 1, 1, 2)

# The smallest shapes at which the kernels can still go wrong: N around the 64-row tile and past two tiles, one to three functions (of
# different tasks; two of one task; out of order), every input dimension class, one and three latents, the small-model path (M = 16)
# and the regular kernels (M = 128).
CASES = (
    dict(name="s_N1", M=16, Q=1, P=1, N=1, functions=(0,), seed=11),
    dict(name="s_N63", M=16, Q=3, P=1, N=63, functions=(1, 2), seed=12),
    dict(name="s_N64", M=16, Q=3, P=2, N=64, functions=(0, 1, 3), seed=13),
    dict(name="s_N65", M=16, Q=3, P=4, N=65, functions=(3, 0), seed=14),
    dict(name="s_N129", M=16, Q=1, P=1, N=129, functions=(0, 2, 3), seed=15),
    dict(name="r_N1", M=128, Q=3, P=1, N=1, functions=(0, 1, 2), seed=21),
    dict(name="r_N63", M=128, Q=3, P=1, N=63, functions=(2, 3), seed=22),
    dict(name="r_N64", M=128, Q=3, P=4, N=64, functions=(1, 2, 3), seed=23),
    dict(name="r_N65", M=128, Q=3, P=1, N=65, functions=(0, 1), seed=24),
    dict(name="r_N129", M=128, Q=1, P=2, N=129, functions=(2,), seed=25),
)
CASE_BY_NAME = {c["name"]: c for c in CASES}
REGEN_CASES = ("s_N1", "s_N63", "s_N65")      # what tests/test_joint_cpu.py regenerates (M = 16: seconds in 50-digit arithmetic)

# measured 2026-10-20 on the CPU (NumPy / LAPACK), the larger of the default and the strict form; the raw figure beside each constant
C_ORACLE = {
    "mean": 1.0,       # raw 0.163 (s_N129)
    "cov": 128.0,      # raw 119.3 (s_N129, strict; default 118.9).  A property of GPy's rounding order in float64 that the issue's scale does
                       # not fold in: r2 = -2 x.x' + (|x|^2 + |x'|^2) cancels from terms of size 2 / l^2 (352 at M = 16, P = 1; 91.4 at r_N129,
                       # 28.9 at r_N65), so k_q(x_i, x_i') carries that many ulps.  The cases with l ~ 0.3 .. 0.9 (P > 1) stay below 1.  The
                       # device rounds k_q in the same order: against THIS file it stays within 3.
}
C_Z = 16.0             # draw-level constant of the device's normal_pair: tests/test_mclp_ref_cpu.py holds the restatement's z to 4 ulps of r
                       # (measured 0.851) against 50 digits; the device's libm gets max(16, 4 x 4) by the same convention


def c_oracle(what):
    return float(C_ORACLE[what])


def c_kernel(what):
    return max(16.0, 4.0 * C_ORACLE[what])


def c_sum(what):
    """Bound between a device result and this file's float64 value (or predict_f's): each within its own constant of R."""
    return c_kernel(what) + c_oracle(what)


# ------------------------------------------------------------------------------------------------------------ designed parameters
def inducing_grid(M, P):
    if P == 1:
        return np.linspace(0, 1, M)[:, None], 1.0 / max(M - 1, 1)
    g = int(np.ceil(M ** (1.0 / P)))
    base = np.stack(np.meshgrid(*[np.linspace(0, 1, g)] * P, indexing="ij"), -1).reshape(-1, P)[:M]
    return base, 1.0 / max(g - 1, 1)


def make_params(case):
    """(prm, Xnew) of a designed case.  Inducing inputs on a grid, lengthscale ~ the grid spacing (condition estimate below COND_FLAG); q(u)'s
    factor is banded (three sub-diagonals) so that the stored parameters stay small; kappa > 0 so that its term is exercised."""
    M, Q, P, N = case["M"], case["Q"], case["P"], case["N"]
    rng = np.random.RandomState(case["seed"])
    base, h = inducing_grid(M, P)
    Z = np.tile(base, (1, Q)) + 0.05 * h * rng.uniform(-1, 1, (M, Q * P))
    c = np.array([0.8, 1.0, 1.25])[:Q] if P == 1 else np.array([0.7, 0.8, 0.9])[:Q]
    r, cc = np.tril_indices(M)
    L_flat = np.zeros((M * (M + 1) // 2, Q))
    for q in range(Q):
        L = np.diag(rng.uniform(0.3, 0.9, M))
        for b in (1, 2, 3):
            L += np.diag(0.1 * rng.randn(M - b), -b) if M > b else 0.0
        L_flat[:, q] = L[r, cc]
    prm = dict(Z=Z, m_u=0.5 * rng.randn(M, Q), L_flat=L_flat, variance=rng.uniform(0.4, 1.5, Q), lengthscale=c * h,
               W=np.where(rng.rand(Q, DF) < 0.5, 1.0, -1.0) * rng.uniform(0.3, 1.2, (Q, DF)), kappa=rng.uniform(0.05, 0.5, (Q, DF)))
    Xnew = rng.rand(N, P)
    return prm, Xnew


def train_data(case, rows=24):
    """A few training rows per task: the engine needs an evaluation to predict from; the joint posterior depends on the parameters only."""
    rng = np.random.RandomState(1000 + case["seed"])
    X = [rng.rand(rows, case["P"]) for _ in SPECS]
    Y = [rng.randn(rows, 1), rng.randn(rows, 1), rng.poisson(1.5, (rows, 1)).astype(float)]
    return X, Y


def offdiag_subset(n, seed):
    """The seeded off-diagonal entries the grid stores for n > FULL_MAX: (rows, cols), both triangles."""
    rng = np.random.RandomState(7000 + seed)
    ri, ci = rng.randint(0, n, N_SUBSET), rng.randint(0, n, N_SUBSET)
    ci = np.where(ri == ci, (ci + 1) % n, ci)
    return ri, ci


def stored_entries(case):
    n = len(case["functions"]) * case["N"]
    if n <= FULL_MAX:
        ri, ci = np.divmod(np.arange(n * n), n)
        return ri, ci
    ri, ci = offdiag_subset(n, case["seed"])
    d = np.arange(n)
    return np.concatenate([d, ri]), np.concatenate([d, ci])


# ------------------------------------------------------------------------------------------------------------ the restatement
def r2_gpy(X, Z, ell):
    """GPy's scaled squared distance, op by op: r = sqrt(clip(-2 x.z + (|x|^2 + |z|^2), 0)) / l, returned as r * r."""
    X, Z = np.asarray(X, float), np.asarray(Z, float)
    P = X.shape[1]
    dot = X[:, None, 0] * Z[None, :, 0]
    xs, zs = X[:, 0] * X[:, 0], Z[:, 0] * Z[:, 0]
    for p in range(1, P):
        dot = dot + X[:, None, p] * Z[None, :, p]
        xs, zs = xs + X[:, p] * X[:, p], zs + Z[:, p] * Z[:, p]
    r2 = np.maximum(-2.0 * dot + (xs[:, None] + zs[None, :]), 0.0)
    r = np.sqrt(r2) / ell
    return r * r


def rbf(X, Z, var, ell):
    return var * np.exp(-0.5 * r2_gpy(X, Z, ell))


def tril_from_flat(flat, M):
    L = np.zeros((M, M))
    L[np.tril_indices(M)] = flat
    return L


def latent(prm, q, Xnew):
    """Per-latent pieces: A, K^-1 m, C (explicit), the factors, and the squared distances of A."""
    M = prm["Z"].shape[0]
    P = Xnew.shape[1]
    Zq = prm["Z"][:, q * P:(q + 1) * P]
    var, ell = float(prm["variance"][q]), float(prm["lengthscale"][q])
    K = rbf(Zq, Zq, var, ell)
    Lk = np.linalg.cholesky(K)
    Ki = np.linalg.inv(K)
    Ki = 0.5 * (Ki + Ki.T)
    Lq = tril_from_flat(prm["L_flat"][:, q], M)
    S = Lq @ Lq.T
    C = Ki @ S @ Ki - Ki
    r2A = r2_gpy(Xnew, Zq, ell)
    A = var * np.exp(-0.5 * r2A)
    canc = ((np.abs(Xnew)[:, None, :] + np.abs(Zq)[None, :, :]) ** 2).sum(-1) / (ell * ell)
    return dict(A=A, r2A=r2A, canc=canc, alpha=Ki @ prm["m_u"][:, q], C=C, Ki=Ki, Lk=Lk, Lq=Lq, var=var, ell=ell, cond=var * np.max(np.diag(Ki)))


def g_matrix(lt, strict):
    A = lt["A"]
    if not strict:
        return A @ lt["C"] @ A.T
    from scipy.linalg import cho_solve
    R = cho_solve((lt["Lk"], True), A.T).T
    T = R @ lt["Lq"]
    return T @ T.T - R @ A.T


def joint(prm, Xnew, functions, strict=False, return_scale=False):
    """(mean (nD, N), cov (n, n)) in float64; with return_scale also (scale_mean (nD, N), scale_cov (n, n))."""
    Xnew = np.asarray(Xnew, float)
    N, Q = Xnew.shape[0], prm["variance"].shape[0]
    d = list(functions)
    nD = len(d)
    mean, cov = np.zeros((nD, N)), np.zeros((nD, N, nD, N))
    smean, scov = np.zeros((nD, N)), np.zeros((nD, N, nD, N))
    for q in range(Q):
        lt = latent(prm, q, Xnew)
        G = g_matrix(lt, strict)
        G = np.tril(G) + np.tril(G, -1).T                  # the lower triangle, mirrored
        r2 = r2_gpy(Xnew, Xnew, lt["ell"])
        k = lt["var"] * np.exp(-0.5 * r2)
        w, kap = prm["W"][q, d], prm["kappa"][q, d]
        p = lt["A"] @ lt["alpha"]
        mean += w[:, None] * p[None, :]
        ww = w[:, None] * w[None, :]
        ck = ww + np.diag(kap)
        cov += ck[:, None, :, None] * k[None, :, None, :] + ww[:, None, :, None] * G[None, :, None, :]
        if return_scale:
            aA = np.abs(lt["A"])
            smean += np.abs(w)[:, None] * ((aA * (1.0 + 0.5 * lt["r2A"] + 0.5 * lt["canc"])) @ (np.abs(lt["Ki"]) @ np.abs(prm["m_u"][:, q])))[None, :]
            sk, sg = k * (1.0 + 0.5 * r2), aA @ np.abs(lt["C"]) @ aA.T
            scov += np.abs(ck)[:, None, :, None] * sk[None, :, None, :] + np.abs(ww)[:, None, :, None] * sg[None, :, None, :]
    n = nD * N
    if return_scale:
        return mean, cov.reshape(n, n), smean, scov.reshape(n, n)
    return mean, cov.reshape(n, n)


def predict_f(prm, Xnew):
    """q(f) as `hmogp_predict_f` forms it: m, v [N, Df], v before any abs."""
    Xnew = np.asarray(Xnew, float)
    N, Q = Xnew.shape[0], prm["variance"].shape[0]
    Df = prm["W"].shape[1]
    m, v = np.zeros((N, Df)), np.zeros((N, Df))
    for q in range(Q):
        lt = latent(prm, q, Xnew)
        p, c = lt["A"] @ lt["alpha"], np.einsum("im,mk,ik->i", lt["A"], lt["C"], lt["A"])
        w, kap = prm["W"][q], prm["kappa"][q]
        m += p[:, None] * w[None, :]
        v += (w * w + kap)[None, :] * lt["var"] + (w * w)[None, :] * c[:, None]
    return m, v


def cond_estimates(prm, P):
    X0 = np.zeros((1, P))
    return [latent(prm, q, X0)["cond"] for q in range(prm["variance"].shape[0])]


# ------------------------------------------------------------------------------------------------------------ the sampler
def jitchol(cov):
    """(L, jitter, rung) on the ladder of `hmogp_jitchol_inv`: plain first (rung -1, jitter 0), then mean(diag) 1e-6 10^k for k = 0 .. 4."""
    try:
        return np.linalg.cholesky(cov), 0.0, -1
    except np.linalg.LinAlgError:
        pass
    dm = float(np.mean(np.diag(cov)))
    for k in range(5):
        jit = dm * 1e-6 * 10.0 ** k
        try:
            return np.linalg.cholesky(cov + jit * np.eye(cov.shape[0])), jit, k
        except np.linalg.LinAlgError:
            continue
    raise np.linalg.LinAlgError("not positive definite, even with jitter.")


def chol_backward(cov, L, jitter):
    """max |L L^T - (cov + jitter I)| in units of n 2^-52 max diag(cov)."""
    n = cov.shape[0]
    return float(np.max(np.abs(L @ L.T - (cov + jitter * np.eye(n)))) / (n * EPS * np.max(np.diag(cov))))


def normals(seed, n, S):
    """z [S, n]: z_s[i] = z0 of normal_pair(seed, row i, sample s, pair 0)."""
    import mclp_ref as mr
    z0, _ = mr.normal_pair(int(seed), np.arange(n).reshape(1, -1), np.arange(S).reshape(-1, 1), 0)
    return z0


def sample(mean, cov, S, seed):
    """F [S, n] = mean + L z_s, with the factor, the jitter and the rung."""
    L, jit, rung = jitchol(cov)
    z = normals(seed, cov.shape[0], S)
    m = np.asarray(mean, float).reshape(-1)
    return np.stack([m + L @ zs for zs in z]), L, jit, rung      # (one product per draw: BLAS blocks z @ L.T by the number of draws)


# ------------------------------------------------------------------------------------------------------------ the grid
def load_grid(path=GRID):
    g = np.load(path)
    out = {}
    for c in CASES:
        k = c["name"] + "/"
        prm = {key: g[k + key] for key in ("Z", "m_u", "L_flat", "variance", "lengthscale", "W", "kappa")}
        out[c["name"]] = dict(case=c, prm=prm, Xnew=g[k + "Xnew"], mean=g[k + "mean"], mean_scale=g[k + "mean_scale"], ri=g[k + "ri"],
                              ci=g[k + "ci"], cov=g[k + "cov"], cov_scale=g[k + "cov_scale"])
    return out


def ratios(got, R, scale):
    """|got - R| / (2^-52 scale) per entry (0 where both are equal, inf where a value is not finite)."""
    got, R, scale = np.asarray(got, float), np.asarray(R, float), np.asarray(scale, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - R) / (EPS * scale)
    r = np.where(got == R, 0.0, r)
    return np.where(np.isfinite(got), r, np.inf)


def case_ratios(entry, mean, cov):
    """(worst mean ratio, worst cov ratio) of a result (mean (nD, N), cov (n, n)) against a loaded grid case."""
    rm = ratios(np.asarray(mean).reshape(-1), entry["mean"], entry["mean_scale"])
    rc = ratios(np.asarray(cov)[entry["ri"], entry["ci"]], entry["cov"], entry["cov_scale"])
    return float(np.max(rm)), float(np.max(rc))


# ------------------------------------------------------------------------------------------------------------ the factor, the singular and the statistical case
# NumPy's (LAPACK's) own |L L^T - (cov + jitter I)| on the designed cases, in units of n 2^-52 max diag: measured 2026-10-20, worst 0.786
# (s_N1; every n > 3 case below 0.05), rounded up; the device gets max(16, 4 x) that
C_CHOL_LAPACK = 1.0
C_CHOL_KERNEL = max(16.0, 4.0 * C_CHOL_LAPACK)

SINGULAR_SEED, SINGULAR_DRAWS = 11, 16
SINGULAR_TWINS = ((0, 3), (1, 4), (2, 5))      # rows of Xnew that are identical


def singular_case():
    """(prm, Xnew, functions): six inputs, the last three repeating the first three -- cov is exactly singular (n = 12, rank 6)."""
    prm, _ = make_params(CASE_BY_NAME["s_N64"])
    x = np.random.RandomState(41).rand(3, 2)
    return prm, np.vstack([x, x]), (0, 1)


STAT_SEED, STAT_DRAWS = 2024, 4096
STAT_FALSE_ALARM = 1e-6                         # overall, split evenly over the statistics (Bonferroni)


def stat_case():
    """(prm, Xnew, functions): n = 8 -- four spread-out inputs, two functions of different tasks."""
    prm, _ = make_params(CASE_BY_NAME["s_N64"])
    return prm, np.random.RandomState(99).rand(4, 2), (0, 3)


def stat_count(n):
    return 2 * n + n * (n - 1)                  # n means, n variances, two statistics per pair


def stat_threshold(n):
    """|z| beyond which one of the stat_count(n) statistics rejects at the overall level STAT_FALSE_ALARM."""
    from scipy import stats
    return float(stats.norm.isf(STAT_FALSE_ALARM / stat_count(n) / 2.0))


def stat_zscores(F, mean, cov):
    """(max |z| over the n sample means, max equivalent |z| over the second-moment statistics) of draws F [S, n] under N(mean, cov).
    Every statistic has an EXACT law: the sample mean is normal; with the mean known, sum_s d_i^2 / c_ii is chi-square with S degrees of
    freedom, and so are sum_s (d_i / s_i + d_j / s_j)^2 / (2 (1 + rho)) and sum_s (d_i / s_i - d_j / s_j)^2 / (2 (1 - rho)) for a pair --
    together they hold c_ij.  A chi-square p-value is reported as the |z| of the same two-sided normal p-value."""
    from scipy import stats
    F, mean = np.asarray(F, float), np.asarray(mean, float).reshape(1, -1)
    S, n = F.shape
    sd = np.sqrt(np.diag(cov))
    D = (F - mean) / sd[None, :]
    zm = float(np.max(np.abs(D.mean(0)) * np.sqrt(S)))
    chi = [np.sum(D[:, i] ** 2) for i in range(n)]
    for i in range(n):
        for j in range(i):
            rho = cov[i, j] / (sd[i] * sd[j])
            chi.append(np.sum((D[:, i] + D[:, j]) ** 2) / (2.0 * (1.0 + rho)))
            chi.append(np.sum((D[:, i] - D[:, j]) ** 2) / (2.0 * (1.0 - rho)))
    chi = np.array(chi)
    p = 2.0 * np.minimum(stats.chi2.cdf(chi, S), stats.chi2.sf(chi, S))
    return zm, float(np.max(stats.norm.isf(np.maximum(p, 1e-300) / 2.0)))
