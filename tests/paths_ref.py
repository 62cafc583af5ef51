"""float64 NumPy restatement of the pathwise (Matheron) posterior samples (`hmogp_paths_*`; csrc/paths.hip and `hmogp_engine::paths_create` /
`paths_eval` of csrc/engine_optim.hip), the designed cases, the loader / criteria of their grid tests/golden/pathsgrid.npz
(tools/make_paths_grid.py; 50-digit values from tests/paths_ref_mp.py).

A path set = (functions d_1 .. d_nD, S samples, Lf frequencies per latent, seed), from the raw parameters of tests/joint_ref.py:
  draws (z0 of mclp_ref.normal_pair(seed, n, s, pair)):
    zeta[q, l, p]      n = l,            s = 4 q + p,  pair 1        omega = zeta / (pi l_q), formed once: the STORED value is the contract
    theta[q, s, k]     n = k < 2 Lf,     s = s Q + q,  pair 2
    eps[q, s, m]       n = m < M,        s = s Q + q,  pair 3
    thetak[j, q, s, k] n = d_j 2 Lf + k, s = s Q + q,  pair 4        (d_j the function's index, not its position j)
  features  t_l(x) = sum_p omega[q, l, p] x_p (p order), c_q = sqrt(variance_q / Lf), phi[l] = c_q cos(pi t_l), phi[Lf + l] = c_q sin(pi t_l)
  state     u[q, s] = m_q + L_q eps[q, s];  v[q, s] = K_q^-1 (u[q, s] - Phi_q(Z_q) theta[q, s])
            theta~[q, k, s, j] = w_jq theta[q, s, k] + sqrt(kappa_jq) thetak[j, q, s, k];   v~[q, m, s, j] = w_jq v[q, s, m]
  paths     F[s, j, i] = sum_q phi_q(x_i) . theta~[q, :, s, j] + k_q(x_i, Z_q) . v~[q, :, s, j]
K_q and k_q(x, Z_q) in GPy's rounding order (joint_ref.rbf), as K_uu and the strict K_uf are built on the device.

Criteria: |got - R| <= C 2^-52 scale per entry, R the 50-digit value rounded to double and
  scale_theta = |w| |theta| + sqrt(kappa) |thetak|                                           (draw level: C_Z ulps of each normal)
  scale_u     = |m| + |L_q| |eps|
  scale_v     = |w| |K^-1| ( |m| + |L_q| |eps| + sum_k |Phi_Z,k| |theta_k| (1 + pi sum_p |omega_kp z_p|) + |Luu| |Luu^T| |v| )
  scale_F     = sum_q [ c_q sum_k |theta~_k| (1 + pi sum_p |omega_kp x_p|) + sum_m |a_m| |v~_m| (1 + r2 / 2 + c / 2) ]
(c: what GPy's order cancels r2 from, as in joint_ref's mean scale).  The evaluation is always held against the 50-digit evaluation FROM THE
STATE IT WAS GIVEN (the device's own, read back), so the solve's error does not compound; scale_F carries no K.

C_ORACLE: the largest ratio of THIS file against the grid, rounded up to the next power of two (`python tools/make_paths_grid.py --measure`
prints the raw figures; tests/test_paths_cpu.py re-measures them).  The device gets max(16, 4 C_ORACLE), the convention of DESIGN 9k."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import joint_ref as jr            # noqa: E402
import mclp_ref as mr             # noqa: E402

EPS = jr.EPS
GRID = os.path.join(HERE, "golden", "pathsgrid.npz")
SPECS, DF, TASK_OF = jr.SPECS, jr.DF, jr.TASK_OF
MAXFEAT, MAXCOLS, MAXSETS = 8192, 4096, 16
TAG_FREQ, TAG_PRIOR, TAG_QU, TAG_KAPPA = 1, 2, 3, 4
FULL_MAX = 400                     # entries up to which the grid stores an array in full; beyond it N_SUBSET seeded entries
N_SUBSET = 200
GRID_SEED = 7                      # the seed of every designed path set

# The model set-up of DESIGN 9r's grid (same seeds: the same parameters), with the path set's own shape classes: S in {1, 3, 8}, Lf in
# {1, 8, 50, 64} (2 x 50 = 100 is no multiple of the GEMM's k-block of 32; contraction lengths stay <= 2 x 64 + 128).
CASES = (
    dict(name="s_N1", M=16, Q=1, P=1, N=1, functions=(0,), seed=11, S=1, Lf=1),
    dict(name="s_N63", M=16, Q=3, P=1, N=63, functions=(1, 2), seed=12, S=3, Lf=8),
    dict(name="s_N64", M=16, Q=3, P=2, N=64, functions=(0, 1, 3), seed=13, S=8, Lf=50),
    dict(name="s_N65", M=16, Q=3, P=4, N=65, functions=(3, 0), seed=14, S=3, Lf=64),
    dict(name="s_N129", M=16, Q=1, P=1, N=129, functions=(0, 2, 3), seed=15, S=8, Lf=8),
    dict(name="r_N1", M=128, Q=3, P=1, N=1, functions=(0, 1, 2), seed=21, S=3, Lf=64),
    dict(name="r_N63", M=128, Q=3, P=1, N=63, functions=(2, 3), seed=22, S=8, Lf=1),
    dict(name="r_N64", M=128, Q=3, P=4, N=64, functions=(1, 2, 3), seed=23, S=1, Lf=50),
    dict(name="r_N65", M=128, Q=3, P=1, N=65, functions=(0, 1), seed=24, S=3, Lf=64),
    dict(name="r_N129", M=128, Q=1, P=2, N=129, functions=(2,), seed=25, S=8, Lf=50),
)
CASE_BY_NAME = {c["name"]: c for c in CASES}
REGEN_CASES = ("s_N1", "s_N63", "s_N129")      # what tests/test_paths_cpu.py regenerates (M = 16, short features: seconds in 50 digits)

# measured 2026-10-21 on the CPU (NumPy / LAPACK); the raw figure beside each constant
C_ORACLE = {
    "u": 2.0,          # raw 1.548 (r_N64): the restated normals are themselves within 4 ulps of the 50-digit ones (measured 1.64 here)
    "v": 1024.0,       # raw 820.4 (r_N63; 311.6 r_N1, 204.1 r_N65, 7.9 s_N63, below 5 elsewhere).  A property of GPy's rounding order of K_q in
                       # float64 that scale_v does not fold in, as for the covariance of DESIGN 9r: r2 = -2 z.z' + (|z|^2 + |z'|^2)
                       # cancels from terms of size 2 / l^2 (32 000 at M = 128, P = 1; 352 at M = 16, P = 1), so K_q carries that many ulps
                       # and v = K_q^-1 (..) inherits them through |K^-1| |dK| |v|.  The cases with l ~ 0.3 .. 0.9 (P > 1) stay below 2.  The
                       # device builds K_uu in the same order.
    "F": 1.0,          # raw 0.391 (s_N129)
}
C_Z = jr.C_Z           # draw-level constant of the device's normal_pair: 16 ulps of |z|


def c_oracle(what):
    return float(C_ORACLE[what])


def c_kernel(what):
    return max(16.0, 4.0 * C_ORACLE[what])


make_params, train_data, ratios = jr.make_params, jr.train_data, jr.ratios


# ------------------------------------------------------------------------------------------------------------ the draws
def normals(seed, n, s, pair):
    return mr.normal_pair(int(seed), np.asarray(n), np.asarray(s), pair)[0]


def draws(seed, Q, P, M, S, Lf, functions):
    """dict(zeta [Q, Lf, P], theta [Q, S, 2 Lf], eps [Q, S, M], thetak [nD, Q, S, 2 Lf])."""
    q, s = np.arange(Q), np.arange(S)
    sq = s[None, :, None] * Q + q[:, None, None]
    d = np.asarray(list(functions))
    return dict(zeta=normals(seed, np.arange(Lf)[None, :, None], q[:, None, None] * 4 + np.arange(P)[None, None, :], TAG_FREQ),
                theta=normals(seed, np.arange(2 * Lf)[None, None, :], sq, TAG_PRIOR),
                eps=normals(seed, np.arange(M)[None, None, :], sq, TAG_QU),
                thetak=normals(seed, d[:, None, None, None] * 2 * Lf + np.arange(2 * Lf)[None, None, None, :], sq[None], TAG_KAPPA))


def used_triples(Q, P, M, S, Lf, functions):
    """Every (n, s, pair) triple a set draws, as one integer array [count, 3] (the stream-separation test counts the distinct ones)."""
    out = []
    q, s = np.arange(Q), np.arange(S)
    sq = (s[None, :] * Q + q[:, None]).reshape(-1)
    for n, ss, tag in ((np.arange(Lf), (q[:, None] * 4 + np.arange(P)[None, :]).reshape(-1), TAG_FREQ), (np.arange(2 * Lf), sq, TAG_PRIOR),
                       (np.arange(M), sq, TAG_QU)):
        a, b = np.meshgrid(n, ss, indexing="ij")
        out.append(np.stack([a.ravel(), b.ravel(), np.full(a.size, tag)], 1))
    for d in functions:
        a, b = np.meshgrid(d * 2 * Lf + np.arange(2 * Lf), sq, indexing="ij")
        out.append(np.stack([a.ravel(), b.ravel(), np.full(a.size, TAG_KAPPA)], 1))
    return np.concatenate(out).astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ the features
def sincospi(t):
    """(sin(pi t), cos(pi t)) with the exact argument reduction of the device's sincospi: r = t - 2 round(t / 2) is exact in float64."""
    r = t - 2.0 * np.round(0.5 * t)
    return np.sin(np.pi * r), np.cos(np.pi * r)


def features(omega_q, c, X):
    """(Phi [N, 2 Lf], sum_p |omega_lp x_p| [N, Lf]) of one latent: t summed in p order."""
    X = np.asarray(X, float)
    t = X[:, None, 0] * omega_q[None, :, 0]
    at = np.abs(t)
    for p in range(1, X.shape[1]):
        t = t + X[:, None, p] * omega_q[None, :, p]
        at = at + np.abs(X[:, None, p] * omega_q[None, :, p])
    sn, cs = sincospi(t)
    return np.concatenate([c * cs, c * sn], 1), at


def latent_q(prm, q, P):
    M = prm["Z"].shape[0]
    Zq = prm["Z"][:, q * P:(q + 1) * P]
    var, ell = float(prm["variance"][q]), float(prm["lengthscale"][q])
    K = jr.rbf(Zq, Zq, var, ell)
    return dict(Zq=Zq, var=var, ell=ell, K=K, Lk=np.linalg.cholesky(K), Lq=jr.tril_from_flat(prm["L_flat"][:, q], M), m=prm["m_u"][:, q])


# ------------------------------------------------------------------------------------------------------------ the state
def state(prm, P, functions, S, Lf, seed, return_scale=False):
    """dict(omega [Q, Lf, P], theta [Q, 2 Lf, S, nD], v [Q, M, S, nD], u [Q, S, M]) -- the arrays of `hmogp_paths_state` -- and with
    return_scale the scales of theta, u, v under the same keys of a second dict."""
    from scipy.linalg import cho_solve
    M, Q = prm["m_u"].shape
    d = list(functions)
    nD = len(d)
    dr = draws(seed, Q, P, M, S, Lf, d)
    omega = np.stack([dr["zeta"][q] / (np.pi * float(prm["lengthscale"][q])) for q in range(Q)])
    st = dict(omega=omega, theta=np.zeros((Q, 2 * Lf, S, nD)), v=np.zeros((Q, M, S, nD)), u=np.zeros((Q, S, M)))
    sc = dict(theta=np.zeros((Q, 2 * Lf, S, nD)), v=np.zeros((Q, M, S, nD)), u=np.zeros((Q, S, M)))
    for q in range(Q):
        lt = latent_q(prm, q, P)
        PhiZ, atZ = features(omega[q], np.sqrt(lt["var"] / Lf), lt["Zq"])
        w, sk = prm["W"][q, d], np.sqrt(prm["kappa"][q, d])
        th, thk = dr["theta"][q], dr["thetak"][:, q]                        # [S, 2 Lf], [nD, S, 2 Lf]
        u = lt["m"][None, :] + dr["eps"][q] @ lt["Lq"].T                    # [S, M]
        v = cho_solve((lt["Lk"], True), (u - th @ PhiZ.T).T).T             # [S, M]
        st["u"][q] = u
        st["theta"][q] = (w[None, None, :] * th.T[:, :, None]) + sk[None, None, :] * np.transpose(thk, (2, 1, 0))
        st["v"][q] = v.T[:, :, None] * w[None, None, :]
        if return_scale:
            Ki = np.linalg.inv(lt["K"])
            su = np.abs(lt["m"])[None, :] + np.abs(dr["eps"][q]) @ np.abs(lt["Lq"]).T
            grow = 1.0 + np.pi * np.concatenate([atZ, atZ], 1)                # [M, 2 Lf]
            inner = su + np.abs(th) @ (np.abs(PhiZ) * grow).T + np.abs(v) @ (np.abs(lt["Lk"]) @ np.abs(lt["Lk"]).T).T
            sv = inner @ np.abs(Ki).T                                        # [S, M]
            sc["u"][q] = su
            sc["theta"][q] = np.abs(w)[None, None, :] * np.abs(th).T[:, :, None] + sk[None, None, :] * np.abs(np.transpose(thk, (2, 1, 0)))
            sc["v"][q] = sv.T[:, :, None] * np.abs(w)[None, None, :]
    return (st, sc) if return_scale else st


def synthetic_state(case, prm):
    """A designed state for the evaluation grid: seeded arrays of the real state's shapes and sizes (the evaluation is a function of a
    GIVEN state; LAPACK's own state is not bit-stable across machines, a seeded one is)."""
    rng = np.random.RandomState(5000 + case["seed"])
    Q, M, P, S, Lf, nD = case["Q"], case["M"], case["P"], case["S"], case["Lf"], len(case["functions"])
    omega = rng.randn(Q, Lf, P) / (np.pi * prm["lengthscale"][:, None, None])
    return dict(omega=omega, theta=rng.randn(Q, 2 * Lf, S, nD), v=rng.randn(Q, M, S, nD) * 0.7, u=np.zeros((Q, S, M)))


# ------------------------------------------------------------------------------------------------------------ the evaluation
def evaluate(st, prm, P, Xnew, return_scale=False):
    """F [S, nD, N] from a given state (its omega, theta, v); with return_scale also scale_F."""
    Xnew = np.asarray(Xnew, float).reshape(-1, P)
    Q, K2, S, nD = st["theta"].shape
    Lf, N = K2 // 2, Xnew.shape[0]
    F, sF = np.zeros((S, nD, N)), np.zeros((S, nD, N))
    for q in range(Q):
        lt = latent_q(prm, q, P)
        c = np.sqrt(lt["var"] / Lf)
        Phi, at = features(st["omega"][q], c, Xnew)
        r2 = jr.r2_gpy(Xnew, lt["Zq"], lt["ell"])
        A = lt["var"] * np.exp(-0.5 * r2)
        F += np.einsum("ik,ksj->sji", Phi, st["theta"][q]) + np.einsum("im,msj->sji", A, st["v"][q])
        if return_scale:
            canc = ((np.abs(Xnew)[:, None, :] + np.abs(lt["Zq"])[None, :, :]) ** 2).sum(-1) / (lt["ell"] * lt["ell"])
            grow = c * (1.0 + np.pi * np.concatenate([at, at], 1))
            sF += np.einsum("ik,ksj->sji", grow, np.abs(st["theta"][q])) + np.einsum("im,msj->sji", np.abs(A) * (1.0 + 0.5 * r2 + 0.5 * canc),
                                                                                   np.abs(st["v"][q]))
    return (F, sF) if return_scale else F


# ------------------------------------------------------------------------------------------------------------ the law given the frequencies
def _pieces(omega, prm, P, functions, Xnew):
    from scipy.linalg import cho_solve
    Xnew = np.asarray(Xnew, float).reshape(-1, P)
    Q, Lf = omega.shape[0], omega.shape[1]
    out = []
    for q in range(Q):
        lt = latent_q(prm, q, P)
        c = np.sqrt(lt["var"] / Lf)
        Phi, PhiZ = features(omega[q], c, Xnew)[0], features(omega[q], c, lt["Zq"])[0]
        A = jr.rbf(Xnew, lt["Zq"], lt["var"], lt["ell"])
        R = cho_solve((lt["Lk"], True), A.T).T                             # A K^-1
        out.append(dict(lt, Phi=Phi, PhiZ=PhiZ, A=A, R=R, w=prm["W"][q, list(functions)], kap=prm["kappa"][q, list(functions)]))
    return out


def cond_cov(omega, prm, P, functions, Xnew):
    """Covariance [n, n] (function-major, n = nD N) of the paths GIVEN the frequencies, from the paths' own linear form: f = mean + B xi with
    xi = (theta, thetak, eps) standard normal, cov = B B^T block by block."""
    pcs = _pieces(omega, prm, P, functions, Xnew)
    nD, N = len(list(functions)), pcs[0]["A"].shape[0]
    cov = np.zeros((nD, N, nD, N))
    for pc in pcs:
        Bt = pc["Phi"] - pc["R"] @ pc["PhiZ"]                              # d f / d theta (per unit w)
        Be = pc["R"] @ pc["Lq"]                                            # d f / d eps
        core = Bt @ Bt.T + Be @ Be.T
        pp = pc["Phi"] @ pc["Phi"].T
        ww = pc["w"][:, None] * pc["w"][None, :]
        cov += ww[:, None, :, None] * core[None, :, None, :] + np.diag(pc["kap"])[:, None, :, None] * pp[None, :, None, :]
    return cov.reshape(nD * N, nD * N)


def cond_cov_formula(omega, prm, P, functions, Xnew):
    """The same covariance as DESIGN 9r's formula with k_q(x, x') replaced by phi_q(x)^T phi_q(x'): (w w' + kappa [j == j']) phi^T phi' + w w'
    (G_q + E_q), G_q = A C_q A^T as 9r forms it (joint_ref.g_matrix, strict form) and E_q = R D - (Phi Phi_Z^T - R Phi_Z Phi_Z^T) R^T, D = A^T -
    Phi_Z Phi^T, the term that vanishes where the features reproduce k_q at the inducing inputs (R = A K^-1)."""
    pcs = _pieces(omega, prm, P, functions, Xnew)
    nD, N = len(list(functions)), pcs[0]["A"].shape[0]
    cov = np.zeros((nD, N, nD, N))
    for pc in pcs:
        G = jr.g_matrix(dict(A=pc["A"], Lk=pc["Lk"], Lq=pc["Lq"]), True)
        D = pc["A"].T - pc["PhiZ"] @ pc["Phi"].T
        E = pc["R"] @ D - (pc["Phi"] @ pc["PhiZ"].T - pc["R"] @ pc["PhiZ"] @ pc["PhiZ"].T) @ pc["R"].T
        pp = pc["Phi"] @ pc["Phi"].T
        ww = pc["w"][:, None] * pc["w"][None, :]
        ck = ww + np.diag(pc["kap"])
        cov += ck[:, None, :, None] * pp[None, :, None, :] + ww[:, None, :, None] * (G + E)[None, :, None, :]
    return cov.reshape(nD * N, nD * N)


def freq_terms(omega, prm, P, functions, Xnew):
    """(const [n, n], T [Lf, n, n]): cond_cov = const + mean_l T_l, T_l the contribution of frequency l of every latent (i.i.d. over l, with
    mean exact covariance - const): g_l(i) = psi_l(x_i) - sum_m R_im psi_l(z_m), psi_l = sqrt(variance) (cos, sin)(pi t_l)."""
    pcs = _pieces(omega, prm, P, functions, Xnew)
    nD, N = len(list(functions)), pcs[0]["A"].shape[0]
    Lf = omega.shape[1]
    const, T = np.zeros((nD, N, nD, N)), np.zeros((Lf, nD, N, nD, N))
    for pc in pcs:
        ww = pc["w"][:, None] * pc["w"][None, :]
        Be = pc["R"] @ pc["Lq"]
        const += ww[:, None, :, None] * (Be @ Be.T)[None, :, None, :]
        s = np.sqrt(Lf)                                                    # phi = psi / sqrt(Lf)
        psi = s * np.stack([pc["Phi"][:, :Lf], pc["Phi"][:, Lf:]], -1)     # [N, Lf, 2]
        psz = s * np.stack([pc["PhiZ"][:, :Lf], pc["PhiZ"][:, Lf:]], -1)   # [M, Lf, 2]
        g = psi - np.einsum("im,mlc->ilc", pc["R"], psz)
        gg, pp = np.einsum("ilc,jlc->lij", g, g), np.einsum("ilc,jlc->lij", psi, psi)
        T += ww[None, :, None, :, None] * gg[:, None, :, None, :] + np.diag(pc["kap"])[None, :, None, :, None] * pp[:, None, :, None, :]
    n = nD * N
    return const.reshape(n, n), T.reshape(Lf, n, n)


def feature_error_z(omega, prm, P, functions, Xnew, exact_cov):
    """(worst |z|, worst absolute error) of the conditional covariance against the exact one, entry by entry on the lower triangle: each entry
    is const + a mean of Lf i.i.d. terms, tested with the terms' sample standard deviation."""
    const, T = freq_terms(omega, prm, P, functions, Xnew)
    Lf, n = T.shape[0], T.shape[1]
    il = np.tril_indices(n)
    mean, sd = T.mean(0)[il], T.std(0, ddof=1)[il]
    err = const[il] + mean - np.asarray(exact_cov)[il]
    return float(np.max(np.abs(err) / (sd / np.sqrt(Lf)))), float(np.max(np.abs(err))), len(il[0])


# ------------------------------------------------------------------------------------------------------------ the statistical case
STAT_SEED, STAT_DRAWS, STAT_FEATURES = 2024, 4096, 64
STAT_FALSE_ALARM = jr.STAT_FALSE_ALARM
FEAT_FEATURES, FEAT_SEED = 4096, 77
stat_case, stat_zscores, stat_threshold = jr.stat_case, jr.stat_zscores, jr.stat_threshold


def z_threshold(count):
    """|z| beyond which one of `count` two-sided statistics rejects at the overall level STAT_FALSE_ALARM (Bonferroni)."""
    from scipy import stats
    return float(stats.norm.isf(STAT_FALSE_ALARM / count / 2.0))


# ------------------------------------------------------------------------------------------------------------ the grid
def subset(size, seed):
    """Flat indices the grid stores of an array of `size` entries: all of them up to FULL_MAX, else N_SUBSET seeded ones."""
    if size <= FULL_MAX:
        return np.arange(size)
    return np.sort(np.random.RandomState(9000 + seed).choice(size, N_SUBSET, replace=False))


def load_grid(path=GRID):
    g = np.load(path)
    out = {}
    for c in CASES:
        k = c["name"] + "/"
        if k + "zeta" not in g.files:          # (a grid being written case by case)
            continue
        prm, Xnew = make_params(c)
        out[c["name"]] = dict(case=c, prm=prm, Xnew=Xnew, **{key[len(k):]: g[key] for key in g.files if key.startswith(k)})
    return out


def pick(a, idx):
    return np.asarray(a, float).reshape(-1)[idx]


def state_ratios(entry, st):
    """Worst ratio of a state's theta, u, v against a loaded grid case (omega is held through the draws: see draw_ratios)."""
    return {k: float(np.max(ratios(pick(st[k], entry["i_" + k]), entry[k], entry[k + "_scale"]))) for k in ("theta", "u", "v")}


def draw_ratios(entry, st):
    """Worst |omega pi l - zeta| / (2^-52 |zeta|) and |theta~ - R| / (2^-52 scale_theta) against the 50-digit draws: the draw level."""
    ell = entry["prm"]["lengthscale"][:, None, None]
    rz = ratios(st["omega"] * (np.pi * ell), entry["zeta"], np.abs(entry["zeta"]))
    rt = ratios(pick(st["theta"], entry["i_theta"]), entry["theta"], entry["theta_scale"])
    return float(np.max(rz)), float(np.max(rt))
