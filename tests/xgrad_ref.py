"""float64 NumPy restatement of the gradients of q(f) with respect to the new inputs (`hmogp_qf_input_grad` / `hmogp_predict_f_grad`;
csrc/xgrad.hip and `hmogp_engine::predict_f_grad` of csrc/engine_optim.hip), the designed cases, and the loader / criterion of
their grid tests/golden/xgradgrid.npz (tools/make_xgrad_grid.py; 50-digit values from tests/xgrad_ref_mp.py).

For row x, latent q, function d (Z_q = Z[:, q P : q P + P]):
  k_qm = variance_q exp(-r_qm^2 / 2 l_q^2),   t_qm = sum_m' k_qm' C_q,m'm          (one row of A_q C_q)
  gp_qj = (1 / l_q^2) sum_m a_qm k_qm (z_qmj - x_j),   gc_qj = (2 / l_q^2) sum_m t_qm k_qm (z_qmj - x_j)
  dm[i, d, j] = sum_q W_qd gp_qj,   dv[i, d, j] = sum_q W_qd^2 gc_qj               (v the SIGNED variance: no abs)
k_qm in GPy's rounding order (joint_ref.r2_gpy), the order both device variants follow up to the last bits.

Criterion: |got - R| <= C (2^-52 S + 2^-1022 F) per entry, R the 50-digit value rounded to double and
  e_qm    = 1 + (|x|^2 + |z_qm|^2 + 2 sum_p |x_p| |z_qmp|) / (2 l_q^2) + r_qm^2 / (2 l_q^2)
  S_gp,qj = (1 / l_q^2) sum_m |a_qm| k_qm e_qm |z_qmj - x_j|
  S_gc,qj = (2 / l_q^2) sum_m (sum_m' |C_q,m'm| k_qm' e_qm') k_qm e_qm |z_qmj - x_j|
  S_dm = sum_q |W_qd| S_gp,   S_dv = sum_q W_qd^2 S_gc
e_qm is the rounding of the exponential's argument INCLUDING what GPy's order -2 x.z + (|x|^2 + |z|^2) cancels r^2 from.  The floor, for
kernels that underflow (a result in the subnormal range carries an ABSOLUTE error of up to 2^-1075 variance, whatever its size):
  F_dm = sum_q |W_qd| (1 / l_q^2) sum_m |a_qm| |z_qmj - x_j|
  F_dv = sum_q W_qd^2 (2 / l_q^2) variance_q sum_m (sum_m' |C_q,m'm|) |z_qmj - x_j|
(F_dv: t_qm's absolute error is sum_m' |C_q,m'm| times that of k_qm', and it is multiplied by k_qm <= variance_q; the other factor
variance_q of k_qm' and the 2^-1075 against 2^-1022 leave 2^52 of room.)  The scale itself is evaluated with r^2 = sum_p (x_p - z_p)^2.

C_ORACLE: the largest ratio of THIS file against the grid, rounded up to the next power of two; `python tools/make_xgrad_grid.py --measure`
prints the raw figures, tests/test_xgrad_cpu.py re-measures them.  The device gets C_KERNEL = max(16, 4 C_ORACLE), the rule of DESIGN 9k.

Strict engine path: T = ((A K^-1) L_q L_q^T - A) K^-1 through solves against the factor of K_uu.  Its reference is the 50-digit chain from
(Z, m_u, L_flat, hypers) (xgrad_ref_mp.chain_reference), its scale S x the engine's returned cond_est (max over the latents), and its own
C_ORACLE_STRICT is measured from `chain(..., strict=True)` below, the float64 copy of the solve-based form."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import joint_ref as jr            # noqa: E402

EPS = 2.0 ** -52
TINY = 2.0 ** -1022
GRID = os.path.join(HERE, "golden", "xgradgrid.npz")
MAX_ROWS = 24                      # rows per case the grid holds at 50 digits
FAR = 40.0                         # the far row: at least this many lengthscales from every inducing input (every k underflows to 0)

# The kernel's own boundaries.  N: lane, wave, the four-row block, several blocks.  M: the lane pair (1, 2), odd M's 8-byte path (63, 65,
# 127, 129), one and two rounds of the wave (<= 128 | > 128).  P = 1..4; Q = 1, 3; Df = 1, 4 (dense W: the functions share the latents; one
# entry exactly 0); both rbf variants; `shift`: inputs offset by 10 (the cancellation of GPy's r^2 order); small and large lengthscales.
CASES = (
    dict(name="M1_N1", N=1, M=1, P=1, Q=1, Df=1, exact=True, ell=(0.3,), shift=0.0, seed=101),
    dict(name="M2_N63", N=63, M=2, P=2, Q=3, Df=4, exact=False, ell=(0.9, 0.4, 0.6), shift=0.0, seed=102),
    dict(name="M63_N64", N=64, M=63, P=3, Q=1, Df=4, exact=True, ell=(0.5,), shift=0.0, seed=103),
    dict(name="M64_N65", N=65, M=64, P=4, Q=3, Df=1, exact=False, ell=(0.9, 0.6, 0.7), shift=0.0, seed=104),
    dict(name="M65_N257", N=257, M=65, P=1, Q=3, Df=4, exact=True, ell=(0.05, 0.1, 0.2), shift=0.0, seed=105),
    dict(name="M127_N65", N=65, M=127, P=2, Q=1, Df=1, exact=False, ell=(0.15,), shift=0.0, seed=106),
    dict(name="M128_N257", N=257, M=128, P=4, Q=3, Df=4, exact=True, ell=(0.6, 0.8, 0.5), shift=0.0, seed=107),
    dict(name="M129_N64", N=64, M=129, P=3, Q=3, Df=4, exact=False, ell=(0.3, 0.45, 0.6), shift=0.0, seed=108),
    dict(name="M200_N63", N=63, M=200, P=1, Q=1, Df=4, exact=True, ell=(0.05,), shift=0.0, seed=109),
    dict(name="M16_N65_shift", N=65, M=16, P=2, Q=3, Df=4, exact=False, ell=(0.2, 0.3, 0.25), shift=10.0, seed=110),
    dict(name="M66_N65_P3", N=65, M=66, P=3, Q=3, Df=4, exact=True, ell=(0.4, 0.5, 0.6), shift=0.0, seed=112),      # P = 3 on the 16-byte path
    dict(name="M64_N1_shift", N=1, M=64, P=1, Q=3, Df=4, exact=True, ell=(0.1, 0.07, 0.2), shift=10.0, seed=111),
)
CASE_BY_NAME = {c["name"]: c for c in CASES}
REGEN_CASES = ("M1_N1", "M2_N63", "M16_N65_shift", "M63_N64")     # what tests/test_xgrad_cpu.py regenerates (seconds at 50 digits)

# measured 2026-10-21 on the CPU (NumPy), over every stored row of the grid; the raw figure beside each constant
# (the next power of two)
C_ORACLE = {
    "dm": 0.5,         # raw 0.332 (M2_N63); every case with M >= 63 stays below 0.14
    "dv": 0.125,       # raw 0.092 (M2_N63); every case with M >= 63 stays below 0.01
}
# the float64 solve-based chain (chain(strict=True)) against the 50-digit chain at M = 16, scale S x cond_est (joint_ref's s_N63, s_N65,
# s_N129; cond_est 40.2, 4.4, 2.0) -- the larger of it and the explicit-C chain beside it, which measures dm 0.438, dv 0.027
C_ORACLE_STRICT = {
    "dm": 0.5,         # raw 0.438 (s_N129)
    "dv": 0.03125,     # raw 0.027 (s_N129, explicit C; solve-based 0.013)
}


def c_oracle(what, strict=False):
    return float((C_ORACLE_STRICT if strict else C_ORACLE)[what])


def c_kernel(what, strict=False):
    return max(16.0, 4.0 * c_oracle(what, strict))


def c_sum(what):
    """Bound between a device result and this file's float64 value: each within its own constant of R."""
    return c_kernel(what) + c_oracle(what)


# ------------------------------------------------------------------------------------------------------------ designed inputs
def far_row(Z, ell, P, Q):
    """A row at least FAR lengthscales (of every latent) from every inducing input: beyond the largest coordinate 0."""
    x = np.array(Z[0, :P], dtype=float)
    x[0] = max(Z[:, q * P].max() for q in range(Q)) + (FAR + 1.0) * max(ell)
    return x


def make_inputs(case):
    """dict(X, Z, variance, lengthscale, a, C, W) of a designed case, from its seed alone.  a and C are seeded, C symmetric and indefinite;
    W is dense with one entry exactly 0; three rows sit exactly on inducing inputs (of different latents where there are several) and one
    row is far from every inducing input (where N allows: the first row is always an ordinary one)."""
    N, M, P, Q, Df = case["N"], case["M"], case["P"], case["Q"], case["Df"]
    rng = np.random.RandomState(case["seed"])
    Z = rng.rand(M, Q * P) + case["shift"]
    X = rng.rand(N, P) + case["shift"]
    ell = np.array(case["ell"], dtype=float)
    var = rng.uniform(0.4, 1.5, Q)
    a = rng.randn(Q, M)
    B = rng.randn(Q, M, M) / np.sqrt(M)
    C = 0.5 * (B + np.transpose(B, (0, 2, 1)))
    W = np.where(rng.rand(Q, Df) < 0.5, 1.0, -1.0) * rng.uniform(0.3, 1.2, (Q, Df))
    if Q * Df > 1:
        W[Q - 1, 0] = 0.0
    on, far = special_rows(case)
    for t, i in enumerate(on):
        q, m = t % Q, (7 * t + 3) % M
        X[i] = Z[m, q * P:(q + 1) * P]
    if far is not None:
        X[far] = far_row(Z, ell, P, Q)
    return dict(X=X, Z=Z, variance=var, lengthscale=ell, a=a, C=C, W=W)


def special_rows(case):
    """(rows exactly on inducing inputs, the far row or None)."""
    N = case["N"]
    if N < 8:
        return [], None
    return [2, N // 2, N - 3], 5


def stored_rows(case):
    """The rows of a case the grid holds at 50 digits: first and last, around 63 / 64 / 65, the special rows, then seeded others."""
    N = case["N"]
    on, far = special_rows(case)
    want = [0, N - 1] + [i for i in (62, 63, 64, 65) if i < N] + on + ([far] if far is not None else [])
    rows = []
    for i in want:
        if i not in rows:
            rows.append(i)
    rng = np.random.RandomState(9000 + case["seed"])
    for i in rng.permutation(N):
        if len(rows) >= min(MAX_ROWS, N):
            break
        if int(i) not in rows:
            rows.append(int(i))
    return np.array(sorted(rows), dtype=np.int64)


# ------------------------------------------------------------------------------------------------------------ the restatement
def latent_terms(inp, q, X):
    P = X.shape[1]
    Zq = inp["Z"][:, q * P:(q + 1) * P]
    var, ell = float(inp["variance"][q]), float(inp["lengthscale"][q])
    k = var * np.exp(-0.5 * jr.r2_gpy(X, Zq, ell))
    D = Zq[None, :, :] - X[:, None, :]                    # (n, M, P): one subtraction per term
    return Zq, var, ell, k, D


def grads_from(inp, X, a, T_of, return_scale=False):
    """dm, dv (n, Df, P) with t_q = T_of(q, k_q); with return_scale also (S_dm, S_dv, F_dm, F_dv)."""
    X = np.asarray(X, float)
    n, P = X.shape
    W = inp["W"]
    Q, Df = W.shape
    dm, dv = np.zeros((n, Df, P)), np.zeros((n, Df, P))
    sm, sv, fm, fv = (np.zeros((n, Df, P)) for _ in range(4))
    for q in range(Q):
        Zq, var, ell, k, D = latent_terms(inp, q, X)
        il2 = 1.0 / (ell * ell)
        T = T_of(q, k)
        gp = il2 * np.einsum("m,im,imj->ij", a[q], k, D)
        gc = (2.0 * il2) * np.einsum("im,im,imj->ij", T, k, D)
        w = W[q]
        dm += w[None, :, None] * gp[:, None, :]
        dv += (w * w)[None, :, None] * gc[:, None, :]
        if return_scale:
            aX, aZ, aD = np.abs(X), np.abs(Zq), np.abs(D)
            r2 = np.sum(D * D, -1)
            e = 1.0 + ((aX * aX).sum(-1)[:, None] + (aZ * aZ).sum(-1)[None, :] + 2.0 * aX @ aZ.T) * (0.5 * il2) + r2 * (0.5 * il2)
            ke = var * np.exp(-0.5 * r2 * il2) * e
            aC = np.abs(inp["C"][q])
            sgp = il2 * np.einsum("m,im,imj->ij", np.abs(a[q]), ke, aD)
            sgc = (2.0 * il2) * np.einsum("im,im,imj->ij", ke @ aC, ke, aD)
            fgp = il2 * np.einsum("m,imj->ij", np.abs(a[q]), aD)
            fgc = (2.0 * il2) * var * np.einsum("m,imj->ij", aC.sum(0), aD)
            aw = np.abs(w)
            sm += aw[None, :, None] * sgp[:, None, :]
            sv += (w * w)[None, :, None] * sgc[:, None, :]
            fm += aw[None, :, None] * fgp[:, None, :]
            fv += (w * w)[None, :, None] * fgc[:, None, :]
    if return_scale:
        return dm, dv, sm, sv, fm, fv
    return dm, dv


def input_grad(inp, X=None, return_scale=False):
    """The building block in float64: (dm, dv) (n, Df, P) at the rows X (default: the case's own)."""
    X = inp["X"] if X is None else X
    return grads_from(inp, X, inp["a"], lambda q, k: k @ inp["C"][q], return_scale)


def mean_var_terms(inp, X):
    """m (n, Df) and the x-dependent part of v (n, Df) of the same coefficients: sum_q W_qd p_q and sum_q W_qd^2 c_q."""
    X = np.asarray(X, float)
    W = inp["W"]
    m, v = np.zeros((X.shape[0], W.shape[1])), np.zeros((X.shape[0], W.shape[1]))
    for q in range(W.shape[0]):
        _, _, _, k, _ = latent_terms(inp, q, X)
        m += (k @ inp["a"][q])[:, None] * W[q][None, :]
        v += np.einsum("im,mk,ik->i", k, inp["C"][q], k)[:, None] * (W[q] * W[q])[None, :]
    return m, v


def sensitivity(dm):
    """Root mean square over the rows: (Df, P)."""
    return np.sqrt(np.mean(dm * dm, axis=0))


# ------------------------------------------------------------------------------------------------------------ the engine's chain
def chain_inputs(prm, Xnew):
    """The building block's inputs from the raw parameters (Z, m_u, L_flat, hypers; joint_ref.make_params): a = K^-1 m, C = K^-1 S K^-1 - K^-1."""
    Q = prm["variance"].shape[0]
    lts = [jr.latent(prm, q, np.asarray(Xnew, float)) for q in range(Q)]
    return dict(X=np.asarray(Xnew, float), Z=prm["Z"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                a=np.stack([lt["alpha"] for lt in lts]), C=np.stack([lt["C"] for lt in lts]), W=prm["W"]), lts


def chain(prm, Xnew, strict=False, return_scale=False):
    """(dm, dv) of the whole chain in float64.  strict=True: T = ((A K^-1) L_q L_q^T - A) K^-1 through solves against the Cholesky factor of
    K_uu, as the strict mode forms it; the mean's coefficients are K^-1 m in both."""
    from scipy.linalg import cho_solve
    inp, lts = chain_inputs(prm, Xnew)

    def T_of(q, k):
        if not strict:
            return k @ inp["C"][q]
        lt = lts[q]
        R = cho_solve((lt["Lk"], True), k.T).T
        U = (R @ lt["Lq"]) @ lt["Lq"].T - k
        return cho_solve((lt["Lk"], True), U.T).T
    return grads_from(inp, inp["X"], inp["a"], T_of, return_scale)


# ------------------------------------------------------------------------------------------------------------ the designed sensitivity case
def sensitivity_case():
    """2-D inputs; q(u)'s mean is a function of column 0 of the inducing inputs only (sin 2 pi z_0), small S: (prm, X).  One latent, the
    four functions of joint_ref.SPECS; 6 x 6 inducing grid."""
    case = dict(M=36, Q=1, P=2, N=50, seed=77)
    prm, X = jr.make_params(case)
    Z = prm["Z"]
    prm["m_u"] = np.sin(2.0 * np.pi * Z[:, :1])
    M = Z.shape[0]
    prm["L_flat"] = (0.05 * np.eye(M))[np.tril_indices(M)][:, None]
    prm["lengthscale"] = np.array([0.2])                  # the grid's spacing: the interpolant of sin(2 pi z_0) has no ripple along column 1
    prm["variance"] = np.array([1.0])
    return prm, X


# ------------------------------------------------------------------------------------------------------------ the grid
def load_grid(path=GRID):
    g = np.load(path)
    out = {}
    for c in CASES:
        k = c["name"] + "/"
        out[c["name"]] = dict(case=c, rows=g[k + "rows"], **{key: g[k + key] for key in ("dm", "dv", "S_dm", "S_dv", "F_dm", "F_dv")})
    return out


def ratios(got, R, S, F):
    """|got - R| / (2^-52 S + 2^-1022 F) per entry (0 where both are equal, inf where a value is not finite)."""
    got, R = np.asarray(got, float), np.asarray(R, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(got - R) / (EPS * np.asarray(S, float) + TINY * np.asarray(F, float))
    r = np.where(got == R, 0.0, r)
    return np.where(np.isfinite(got), r, np.inf)


def case_ratios(entry, dm, dv):
    """(worst dm ratio, worst dv ratio) of a full result (N, Df, P) against a loaded grid case (its stored rows)."""
    rows = entry["rows"]
    rm = ratios(np.asarray(dm)[rows], entry["dm"], entry["S_dm"], entry["F_dm"])
    rv = ratios(np.asarray(dv)[rows], entry["dv"], entry["S_dv"], entry["F_dv"])
    return float(np.max(rm)), float(np.max(rv))
