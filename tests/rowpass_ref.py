"""Extended-precision restatement of the row pass: the forward P~ = K^ C, the row statistics, the weighted Gram
H = K^T diag(beta) K^, the column statistics and the inner-protocol gradients, element by element, with one condition scale per
element.  Needs NumPy and mpmath only: it imports neither the oracle nor the package.

  R  every quantity in np.longdouble (64-bit significand).  The float64 inputs (Z, m_u, L_flat, the hyper-parameters, X, Y) are taken
     as exact numbers.  The M x M side is a hand-written Cholesky and triangular inverse (vectorised by column / row), the row weights
     gm, gv come from the 50-digit rules of tests/lik_ref_mp.py evaluated at the longdouble m, v.
  S  one condition scale per element of R: the sum of the absolute values of the addends of the element's own reduction; wherever a
     factor is itself a computed sum (beta_n, alpha_n, P~_nm, p, c, a, C) that factor's scale stands in for its absolute value -- a
     running error bound, as DESIGN 9a defines S for the likelihood rows.  Never an array maximum.  Scales are float64 (BLAS): a scale
     needs no more.

Criterion, in the form of tests/likgrid.py:   |got - R| <= C[kind] * 2^-52 * max(S, 2^-1022)   for every element,
kinds ve, sgv, H, r, dZ, sa, sl, swk, dKmn, dKdiag, m, v.  `check` prints the worst ratio per kind before it asserts.

Constants.  C_ORACLE[kind] = the largest |oracle - R| / (2^-52 S) of the float64 NumPy oracle (`so.u_algebra` + `so.local_stats`, BLAS /
LAPACK) over cases A-E with case D's batch-scale, row-shard and strict variants, rounded up to the next power of two: what plain float64 achieves on these
formulas (tests/test_rowpass_ref_cpu.py measures it and asserts it).  The kernels get C_KERNEL = max(16, 4 * C_ORACLE): another
summation order, MFMA accumulation, special functions with 1-2 ulp.  Against the float64 oracle instead of R the two constants add.
Cases G, H, I (3-D / 4-D inputs, eight latents) have C_ORACLE_WIDE / C_KERNEL_WIDE: the same rule over their own oracle measurement,
never below C_ORACLE; cases A-F stay on C_ORACLE / C_KERNEL."""
import numpy as np

import lik_ref_mp as lr

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "rowpass_ref needs an extended-precision np.longdouble (eps <= 2^-63); this platform has %r" % (
    np.finfo(LD).eps,)

EPS = 2.0 ** -52
TINY = 2.0 ** -1022
KINDS = ("ve", "sgv", "H", "r", "dZ", "sa", "sl", "swk", "dKmn", "dKdiag", "m", "v")
BUNDLE_KINDS = ("ve", "sgv", "H", "r", "dZ", "sa", "sl", "swk")

# Largest ratio of the float64 oracle over cases A-E and D's variants, rounded up to a power of two (measured 2026-10-17 on the CPU; the raw
# figures per case are in DESIGN 9c).
C_ORACLE = dict(ve=16.0, sgv=8.0, H=256.0, r=64.0, dZ=4.0, sa=1.0, sl=1.0, swk=1.0, dKmn=512.0, dKdiag=256.0, m=16.0, v=1.0)
# Elements beyond C_KERNEL that are inherent to the formulation: {(case tag, kind): [index tuples]} -- at most 1 % of an array, none in
# a tile of the 100 h latent, each justified in DESIGN 9c.  None is needed.
KERNEL_EXCEPTIONS = {}
# Cases G, H, I (3-D / 4-D inputs, eight latents) and their variants: per kind max(C_ORACLE, the float64 oracle's largest ratio over
# them rounded up to a power of two), by the same rule and against R (measured 2026-10-19 on the CPU).  Two kinds move, both
# sums of quadrature rows in NumPy's pairwise order: ve (24.7 on G) and sgv (24.2 on I).  Cases A-F stay on C_ORACLE.
C_ORACLE_WIDE = dict(C_ORACLE, ve=32.0, sgv=32.0)
# The `strict2` variants (the two-solve form of the strict q(f) mode) and case J need no constants of their own: the
# float64 oracle's two-solve restatement stays within C_ORACLE on B, D, J and within C_ORACLE_WIDE on G, H in every kind (measured
# 2026-10-21 on the CPU, table in DESIGN 9x; tests/test_rowpass_ref_cpu.py asserts it).  Nothing is widened.


def c_kernel():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE.items()}


def c_kernel_wide():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE_WIDE.items()}


def c_kernel_vs_float64():
    return {k: max(16.0, 4.0 * c) + c for k, c in C_ORACLE.items()}


# ================================================================================================ M x M side
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def cholesky_ld(A):
    """Lower Cholesky factor, one column at a time."""
    M = A.shape[0]
    L = np.zeros((M, M), dtype=LD)
    for j in range(M):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def tri_inverse_ld(L):
    """Inverse of a lower-triangular matrix by forward substitution, one row at a time (all columns at once)."""
    M = L.shape[0]
    X = np.zeros((M, M), dtype=LD)
    for i in range(M):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = LD(1) / L[i, i]
    return X


def flat_to_tril(flat_col, M):
    L = np.zeros((M, M), dtype=LD)
    L[np.tril_indices(M)] = _ld(flat_col)
    return L


def sqdist_ld(X, Z):
    """sum_p (x_p - z_p)^2, [N, M]."""
    X, Z = _ld(X), _ld(Z)
    d = X[:, None, :] - Z[None, :, :]
    return np.sum(d * d, axis=2)


def u_side(prm, prob, forced_rungs):
    """Per latent: Kuu (without jitter), jitter, Luu, Li = Luu^-1, Kuui, L, S, a, C in longdouble; scales s_a, s_C (and, for the
    strict form, Li_abs) in float64.  The jitter is the float64 number GPy forms: fl(fl(mean(diag) * 1e-6) * 10^rung), mean(diag) =
    variance; rung -1 = none."""
    Q, M, P = prob["Q"], prob["M"], prob["P"]
    out = []
    for q in range(Q):
        Zq = prm["Z"][:, q * P:(q + 1) * P]
        var, ell = LD(float(prm["variance"][q])), LD(float(prm["lengthscale"][q]))
        Kuu = var * np.exp(-sqdist_ld(Zq, Zq) / (ell * ell) / 2)
        rung = -1 if forced_rungs is None else int(forced_rungs[q])
        jit = 0.0 if rung < 0 else float(np.float64(prm["variance"][q]) * np.float64(1e-6) * np.float64(10.0 ** rung))
        Luu = cholesky_ld(Kuu + np.eye(M, dtype=LD) * LD(jit))
        Li = tri_inverse_ld(Luu)
        Kuui = Li.T @ Li
        L = flat_to_tril(prm["L_flat"][:, q], M)
        S = L @ L.T
        m = _ld(prm["m_u"][:, q])
        a = Kuui @ m
        B = Kuui @ L
        C = B @ B.T - Kuui
        Ka, La = np.abs(Kuui).astype(np.float64), np.abs(L).astype(np.float64)
        Ba = Ka @ La
        out.append(dict(Kuu=Kuu, jitter=jit, Luu=Luu, Li=Li, Kuui=Kuui, L=L, S=S, a=a, C=C,
                        s_a=Ka @ np.abs(prm["m_u"][:, q]), s_C=Ba @ Ba.T + Ka, Li_abs=np.abs(Li).astype(np.float64)))
    return out


# ================================================================================================ likelihood rows
def _to_mpf(x):
    hi = float(x)
    return lr.mpf(hi) + lr.mpf(float(x - LD(hi)))


def _from_mpf(z):
    hi = float(z)
    return LD(hi) + LD(float(z - lr.mpf(hi)))


def lik_rows(name, kw, y, m, v):
    """The rules of lik_ref_mp at longdouble m, v [N, J]: (ve [N], gm [N, J], gv [N, J]) in longdouble and their scales in float64."""
    N, J = m.shape
    fam = lr.FAMILIES[name]
    kw = {k: a for k, a in kw.items() if a is not None}
    R = np.zeros((N, 1 + 2 * J), dtype=LD)
    S = np.zeros((N, 1 + 2 * J))
    for n in range(N):
        acc = fam(float(y[n]), [_to_mpf(a) for a in m[n]], [_to_mpf(a) for a in v[n]], **kw)
        R[n] = [_from_mpf(a.r) for a in acc]
        S[n] = [float(a.s) for a in acc]
    return (R[:, 0], R[:, 1:1 + J], R[:, 1 + J:]), (S[:, 0], S[:, 1:1 + J], S[:, 1 + J:])


# ================================================================================================ per row
def task_functions(prob, t):
    return [d for d in range(prob["Df"]) if prob["f_index"][d] == t]


def row_side(prm, prob, side, X, Y):
    """Per task t (all its rows): per latent K^, gate (r2 != 0, quirk Q10), P~, p, c, p~, c~ and the strict form's X = K^ Luu^-T; m_fd,
    v_fd, and the UNSCALED row weights ve, gm, gv.  Every array comes with its scale (key "s_" + name)."""
    Q, M, P, T = prob["Q"], prob["M"], prob["P"], prob["T"]
    W, kap = np.asarray(prm["W"], float), np.asarray(prm["kappa"], float)
    rows = []
    for t in range(T):
        ds = task_functions(prob, t)
        Xt = np.asarray(X[t], float).reshape(-1, P)
        N = Xt.shape[0]
        o = dict(N=N, ds=ds, lat=[])
        for q in range(Q):
            u = side[q]
            Zq = prm["Z"][:, q * P:(q + 1) * P]
            var, ell = LD(float(prm["variance"][q])), LD(float(prm["lengthscale"][q]))
            d2 = sqdist_ld(Xt, Zq)
            r2 = d2 / (ell * ell)
            K = var * np.exp(-r2 / 2)
            Pt = K @ u["C"]
            Kf, r2f = K.astype(np.float64), r2.astype(np.float64)
            sP = Kf @ u["s_C"]
            lat = dict(K=K, r2=r2, gate=d2 != 0, Pt=Pt, s_Pt=sP, p=K @ u["a"], s_p=Kf @ u["s_a"], c=np.sum(Pt * K, 1),
                       s_c=np.sum(sP * Kf, 1), pt=(K * r2) @ u["a"], s_pt=(Kf * r2f) @ u["s_a"], ct=np.sum(Pt * K * r2, 1),
                       s_ct=np.sum(sP * Kf * r2f, 1))
            o["lat"].append(lat)
        J = len(ds)
        m, v = np.zeros((N, J), dtype=LD), np.zeros((N, J), dtype=LD)
        sm, sv = np.zeros((N, J)), np.zeros((N, J))
        for j, d in enumerate(ds):
            for q in range(Q):
                w, lat = LD(W[q, d]), o["lat"][q]
                bdd = (w * w + LD(kap[q, d])) * LD(float(prm["variance"][q]))
                m[:, j] += w * lat["p"]
                v[:, j] += bdd + w * w * lat["c"]
                sm[:, j] += abs(W[q, d]) * lat["s_p"]
                sv[:, j] += abs(float(bdd)) + W[q, d] ** 2 * lat["s_c"]
        o.update(m=m, v=v, s_m=sm, s_v=sv)
        name, kw = prob["specs"][t]
        if N:
            (o["ve"], o["gm"], o["gv"]), (o["s_ve"], o["s_gm"], o["s_gv"]) = lik_rows(name, kw, np.asarray(Y[t], float).reshape(-1), m, v)
        else:
            o.update(ve=np.zeros(0, LD), gm=np.zeros((0, J), LD), gv=np.zeros((0, J), LD), s_ve=np.zeros(0), s_gm=np.zeros((0, J)),
                     s_gv=np.zeros((0, J)))
        rows.append(o)
    return rows


def strict_rows(side, rows, form=True):
    """One-solve form: X = K^ Luu^-T (forward substitution: Li is Luu^-1 by forward substitution) and its scale, added to every (task,
    latent).  form="two": A = K^ Kuu^-1 (both halves of the solve) and its scale s_A = |K^| |Kuu^-1|, from the cached K^ and Kuu^-1."""
    for o in rows:
        for q, lat in enumerate(o["lat"]):
            if form == "two":
                if "As" not in lat:
                    lat["As"] = np.ascontiguousarray(lat["K"]) @ np.ascontiguousarray(side[q]["Kuui"].T).T
                    lat["s_As"] = lat["K"].astype(np.float64) @ np.abs(side[q]["Kuui"]).astype(np.float64)
            elif "Xs" not in lat:
                lat["Xs"] = lat["K"] @ side[q]["Li"].T
                lat["s_Xs"] = lat["K"].astype(np.float64) @ side[q]["Li_abs"].T


# ================================================================================================ reductions
def reduce_rows(prm, prob, side, rows, X, batch_scale=None, row_begin=None, row_end=None, strict=False, raw=True):
    """The statistic bundle of the rows [row_begin[t], row_end[t]) of every task, the inner-protocol gradients and q(f) of those
    rows.  Returns (R, S): dicts kind -> array,
      ve (1,)  nneg (1,)  sgv (Df,)  H (Q, M, M)  r (Q, M)  dZ (Q, M, P)  sa (Q,)  sl (Q,)  swk (Q, Df)
      dKmn [q][d] (M, n_t)  dKdiag [q][d] (n_t,)  m [d] (n_t,)  v [d] (n_t,)
    strict=True: H and r hold X^T diag(beta) X and X^T alpha (X = K^ Luu^-T), the rest is the same mathematics.
    strict="two": the two-solve form, H = A^T diag(beta) A and r = A^T alpha (A = K^ Kuu^-1, scale s_A = |K^| |Kuu^-1|): dVE_dS and
    dVE_dmu themselves; the rest is the same mathematics."""
    assert strict in (False, True, "two"), strict
    Q, M, P, T, Df = prob["Q"], prob["M"], prob["P"], prob["T"], prob["Df"]
    W = np.asarray(prm["W"], float)
    W0 = np.asarray(prm.get("W0", prm["W"]), float)
    bs = [1.0] * T if batch_scale is None else [float(b) for b in batch_scale]
    b0 = [0] * T if row_begin is None else [int(b) for b in row_begin]
    e0 = [rows[t]["N"] for t in range(T)] if row_end is None else [int(e) for e in row_end]
    R = dict(ve=np.zeros(1, LD), nneg=np.zeros(1, LD), sgv=np.zeros(Df, LD), H=np.zeros((Q, M, M), LD), r=np.zeros((Q, M), LD),
             dZ=np.zeros((Q, M, P), LD), sa=np.zeros(Q, LD), sl=np.zeros(Q, LD), swk=np.zeros((Q, Df), LD),
             dKmn=[[None] * Df for _ in range(Q)], dKdiag=[[None] * Df for _ in range(Q)], m=[None] * Df, v=[None] * Df)
    S = dict(ve=np.zeros(1), nneg=np.zeros(1), sgv=np.zeros(Df), H=np.zeros((Q, M, M)), r=np.zeros((Q, M)), dZ=np.zeros((Q, M, P)),
             sa=np.zeros(Q), sl=np.zeros(Q), swk=np.zeros((Q, Df)), dKmn=[[None] * Df for _ in range(Q)],
             dKdiag=[[None] * Df for _ in range(Q)], m=[None] * Df, v=[None] * Df)
    if strict:
        strict_rows(side, rows, strict)
    gkey = "As" if strict == "two" else "Xs"
    for t in range(T):
        o, sl_ = rows[t], slice(b0[t], e0[t])
        ds = o["ds"]
        sc = LD(bs[t])
        ve, gm, gv = o["ve"][sl_] * sc, o["gm"][sl_] * sc, o["gv"][sl_] * sc
        sve, sgm, sgv = o["s_ve"][sl_] * abs(bs[t]), o["s_gm"][sl_] * abs(bs[t]), o["s_gv"][sl_] * abs(bs[t])
        R["ve"][0] += ve.sum()
        S["ve"][0] += sve.sum()
        R["nneg"][0] += int((o["v"][sl_] < 0).sum())
        Xt = _ld(np.asarray(X[t], float).reshape(-1, P)[sl_])
        for j, d in enumerate(ds):
            R["sgv"][d] += gv[:, j].sum()
            S["sgv"][d] += sgv[:, j].sum()
            R["m"][d], S["m"][d] = o["m"][sl_, j], o["s_m"][sl_, j]
            R["v"][d], S["v"][d] = o["v"][sl_, j], o["s_v"][sl_, j]
        for q in range(Q):
            u, lat = side[q], o["lat"][q]
            w, w0 = W[q, ds], W0[q, ds]
            alpha, beta = gm @ _ld(w), gv @ _ld(w * w)
            alpha0, beta0 = gm @ _ld(w0), gv @ (_ld(w0) * _ld(w))
            s_alpha, s_beta = sgm @ np.abs(w), sgv @ (w * w)
            s_alpha0, s_beta0 = sgm @ np.abs(w0), sgv @ np.abs(w0 * w)
            K, Pt = lat["K"][sl_], lat["Pt"][sl_]
            Kf, sP = K.astype(np.float64), lat["s_Pt"][sl_]
            Kg, sKg = (lat[gkey][sl_], lat["s_" + gkey][sl_]) if strict else (K, Kf)
            if K.shape[0]:
                R["H"][q] += np.ascontiguousarray((Kg * beta[:, None]).T) @ Kg
                S["H"][q] += (sKg * s_beta[:, None]).T @ sKg
                R["r"][q] += Kg.T @ alpha
                S["r"][q] += sKg.T @ s_alpha
            E = (alpha0[:, None] * u["a"][None, :] + 2 * beta0[:, None] * Pt) * K * lat["gate"][sl_]
            sE = (s_alpha0[:, None] * u["s_a"][None, :] + 2.0 * s_beta0[:, None] * sP) * Kf * lat["gate"][sl_]
            Zq = _ld(prm["Z"][:, q * P:(q + 1) * P])
            for pp in range(P):
                diff = Xt[:, pp][:, None] - Zq[:, pp][None, :]
                R["dZ"][q, :, pp] += np.sum(E * diff, 0)
                S["dZ"][q, :, pp] += np.sum(sE * np.abs(diff).astype(np.float64), 0)
            p, c, pt, ct = lat["p"][sl_], lat["c"][sl_], lat["pt"][sl_], lat["ct"][sl_]
            sp, s_c, spt, sct = lat["s_p"][sl_], lat["s_c"][sl_], lat["s_pt"][sl_], lat["s_ct"][sl_]
            R["sa"][q] += alpha0 @ p + 2 * (beta0 @ c)
            S["sa"][q] += s_alpha0 @ sp + 2.0 * (s_beta0 @ s_c)
            R["sl"][q] += alpha0 @ pt + 2 * (beta0 @ ct)
            S["sl"][q] += s_alpha0 @ spt + 2.0 * (s_beta0 @ sct)
            for j, d in enumerate(ds):
                R["swk"][q, d] += gm[:, j] @ p + 2 * LD(W[q, d]) * (gv[:, j] @ c)
                S["swk"][q, d] += sgm[:, j] @ sp + 2.0 * abs(W[q, d]) * (sgv[:, j] @ s_c)
                if raw:      # dL_dKmn[q][d][m, n] = a_m gm_nj + 2 w_qd gv_nj P~_nm (svmogp_inf.py:157-161 with C symmetric)
                    R["dKmn"][q][d] = u["a"][:, None] * gm[:, j][None, :] + 2 * LD(W[q, d]) * gv[:, j][None, :] * Pt.T
                    S["dKmn"][q][d] = u["s_a"][:, None] * sgm[:, j][None, :] + 2.0 * abs(W[q, d]) * sgv[:, j][None, :] * sP.T
                    R["dKdiag"][q][d], S["dKdiag"][q][d] = gv[:, j], sgv[:, j]
    return R, S


def reference(prm, prob, X, Y, forced_rungs, batch_scale=None, row_begin=None, row_end=None, strict=False, cache=None):
    """(R, S) of one evaluation.  `cache` (a dict) keeps the M x M side and the per-row quantities between calls that share the
    parameters and the data and differ in batch_scale / the row ranges / the strict form."""
    cache = {} if cache is None else cache
    if "side" not in cache:
        cache["side"] = u_side(prm, prob, forced_rungs)
        cache["rows"] = row_side(prm, prob, cache["side"], X, Y)
    return reduce_rows(prm, prob, cache["side"], cache["rows"], X, batch_scale, row_begin, row_end, strict)


# ================================================================================================ bundle layout
def layout(prob):
    """Offsets (float64 words) of the statistic bundle: the engine's layout, restated."""
    Q, M, P, Df = prob["Q"], prob["M"], prob["P"], prob["Df"]
    per_q = M * M + M + M * P + 2 + Df
    return dict(NG=2 + Df, per_q=per_q, size=2 + Df + Q * per_q, H=0, r=M * M, dZ=M * M + M, sa=M * M + M + M * P,
                sl=M * M + M + M * P + 1, swk=M * M + M + M * P + 2, sgv=2)


def split_bundle(stats, prob):
    """Flat bundle -> dict kind -> array in the shapes of `reduce_rows`."""
    Q, M, P, Df = prob["Q"], prob["M"], prob["P"], prob["Df"]
    lay = layout(prob)
    stats = np.asarray(stats)
    assert stats.shape == (lay["size"],), (stats.shape, lay["size"])
    out = dict(ve=stats[0:1], nneg=stats[1:2], sgv=stats[2:2 + Df])
    per = [stats[lay["NG"] + q * lay["per_q"]:lay["NG"] + (q + 1) * lay["per_q"]] for q in range(Q)]
    out["H"] = np.stack([b[:M * M].reshape(M, M) for b in per])
    out["r"] = np.stack([b[lay["r"]:lay["r"] + M] for b in per])
    out["dZ"] = np.stack([b[lay["dZ"]:lay["dZ"] + M * P].reshape(M, P) for b in per])
    out["sa"] = np.array([b[lay["sa"]] for b in per])
    out["sl"] = np.array([b[lay["sl"]] for b in per])
    out["swk"] = np.stack([b[lay["swk"]:lay["swk"] + Df] for b in per])
    return out


def pack_bundle(R, prob):
    """The whole bundle in layout order (H as the full symmetric matrix), dtype of R."""
    Q = prob["Q"]
    parts = [R["ve"], R["nneg"], R["sgv"]]
    for q in range(Q):
        parts += [R["H"][q].reshape(-1), R["r"][q], R["dZ"][q].reshape(-1), R["sa"][q:q + 1], R["sl"][q:q + 1], R["swk"][q]]
    return np.concatenate([np.asarray(p).reshape(-1) for p in parts])


# ================================================================================================ criterion
def ratios(got, R, S):
    """|got - R| / (2^-52 max(S, 2^-1022)) per element, float64; 0 where got == R exactly, inf where got is not finite."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        d = np.abs(got.astype(LD) - np.asarray(R, dtype=LD))
        r = np.where(d == 0, LD(0), d / (LD(EPS) * np.maximum(np.asarray(S, dtype=LD), LD(TINY)))).astype(np.float64)
    return np.where(np.isfinite(got), r, np.inf)


def pairs(kind, got, R, S):
    """[(label, got, R, S)] of one kind; H is compared on its lower triangle."""
    if kind == "H":
        lo = np.tril(np.ones(R.shape[1:], dtype=bool))
        return [("q%d" % q, np.asarray(got[q])[lo], R[q][lo], S[q][lo]) for q in range(R.shape[0])]
    if kind in ("dKmn", "dKdiag"):
        return [("q%d d%d" % (q, d), got[q][d], R[q][d], S[q][d]) for q in range(len(R)) for d in range(len(R[q]))]
    if kind in ("m", "v"):
        return [("d%d" % d, got[d], R[d], S[d]) for d in range(len(R))]
    return [("", got, R, S)]


def worst_ratios(got, R, S, kinds):
    """{kind: (worst ratio, label, flat index)} over the given kinds of `got` (a dict kind -> array(s) shaped like R)."""
    out = {}
    for k in kinds:
        best = (0.0, "", -1)
        for label, g, r, s in pairs(k, got[k], R[k], S[k]):
            g = np.asarray(g)
            assert g.shape == np.shape(r), (k, label, g.shape, np.shape(r))
            if g.size == 0:
                continue
            x = ratios(g, r, s).reshape(-1)
            i = int(np.argmax(x))
            if x[i] > best[0]:
                best = (float(x[i]), label, i)
        out[k] = best
    return out


def check(case, got, R, S, C, kinds):
    """Every element of every given kind within C[kind] * 2^-52 * S; the count of rows with v < 0 equal.  Prints the worst ratio per
    kind as `[rowpass] <case> <kind> ...` before asserting; returns {kind: worst ratio}."""
    w = worst_ratios(got, R, S, kinds)
    for k in kinds:
        print("[rowpass] %-28s %-6s worst |got - R| / (2^-52 S) = %-10.4g (C = %g) at %s[%d]" % (case, k, w[k][0], C[k], w[k][1], w[k][2]))
    bad = {k: w[k] for k in kinds if not w[k][0] <= C[k]}
    assert not bad, (case, "beyond C", {k: (v, C[k]) for k, v in bad.items()})
    if "nneg" in got:
        assert float(np.asarray(got["nneg"]).reshape(-1)[0]) == float(R["nneg"][0]), (case, "count of v < 0")
    return {k: w[k][0] for k in kinds}
