"""Extended-precision restatement of the gradient tail: everything between the statistic bundle and the numbers the
optimiser consumes -- `hmogp_engine::finish_enqueue` / `finish_tail` with the u-side chain of `step_begin` feeding it, the algebra of
`so.finish` (quirks Q4, Q5, Q10 included).  Needs NumPy (and tests/rowpass_ref.py, whose longdouble conventions, `u_side`,
`tri_inverse_ld` and bundle layout are used as they are); imports neither the oracle nor the package.

  input   a float64 statistic bundle TAKEN AS EXACT (layout: `rr.layout` / `rr.split_bundle` / `rr.pack_bundle`; H_q is read from its
          lower triangle, as the engine reads it) and `rr.u_side(prm, prob, rungs)`; S^-1 = Linv^T Linv, Linv = `tri_inverse_ld(L)`.
  R       per latent, in np.longdouble:  G = K^-1 H K^-1, Kr = K^-1 r  (strict one-solve form: H = X^T beta X, r = X^T alpha in the
          bundle, G = Luu^-T H Luu^-1, Kr = Luu^-T r;  strict two-solve form, strict="two": H = A^T beta A, r = A^T alpha, G = H, Kr = r);  dL_dS = G - (K^-1 - S^-1)/2;  g_L_u = 2 tril(dL_dS L), packed as
          `pack_gl_kernel` packs it;  g_m_u = Kr - a;  GSK = G S K^-1, KSK = K^-1 S K^-1;  dL_dKmm = sym(G - GSK - GSK^T - Kr a^T)
          - (K^-1 - KSK - a a^T)/2;  the K_zz-weighted row sums of `kzz_rows_kernel` (diagonal r^2 forced to 0, terms with r^2 = 0
          dropped);  the four KL terms, kl[q], elbo;  g_variance, g_lengthscale, g_W, g_kappa, g_Z assembled as `finish_tail` assembles
          them from sa, sl, swk, sgv, dZ and the row sums;  wv = a and winv = K^-1 - KSK of `posterior_u`.
  S       one running error bound per element: the sum of the absolute addends of the element's own reduction, a computed factor's
          scale standing in for its absolute value.  K^-1 and S^-1 get the scale of 9f's `sinv` (s = |Li|^T s_Li + s_Li^T |Li| +
          |Li|^T |Li|, s_Li = |Li| |L| |Li|, Li the triangular inverse), and wherever K^-1 is a factor of a product it counts as
          |K^-1| + s_K^-1:
              S(G) = |K^-1||H||K^-1| + s_K^-1 |H||K^-1| + |K^-1||H| s_K^-1.
          The u-side scales s_a = |K^-1||m| and s_C = |K^-1||L||L|^T|K^-1| + |K^-1| of 9c are reused and completed in the same way
          (9c could leave K^-1's own error to its constants; here a and C are outputs): S(wv) = s_a + s_K^-1 |m|,
          S(winv) = s_C + s_K^-1 + s_K^-1 |L||L|^T |K^-1| + |K^-1| |L||L|^T s_K^-1.
          K_zz = variance exp(-r^2 / 2) counts with its value (as in 9a / 9c the amplification of r^2's own rounding through exp is
          not folded into S).  Example: S(g_Z) sums (s_EK_mj + s_EK_jm) |z_j - z_m| / l^2 plus |dZ| / l^2, s_EK = S(dL_dKmm) K_zz.
          Never an array maximum.  Scales are float64 (BLAS).

Criterion, the form of 9a / 9c / 9f:   |got - R| <= C[kind] * 2^-52 * max(S, 2^-1022)   for every element, kinds KINDS.

Constants.  C_ORACLE[kind] = the largest ratio of the float64 oracle (`so.u_algebra` + `so.finish` on the same float64 bundle) over the
dense cases A-E with D's batch-scale and strict variants and the tail-only shapes with M <= 330, rounded up to the next power of two
(tests/test_tail_ref_cpu.py re-measures and asserts it); C_KERNEL = max(16, 4 * C_ORACLE).  Never fitted to the kernels.

`scales(..., const=False)` is the same map with the bundle's absolute values replaced by given non-negative arrays, the terms that do
not depend on the bundle dropped and plain |K^-1| as the factor: how an error bound of the BUNDLE travels through the tail's linear
maps in absolute value (tests/tail_cases.py, the end-to-end small-model cases)."""
import numpy as np

import rowpass_ref as rr
from rowpass_ref import EPS, LD, TINY, _ld, tri_inverse_ld  # noqa: F401

KINDS = ("kl", "elbo", "g_m_u", "g_L_u", "dL_dS", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z", "wv", "winv")
BUNDLE_KEYS = ("ve", "sgv", "H", "r", "dZ", "sa", "sl", "swk")
KL_BLOCKS = 64           # post.h: kl_terms_kernel's partials (element i of the M x M trace belongs to block (i // 256) % KL_BLOCKS)

# Largest ratio of the float64 oracle over cases A-E, D's variants and the tail-only shapes with M <= 330, rounded up to a power of
# two (measured 2026-10-19 on the CPU; the raw figures per case are in DESIGN 9g).
C_ORACLE = dict(kl=1.0, elbo=1.0, g_m_u=128.0, g_L_u=128.0, dL_dS=128.0, g_variance=1.0, g_lengthscale=1.0, g_W=1.0, g_kappa=1.0,
                g_Z=1.0, wv=32.0, winv=16.0)
# The `strict2` variant of D (the two-solve form: G = H and Kr = r taken as exact), by the same rule and for that variant only:
# per kind max(C_ORACLE, the float64 oracle's largest ratio on it rounded up to a power of two), measured 2026-10-21 on the CPU.  Two
# kinds move, dL_dS (205.2) and g_L_u (191.2): with S(G) = |H| instead of |K^-1||H||K^-1| nothing hides the oracle's own error in
# (K^-1 - S^-1) / 2 against 9f's inverse scale any more.  Every other kind stays within C_ORACLE.
C_ORACLE_TWO = dict(C_ORACLE, g_L_u=256.0, dL_dS=256.0)
# Elements beyond C_KERNEL that are inherent to the formulation: none.
KERNEL_EXCEPTIONS = {}


def c_kernel():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE.items()}


def c_kernel_two():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE_TWO.items()}


def next_pow2(x):
    return 1.0 if x <= 1 else float(2.0 ** np.ceil(np.log2(x)))


def mm(A, B):
    """A @ B in longdouble with both operands walked along contiguous rows (NumPy's longdouble product is a plain loop: 3 x faster)."""
    return np.ascontiguousarray(A) @ np.ascontiguousarray(B.T).T


def f64(a):
    return np.asarray(a).astype(np.float64)


def as_ld(a):
    """To longdouble without passing through float64 (a longdouble bundle keeps its digits)."""
    return np.asarray(a).astype(LD)


def sym_lower(H):
    """The symmetric matrix the engine makes of a bundle's H_q: its lower triangle mirrored."""
    H = np.asarray(H)
    return np.tril(H) + np.tril(H, -1).T


def inv_scale(Li_abs, L_abs):
    """9f's `sinv` scale of Li^T Li from |Li| and |L| (float64): (s_Li, s)."""
    s_Li = Li_abs @ L_abs @ Li_abs
    G = Li_abs.T @ s_Li
    return s_Li, G + G.T + Li_abs.T @ Li_abs


# ================================================================================================ the M^3 part, by row ranges
def heavy_rows(job):
    """Rows [r0, r1) of the products of one latent for every bundle of `job["Hs"]` ([(H, strict)]): Sinv = Linv^T Linv once, and per
    bundle G, GSK = (G S) K^-1, dL_dS, TL = dL_dS L.  Row ranges are independent: a pool splits a large latent."""
    Ki, S, L, Linv, Li, r0, r1 = (job[k] for k in ("Ki", "S", "L", "Linv", "Li", "r0", "r1"))
    Sinv = mm(Linv.T[r0:r1], Linv)
    out = dict(r0=r0, r1=r1, Sinv=Sinv, per=[])
    for H, strict in job["Hs"]:
        if strict == "two":          # the two-solve form: the bundle's H is dVE_dS itself, no M x M solve
            G = np.array(H[r0:r1])
        else:
            left = Li.T[r0:r1] if strict else Ki[r0:r1]
            G = mm(mm(left, H), Li if strict else Ki)
        dLdS = G - (Ki[r0:r1] - Sinv) / 2
        out["per"].append(dict(G=G, GSK=mm(mm(G, S), Ki), dLdS=dLdS, TL=mm(dLdS, L)))
    return out


def heavy_jobs(side_q, Hs, block=256):
    """The row-range jobs of one latent: `Hs` = [(H in longdouble, symmetric; strict)]."""
    M = side_q["L"].shape[0]
    Linv = tri_inverse_ld(side_q["L"])
    step = M if M < 2 * block else block
    base = dict(Ki=side_q["Kuui"], S=side_q["S"], L=side_q["L"], Linv=Linv, Li=side_q["Li"], Hs=Hs)
    return Linv, [dict(base, r0=r0, r1=min(M, r0 + step)) for r0 in range(0, M, step)]


def heavy_join(parts, n):
    """[per bundle: dict G, GSK, dLdS, TL], Sinv  from the row-range results."""
    parts = sorted(parts, key=lambda p: p["r0"])
    Sinv = np.concatenate([p["Sinv"] for p in parts])
    return [{k: np.concatenate([p["per"][i][k] for p in parts]) for k in ("G", "GSK", "dLdS", "TL")} for i in range(n)], Sinv


# ================================================================================================ one latent
def _kzz(prm, prob, q):
    """(r2, kz in longdouble, gate, dz [P][M, M] = z_j - z_m) of K_zz as `kzz_rows_kernel` takes it."""
    P, M = prob["P"], prob["M"]
    Zq = _ld(prm["Z"][:, q * P:(q + 1) * P])
    var, ell = LD(float(prm["variance"][q])), LD(float(prm["lengthscale"][q]))
    d = Zq[None, :, :] - Zq[:, None, :]                      # [m, j, p] = z_j - z_m
    d2 = np.sum(d * d, axis=2)
    off = ~np.eye(M, dtype=bool)
    r2 = np.where(off, d2 / (ell * ell), LD(0))
    kz = var * np.exp(-r2 / 2)
    return r2, kz, (d2 != 0) & off, [d[:, :, p] for p in range(P)]


def latent_values(prm, prob, q, u, b, hv, strict):
    """The longdouble quantities of latent q from its bundle slice `b` (dict H, r, dZ, sa, sl, swk in longdouble) and the heavy
    products `hv` (dict G, GSK, dLdS, TL)."""
    M, P = prob["M"], prob["P"]
    Ki, a, m = u["Kuui"], u["a"], _ld(prm["m_u"][:, q])
    Kr = b["r"] if strict == "two" else (u["Li"].T if strict else Ki) @ b["r"]
    G, GSK = hv["G"], hv["GSK"]
    KSK = u["C"] + Ki
    X = G - GSK - GSK.T - Kr[:, None] * a[None, :]
    dK = (X + X.T) / 2 - (Ki / 2 - KSK / 2 - a[:, None] * a[None, :] / 2)
    r2, kz, gate, dz = _kzz(prm, prob, q)
    EK = dK * kz
    T2 = np.where(gate, EK + EK.T, LD(0))
    rows = dict(s1=EK.sum(1), s2=(EK * r2).sum(1), gz=np.stack([(T2 * dz[p]).sum(1) for p in range(P)], 1))
    kl4 = (np.sum(Ki * u["S"]), m @ a, np.sum(np.log(np.abs(np.diag(u["Luu"])))), np.sum(np.log(np.abs(np.diag(u["L"])))))
    return dict(Kr=Kr, dK=dK, rows=rows, kl4=kl4, kl=kl4[0] / 2 + kl4[1] / 2 - LD(M) / 2 + kl4[2] - kl4[3], gmu=Kr - a,
                gL=2 * hv["TL"][np.tril_indices(M)], dLdS=hv["dLdS"], winv=Ki - KSK)


def latent_scales(prm, prob, q, u, Linv_abs, ab, strict, const=True):
    """The float64 scales of latent q from the absolute values `ab` (dict H, r, dZ, sa, sl, swk, non-negative float64)."""
    M, P = prob["M"], prob["P"]
    Ka, La, Lia, Lua = np.abs(f64(u["Kuui"])), np.abs(f64(u["L"])), u["Li_abs"], np.abs(f64(u["Luu"]))
    z = np.zeros((M, M))
    if const:
        s_Li, sK = inv_scale(Lia, Lua)
        _, sSi = inv_scale(Linv_abs, La)
    else:
        s_Li, sK, sSi = z, z, z
    KA, LA = Ka + sK, Lia + s_Li
    a_abs = KA @ np.abs(prm["m_u"][:, q])          # s_a of the u-side, completed by K^-1's own scale (const=False: s_a itself)
    s_a = a_abs if const else np.zeros(M)
    Ha = ab["H"]
    if strict == "two":          # G = H and Kr = r, taken as exact: their scales are their absolute values
        S_G, S_Kr = Ha, ab["r"]
    elif strict:
        S_G = LA.T @ Ha @ LA - s_Li.T @ Ha @ s_Li
        S_Kr = LA.T @ ab["r"]
    else:
        S_G = KA @ Ha @ KA - sK @ Ha @ sK
        S_Kr = KA @ ab["r"]
    S_dLdS = S_G + (sK + sSi) / 2
    S_TL = S_dLdS @ La
    S_GSK = S_G @ (La @ La.T) @ KA
    S_X = S_G + S_GSK + S_GSK.T + S_Kr[:, None] * a_abs[None, :]
    S_dK = (S_X + S_X.T) / 2
    if const:
        Ba = Ka @ La
        S_dK = S_dK + sK / 2 + (Ba @ Ba.T) / 2 + a_abs[:, None] * a_abs[None, :] / 2
    r2, kz, gate, dz = _kzz(prm, prob, q)
    r2, kz = f64(r2), f64(kz)
    sEK = S_dK * kz
    T2 = np.where(gate, sEK + sEK.T, 0.0)
    rows = dict(s1=sEK.sum(1), s2=(sEK * r2).sum(1), gz=np.stack([(T2 * np.abs(f64(dz[p]))).sum(1) for p in range(P)], 1))
    out = dict(rows=rows, gmu=S_Kr + s_a, gL=2.0 * S_TL[np.tril_indices(M)], dLdS=S_dLdS, wv=s_a)
    if const:
        logs = lambda d: float(np.sum(np.abs(np.log(np.abs(f64(d))))))          # noqa: E731
        out["kl"] = ((KA * (La @ La.T)).sum() / 2 + float(np.abs(prm["m_u"][:, q]) @ a_abs) / 2 + M / 2.0
                     + logs(np.diag(u["Luu"])) + M + logs(np.diag(u["L"])))
        SS = La @ La.T
        out["winv"] = u["s_C"] + sK + sK @ SS @ Ka + Ka @ SS @ sK          # s_C of the u-side, completed likewise
    else:
        out["kl"], out["winv"] = 0.0, z
    return out


# ================================================================================================ the whole tail
def _slices(bundle, prob):
    b = rr.split_bundle(np.asarray(bundle), prob)
    return b, [dict(H=sym_lower(b["H"][q]), r=b["r"][q], dZ=b["dZ"][q], sa=b["sa"][q], sl=b["sl"][q], swk=b["swk"][q])
               for q in range(prob["Q"])]


def assemble(prm, prob, head, lat, absolute):
    """`finish_tail`'s host assembly: `head` = dict ve, sgv; `lat` [q] = dict kl, gmu, gL, dLdS, rows, winv, wv, dZ, sa, sl, swk.
    absolute=True: the same sums over absolute values (the scales)."""
    Q, M, P, Df = prob["Q"], prob["M"], prob["P"], prob["Df"]
    dt = np.float64 if absolute else LD
    ab = np.abs if absolute else (lambda x: x)
    W = np.asarray(prm["W"], float)
    W0, k0 = np.asarray(prm.get("W0", prm["W"]), float), np.asarray(prm.get("kappa0", prm["kappa"]), float)
    out = dict(kl=np.zeros(Q, dt), elbo=np.zeros(1, dt), g_m_u=np.zeros((M, Q), dt), g_L_u=np.zeros((M * (M + 1) // 2, Q), dt),
               dL_dS=np.zeros((Q, M, M), dt), g_variance=np.zeros(Q, dt), g_lengthscale=np.zeros(Q, dt), g_W=np.zeros((Q, Df), dt),
               g_kappa=np.zeros((Q, Df), dt), g_Z=np.zeros((M, Q * P), dt), wv=np.zeros((Q, M), dt), winv=np.zeros((Q, M, M), dt))
    sgv = head["sgv"].astype(dt)
    for q in range(Q):
        o = lat[q]
        var, ell = dt(float(prm["variance"][q])), dt(float(prm["lengthscale"][q]))
        out["kl"][q] = o["kl"]
        out["g_m_u"][:, q], out["g_L_u"][:, q], out["dL_dS"][q] = o["gmu"], o["gL"], o["dLdS"]
        out["wv"][q], out["winv"][q] = o["wv"], o["winv"]
        out["g_variance"][q] = o["rows"]["s1"].sum() / var + o["sa"] / var + np.sum(ab(_cast(W0[q] ** 2 + k0[q], dt)) * sgv)
        out["g_lengthscale"][q] = o["rows"]["s2"].sum() / ell + o["sl"] / ell
        out["g_W"][q] = ab(_cast(W[q], dt)) * sgv + o["swk"]              # util.py:230 (quirk Q4) + :252
        out["g_kappa"][q] = sgv                                           # util.py:231 (quirk Q5)
        out["g_Z"][:, q * P:(q + 1) * P] = o["dZ"] / (ell * ell) + o["rows"]["gz"] / (ell * ell)
    out["elbo"][0] = head["ve"].astype(dt)[0] + out["kl"].sum() if absolute else head["ve"].astype(dt)[0] - out["kl"].sum()
    return out


def _cast(a, dt):
    return np.asarray(a, dtype=np.float64).astype(dt)


def scales(prm, prob, side, Linv_abs, absb, strict=False, const=True):
    """S of every kind from `absb` = dict ve, sgv, H, r, dZ, sa, sl, swk of non-negative float64 arrays in the shapes of
    `rr.split_bundle` (const=True: the bundle's absolute values; const=False: a bound of the bundle's own error, see the module
    docstring)."""
    Q = prob["Q"]
    lat = []
    for q in range(Q):
        ab = {k: np.asarray(absb[k][q], dtype=np.float64) for k in ("H", "r", "dZ", "sa", "sl", "swk")}
        o = latent_scales(prm, prob, q, side[q], Linv_abs[q], ab, strict, const)
        o.update(dZ=ab["dZ"], sa=ab["sa"], sl=ab["sl"], swk=ab["swk"])
        lat.append(o)
    return assemble(prm, prob, dict(ve=np.asarray(absb["ve"], float), sgv=np.asarray(absb["sgv"], float)), lat, True)


def reference(prm, prob, side, bundle, strict=False, heavy=None):
    """(R, S, extra) of the tail on a bundle taken as exact (float64, or longdouble for the end-to-end cases).  `heavy` =
    ([per latent: dict G, GSK, dLdS, TL], [Linv per latent]) when a pool has formed the products; otherwise they are formed here.  extra: intermediate longdouble arrays per latent
    (G, GSK, dK, Kr, rows, kl4) for the sharpness tests."""
    Q = prob["Q"]
    b, sl = _slices(bundle, prob)
    if heavy is None:
        hv, Linvs = [], []
        for q in range(Q):
            Linv, jobs = heavy_jobs(side[q], [(as_ld(sl[q]["H"]), strict)])
            per, _ = heavy_join([heavy_rows(j) for j in jobs], 1)
            hv.append(per[0]), Linvs.append(Linv)
    else:
        hv, Linvs = heavy
    lat, extra = [], []
    for q in range(Q):
        bq = {k: as_ld(v) for k, v in sl[q].items()}
        o = latent_values(prm, prob, q, side[q], bq, hv[q], strict)
        o.update(dZ=bq["dZ"], sa=bq["sa"], sl=bq["sl"], swk=bq["swk"], wv=side[q]["a"])
        lat.append(o)
        extra.append(dict(G=hv[q]["G"], GSK=hv[q]["GSK"], dK=o["dK"], Kr=o["Kr"], rows=o["rows"], kl4=o["kl4"]))
    R = assemble(prm, prob, dict(ve=as_ld(b["ve"]), sgv=as_ld(b["sgv"])), lat, False)
    absb = {k: np.abs(np.asarray(b[k], dtype=np.float64)) for k in BUNDLE_KEYS}
    absb["H"] = np.stack([np.abs(f64(s["H"])) for s in sl])
    S = scales(prm, prob, side, [np.abs(f64(x)) for x in Linvs], absb, strict)
    return R, S, extra


# ================================================================================================ criterion
def worst_ratios(got, R, S, kinds=KINDS, B=None, C=None):
    """{kind: (worst ratio, flat index)}.  With B (a dict of float64 arrays) and C the bound of an element is 2^-52 (C[kind] S + B):
    the ratio reported is |got - R| / (2^-52 (S + B / C[kind])), to be held to C[kind] like any other."""
    out = {}
    for k in kinds:
        g = np.asarray(got[k], dtype=np.float64).reshape(np.shape(R[k]))
        s = np.asarray(S[k], dtype=np.float64)
        if B is not None:
            s = s + np.asarray(B[k], dtype=np.float64) / C[k]
        x = rr.ratios(g, R[k], s).reshape(-1)
        i = int(np.argmax(x))
        out[k] = (float(x[i]), i)
    return out


def check(case, got, R, S, C, kinds=KINDS, B=None):
    """Every element of every given kind within C[kind] * 2^-52 * S (+ 2^-52 B).  Prints the worst ratio per kind as
    `[tail] <case> <kind> ...` before asserting; returns {kind: worst ratio}."""
    w = worst_ratios(got, R, S, kinds, B, C)
    for k in kinds:
        print("[tail] %-30s %-13s worst |got - R| / (2^-52 S) = %-10.4g (C = %g) at [%d]" % (case, k, w[k][0], C[k], w[k][1]))
    bad = {k: (w[k], C[k]) for k in kinds if not w[k][0] <= C[k]}
    assert not bad, (case, "beyond C", bad)
    return {k: w[k][0] for k in kinds}


def assert_scales_dense(case, S, kinds=KINDS):
    """No element of S below 1e-8 of its array's largest: nothing is held only by the floor."""
    for k in kinds:
        s = np.asarray(S[k], dtype=np.float64)
        assert np.all(np.isfinite(s)) and s.min() > 0 and s.min() >= 1e-8 * s.max(), (case, k, float(s.min()), float(s.max()))
