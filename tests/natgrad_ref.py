"""Extended-precision restatement of the natural-gradient step on q(u) and its element-by-element criterion, and a NumPy
restatement of `adadelta_kernel`'s deferred recurrence.  Needs NumPy (and tests/linalg_ref.py / tests/tail_ref.py, whose `LD`, `EPS`,
`TINY`, `tri_inverse_ld`, `cholesky_ld`, `mm`, `ratios` and plain float64 algorithms are used as they are); imports neither the oracle
nor the package.

The step (`hmogp_engine::natgrad_core`), per latent q:

    Lambda = sym(S^-1 - 2 gamma dL_dS),   theta1 = S^-1 m + gamma (g_m - 2 dL_dS m),
    J Lambda J = R R^T,   L_new = anti-transpose of R^-1,   m_new = L_new (L_new^T theta1)        (S_new = Lambda^-1 = L_new L_new^T)

  input   m and L (from L_flat), the float64 parameters; dL_dS and g_m_u, the float64 arrays the evaluation EXPORTED, taken as exact
          (they are byte copies of the buffers the step reads: `dLdS` and `gmu` leave through one hipMemcpyAsync each on the regular
          path, engine.hip finish_enqueue; on the small path `finish_small_kernel` writes dL_dS into the same `dLdS` buffer and stores
          one value twice, into `gmu` and into the staging block g_m_u is copied from); gamma.
  S^-1    is not exported.  The reference forms it as Linv^T Linv in longdouble, Linv = tri_inverse_ld(L).  The device's own S^-1 is
          allowed 9f's `sinv` bound, c_kernel()["sinv"] 2^-52 S_sinv (S_sinv = `tail_ref.inv_scale(|Linv|, |L|)`), and that bound
          enters as a term B pushed through the step in absolute value, as tests/tail_cases.py cases (c) push the bundle's bound
          through the tail.

Criterion, per element and never an array maximum:   |quantity| <= 2^-52 (C[kind] max(S, 2^-1022) + B).
The residuals are formed in longdouble from the kernel's float64 output.  L^ = the unpacked L_flat_new.

  kind      quantity                                   S                                                  B
  ng_chol   L^^T Lambda L^ - I, full M x M             E + E^T + E E^T + |L^^T| A |L^|,                    |L^^T| (C_sinv S_sinv) |L^|
                                                       E = |L^^T| |L^^-T|,  A = sym(|S^-1| + 2 gamma |dL_dS|)
  ng_diag   diag(L^) > 0, L_flat_new all finite        none: a condition
  ng_mean   m^ - L^ (L^^T theta1), the kernel's own    |L^| (|L^^T| S_theta),                              |L^| |L^^T| (C_sinv S_sinv |m|)
            L^ taken as exact                          S_theta = |S^-1| |m| + gamma (|g_m| + 2 |dL_dS| |m|)

Derivation (u = 2^-53; gamma_M the usual a-priori constant, left to C as in 9f).
  ng_chol.  The device forms Lambda^ = fl(sym(S^^-1 - 2 gamma dL_dS)): |Lambda^ - Lambda| <= c u A + |S^^-1 - S^-1|, the second term
  within 2^-52 C_sinv S_sinv.  The Cholesky factorisation of J Lambda^ J is backward stable, R^ R^^T = J Lambda^ J + dA with |dA| <=
  gamma_M |R^| |R^^T| (Higham Thm 10.3); with U = J R^ J (upper) that reads U U^T = Lambda^ + dA', |dA'| <= gamma_M |U| |U^T|.  The
  triangular inverse X^ of R^ has the right residual |X^ R^ - I| <= gamma_M |X^| |R^| (Higham 14); the anti-transpose moves elements
  only, L^^T = J X^ J, hence L^^T U = I + F with |F| <= gamma_M |L^^T| |U|.  Together
      L^^T Lambda^ L^ = L^^T (U U^T - dA') L^ = I + F + F^T + F F^T - L^^T dA' L^,
  and to first order U = L^^-T, so |F| <= gamma_M E, |L^^T dA' L^| <= gamma_M |L^^T| |L^^-T| |L^^-1| |L^| = gamma_M E E^T, and the
  perturbation of Lambda itself is seen through |L^^T| . |L^|: the S and B of the table.  Every term is invariant under a row scaling
  of L (L -> D L scales L^ by D and Lambda by D^-1 on both sides), so the ratios do not grow with cond(Lambda).
  ng_mean.  theta1^ carries c u S_theta of its own two products and sums, plus |S^^-1 - S^-1| |m|.  The two matrix-vector products have
  the forward bounds gamma_M |L^^T| |theta1| and gamma_M |L^| |L^^T theta1|, and |theta1| <= S_theta element by element, so both are
  within gamma_M |L^| (|L^^T| S_theta); the error of theta1^ travels through the same two products in absolute value.

Constants.  C_ORACLE[kind] = the largest ratio of the plain float64 restatement `step_f64` (`tri_inverse_f64`, X^T X, `cholesky_f64` of
J Lambda J, flip and transpose, NumPy's matrix-vector products) over all cases of `CASES` (every one has M <= 330), rounded up to the
next power of two; tests/test_natgrad_ref_cpu.py re-measures and asserts it.  It is measured with B = 0: the restatement's own S^-1
(within 9f's C_ORACLE["sinv"] of the reference) is left to the constant, so no constant enters its own measurement.  C_KERNEL =
max(16, 4 C_ORACLE), the rule of 9a / 9c / 9f / 9g.  Never fitted to the kernels; there is no exception list."""
import numpy as np

import linalg_ref as lf
from linalg_ref import EPS, LD, TINY, cholesky_f64, cholesky_ld, ratios, tri_inverse_f64, tri_inverse_ld  # noqa: F401
from tail_ref import f64, inv_scale, mm

KINDS = ("ng_chol", "ng_mean")

# Largest ratio of `step_f64` over CASES, rounded up to a power of two (measured 2026-10-20 on the CPU; the raw figures per case are in
# DESIGN 9m).
C_ORACLE = dict(ng_chol=2.0, ng_mean=2.0)


def c_kernel():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE.items()}


def next_pow2(x):
    return 1.0 if x <= 1 else float(2.0 ** np.ceil(np.log2(x)))


# ================================================================================================ cases
# Shared by the CPU and the GPU test: exactly these steps are accepted (lambda_min(Lambda) > 0 is asserted for each on the CPU).
REGULAR = ["T33", "T65", "T129", "T200", "T330", "T144p2"]      # tail-only shapes of tests/tail_cases.py: injected dense bundle
SMALL = ["S33", "S50", "S64"]                                    # end to end, fused small-model path and regular path
GAMMAS = (0.01, 0.1)
GRADED = "T65"               # the conditioned case: T65 with the rows of L graded by powers of two
GRADED_SPAN = 10             # exponents in [-GRADED_SPAN, 0], both ends present: cond(Lambda) grows by about 2^(2 span)
GRADED_GAMMA = 0.1
REFUSED = ("T33", 1.0)       # latent 0 stays positive definite, latent 1 does not
CASES = [(t, g) for t in REGULAR + SMALL for g in GAMMAS] + [("graded", GRADED_GAMMA)]


def graded_L_flat(L_flat, M):
    """L_flat with row i of every latent's factor scaled by 2^e_i, e seeded integers in [-GRADED_SPAN, 0] with both ends present
    (powers of two: the scaled factor is exact)."""
    rng = np.random.RandomState(6500 + M)
    e = rng.randint(-GRADED_SPAN, 1, M)
    i, j = rng.choice(M, 2, replace=False)
    e[i], e[j] = -GRADED_SPAN, 0
    rows = np.tril_indices(M)[0]
    return np.asarray(L_flat, dtype=np.float64) * (2.0 ** e[rows])[:, None], e


def cpu_inputs(refs, tag):
    """(m_u, L_flat, dL_dS, g_m_u) of one case of tests/tail_cases.py as the CPU test takes them: the parameters, and the longdouble
    tail reference's dL_dS and g_m_u rounded to float64 in place of what the device exports.  tag "graded": the parameters of
    GRADED with `graded_L_flat`, dL_dS = G - (K^-1 - S^-1) / 2 re-formed in longdouble for the graded factor (G, K^-1 and g_m_u do not
    depend on L)."""
    base = GRADED if tag == "graded" else tag
    prm, prob = refs[base]["case"][0], refs[base]["case"][1]
    R = refs[base]["default"]["R"]
    if tag != "graded":
        return prm["m_u"], prm["L_flat"], f64(R["dL_dS"]), f64(R["g_m_u"])
    M, Q = prob["M"], prob["Q"]
    Lf, _ = graded_L_flat(prm["L_flat"], M)
    D = np.zeros((Q, M, M))
    for q in range(Q):
        Linv = tri_inverse_ld(unpack(Lf, M)[q].astype(LD))
        D[q] = f64(refs[base]["default"]["extra"][q]["G"] - (refs[base]["side"][q]["Kuui"] - mm(Linv.T, Linv)) / 2)
    return prm["m_u"], Lf, D, f64(R["g_m_u"])


# ================================================================================================ layout
def unpack(L_flat, M):
    """[Q, M, M] float64 lower-triangular factors from L_flat [M (M + 1) / 2, Q] (row-major lower triangle, latent fastest)."""
    L_flat = np.asarray(L_flat, dtype=np.float64)
    L_flat = L_flat.reshape(M * (M + 1) // 2, -1)
    out = np.zeros((L_flat.shape[1], M, M))
    r, c = np.tril_indices(M)
    for q in range(L_flat.shape[1]):
        out[q][r, c] = L_flat[:, q]
    return out


def pack(Ls):
    r, c = np.tril_indices(Ls[0].shape[0])
    return np.stack([np.asarray(L, dtype=np.float64)[r, c] for L in Ls], 1)


# ================================================================================================ reference
def base(m_u, L_flat, dL_dS, g_m_u):
    """The part of the reference that does not depend on gamma, per latent: S^-1 = Linv^T Linv, S^-1 m and dL_dS m in longdouble, and
    the float64 absolute values and S_sinv the scales are made of."""
    m_u = np.asarray(m_u, dtype=np.float64)
    M, Q = m_u.shape
    Ls, D, g = unpack(L_flat, M), np.asarray(dL_dS, dtype=np.float64).reshape(Q, M, M), np.asarray(g_m_u, dtype=np.float64).reshape(M, Q)
    out = []
    for q in range(Q):
        Ll, m, Dl, gl = Ls[q].astype(LD), m_u[:, q].astype(LD), D[q].astype(LD), g[:, q].astype(LD)
        Linv = tri_inverse_ld(Ll)
        Sinv = mm(Linv.T, Linv)
        _, s_sinv = inv_scale(np.abs(f64(Linv)), np.abs(Ls[q]))
        Sa, Da, ma = np.abs(f64(Sinv)), np.abs(D[q]), np.abs(m_u[:, q])
        out.append(dict(M=M, Sinv=Sinv, D=Dl, Sm=Sinv @ m, Dm=Dl @ m, g=gl, Sa=Sa, Da=Da, s_sinv=s_sinv,
                        Sa_m=Sa @ ma, Da_m=Da @ ma, ga=np.abs(g[:, q]), sinv_m=s_sinv @ ma))
    return out


def at_gamma(b, gamma):
    """Per latent: Lambda and theta1 in longdouble, the float64 scales A and S_theta, lambda_min and cond of Lambda."""
    out = []
    gl = LD(float(gamma))
    for u in b:
        X = u["Sinv"] - 2 * gl * u["D"]
        Lam = (X + X.T) / 2
        theta = u["Sm"] + gl * (u["g"] - 2 * u["Dm"])
        A = u["Sa"] + 2.0 * gamma * u["Da"]
        w = np.linalg.eigvalsh(f64(Lam))
        out.append(dict(M=u["M"], Lam=Lam, theta=theta, A=(A + A.T) / 2, S_theta=u["Sa_m"] + gamma * (u["ga"] + 2.0 * u["Da_m"]),
                        s_sinv=u["s_sinv"], sinv_m=u["sinv_m"], lam_min=float(w[0]), cond=float(w[-1] / w[0]) if w[0] > 0 else np.inf))
    return out


def reference(m_u, L_flat, dL_dS, g_m_u, gamma):
    return at_gamma(base(m_u, L_flat, dL_dS, g_m_u), gamma)


def latent_terms(ref, Lhat, mhat):
    """{kind: (quantity in longdouble, S, B without its constant)} of one latent for a float64 factor L^ (lower triangle read) and
    mean m^.  B is returned per unit of C_sinv: the caller multiplies."""
    Lh = np.tril(np.asarray(Lhat, dtype=np.float64))
    M = Lh.shape[0]
    Ll = Lh.astype(LD)
    with np.errstate(all="ignore"):
        quantity = mm(mm(Ll.T, ref["Lam"]), Ll) - np.eye(M, dtype=LD)
        La = np.abs(Lh)
        if np.all(np.isfinite(Lh)) and np.all(np.diag(Lh) != 0):
            Lia = np.abs(f64(tri_inverse_ld(Ll)))
        else:
            Lia = np.zeros((M, M))               # (a factor that fails ng_diag: the scale has no inverse to draw on)
        E = La.T @ Lia.T
        S_chol = E + E.T + E @ E.T + La.T @ ref["A"] @ La
        B_chol = La.T @ ref["s_sinv"] @ La
        mean = np.asarray(mhat, dtype=np.float64).astype(LD) - Ll @ (Ll.T @ ref["theta"])
        S_mean = La @ (La.T @ ref["S_theta"])
        B_mean = La @ (La.T @ ref["sinv_m"])
    return {"ng_chol": (quantity, S_chol, B_chol), "ng_mean": (mean, S_mean, B_mean)}


def diag_ok(L_flat_new, M):
    """ng_diag: every entry of L_flat_new finite and every diagonal entry of every factor positive."""
    Lf = np.asarray(L_flat_new, dtype=np.float64).reshape(M * (M + 1) // 2, -1)
    i = np.arange(M)
    return bool(np.all(np.isfinite(Lf)) and np.all(Lf[i * (i + 1) // 2 + i] > 0))


def worst_ratios(refs_q, m_new, L_flat_new, C, with_B=True):
    """{kind: (worst ratio over latents and elements, latent, flat index)}: the ratio reported is
    |quantity| / (2^-52 (max(S, 2^-1022) + B / C[kind])), to be held to C[kind] like any other (tail_ref.worst_ratios).  with_B=False
    leaves B out: how C_ORACLE is measured."""
    M = refs_q[0]["M"]
    Ls, m_new = unpack(L_flat_new, M), np.asarray(m_new, dtype=np.float64).reshape(M, -1)
    c_sinv = lf.c_kernel()["sinv"]
    out = {}
    for q, ref in enumerate(refs_q):
        for k, (quantity, S, B) in latent_terms(ref, Ls[q], m_new[:, q]).items():
            with np.errstate(all="ignore"):
                x = ratios(quantity, np.maximum(S, TINY) + (c_sinv * B / C[k] if with_B else 0.0)).reshape(-1)
            i = int(np.argmax(x))
            if k not in out or not float(x[i]) <= out[k][0]:
                out[k] = (float(x[i]), q, i)
    return out


def check(case, refs_q, m_new, L_flat_new, C, with_B=True):
    """ng_diag holds and every element of ng_chol and ng_mean is within 2^-52 (C[kind] S + B).  Prints the worst ratio per kind as
    `[natgrad] <case> <kind> ...` before it asserts; returns {kind: worst ratio}."""
    M = refs_q[0]["M"]
    ok = diag_ok(L_flat_new, M)
    print("[natgrad] %-34s %-8s %s" % (case, "ng_diag", "holds" if ok else "VIOLATED"))
    w = worst_ratios(refs_q, m_new, L_flat_new, C, with_B)
    for k in KINDS:
        print("[natgrad] %-34s %-8s worst |quantity| / (2^-52 (S + B / C)) = %-10.4g (C = %g) at latent %d [%d]" % (
            case, k, w[k][0], C[k], w[k][1], w[k][2]))
    assert ok, (case, "ng_diag")
    bad = {k: (w[k][0], C[k]) for k in KINDS if not w[k][0] <= C[k]}
    assert not bad, (case, "beyond C", bad)
    return {k: w[k][0] for k in KINDS}


def assert_scales_dense(case, refs_q, m_new, L_flat_new):
    """No element of S below 1e-8 of its array's largest: nothing is held only by the floor."""
    M = refs_q[0]["M"]
    Ls, m_new = unpack(L_flat_new, M), np.asarray(m_new, dtype=np.float64).reshape(M, -1)
    for q, ref in enumerate(refs_q):
        for k, (_, S, _) in latent_terms(ref, Ls[q], m_new[:, q]).items():
            assert np.all(np.isfinite(S)) and S.min() > TINY and S.min() >= 1e-8 * S.max(), (case, q, k, float(S.min()), float(S.max()))


# ================================================================================================ plain float64 restatement
def step_f64(m_u, L_flat, dL_dS, g_m_u, gamma, lam_factor=2.0, theta_dlds=True, reversed_route=True, gemv_t_rows=None):
    """The step in plain float64, in the kernels' order of formation: S^-1 = X^T X with X = `tri_inverse_f64(L)`, Lambda symmetrised as
    `natgrad_prec_kernel` does, `cholesky_f64` of J Lambda J, `tri_inverse_f64`, flip and transpose, two matrix-vector products.
    Returns (m_new [M, Q], L_flat_new [M (M + 1) / 2, Q]); raises LinAlgError when a latent leaves the positive-definite cone.
    The keyword arguments state what a wrong kernel would compute (tests/test_natgrad_ref_cpu.py): `lam_factor` for the 2 of 2 gamma in
    Lambda, `theta_dlds=False` drops - 2 dL_dS m from theta1, `reversed_route=False` factorises Lambda itself and packs the plain
    inverse of its factor, `gemv_t_rows=n` sums L^T theta1 over the first n rows only."""
    m_u = np.asarray(m_u, dtype=np.float64)
    M, Q = m_u.shape
    Ls, D, g = unpack(L_flat, M), np.asarray(dL_dS, dtype=np.float64).reshape(Q, M, M), np.asarray(g_m_u, dtype=np.float64).reshape(M, Q)
    m_new, L_new = np.zeros((M, Q)), []
    for q in range(Q):
        X = tri_inverse_f64(Ls[q])
        Sinv = X.T @ X
        Y = Sinv - lam_factor * gamma * D[q]
        Lam = 0.5 * (Y + Y.T)
        t2 = D[q] @ m_u[:, q]
        theta = Sinv @ m_u[:, q] + gamma * (g[:, q] - (2.0 * t2 if theta_dlds else 0.0))
        if reversed_route:
            Rinv = tri_inverse_f64(cholesky_f64(Lam[::-1, ::-1]))
            Ln = np.ascontiguousarray(Rinv[::-1, ::-1].T)
        else:
            Ln = tri_inverse_f64(cholesky_f64(Lam))
        n = M if gemv_t_rows is None else gemv_t_rows
        m_new[:, q] = Ln @ (Ln[:n].T @ theta[:n])
        L_new.append(Ln)
    return m_new, pack(L_new)


# ================================================================================================ Adadelta
def adadelta_state(x):
    """The five arrays of the device-resident recurrence at `hmogp_qu_load`: x, and gms, sms, step, pend zeroed."""
    x = np.array(x, dtype=np.float64).reshape(-1)
    return dict(x=x, gms=np.zeros_like(x), sms=np.zeros_like(x), step=np.zeros_like(x), pend=np.zeros_like(x))


def adadelta_phase(s, phase, grad, rate, m, d, omd, o):
    """One launch of `adadelta_kernel` on the state `s` (in place), every operation its own NumPy call in the kernel's order, so each is
    separately rounded.  phase 0: x = (x - pend) - m step, pend = 0.  phase 1: the accumulators and pend from g = -grad (`grad` None:
    g = 0, the kernel's `grad == nullptr` branch)."""
    step1 = np.multiply(s["step"], m)
    if phase == 0:
        xv = np.subtract(s["x"], s["pend"])
        s["x"] = np.subtract(xv, step1)
        s["pend"] = np.zeros_like(s["x"])
        return s
    g = np.zeros_like(s["x"]) if grad is None else np.multiply(-1.0, np.asarray(grad, dtype=np.float64).reshape(-1))
    t1 = np.multiply(g, g)
    t1 = np.multiply(t1, omd)
    gm = np.multiply(s["gms"], d)
    gm = np.add(gm, t1)
    s["gms"] = gm
    a = np.sqrt(np.add(s["sms"], o))
    b = np.sqrt(np.add(gm, o))
    a = np.divide(a, b)
    a = np.multiply(a, g)
    a = np.multiply(a, rate)
    s["pend"] = a
    st = np.add(step1, a)
    s["step"] = st
    t2 = np.multiply(st, st)
    t2 = np.multiply(t2, omd)
    sm = np.multiply(s["sms"], d)
    s["sms"] = np.add(sm, t2)
    return s
