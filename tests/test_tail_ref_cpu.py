"""CPU: the extended-precision reference of the gradient tail (tests/tail_ref.py) against the float64 NumPy oracle.
  (a) every case is dense and well-conditioned (asserted on the scales themselves: no element is held only by the floor), and the
      oracle's own tail (`so.u_algebra` + `so.finish` on the same float64 bundle) sits within C_ORACLE of R in every element of every
      kind -- the measurement C_ORACLE was taken from, re-measured here;
  (b) the element-wise criterion rejects nine seeded indexing corruptions of the oracle's own output (arithmetic on arrays: nothing
      is run wrongly), while the array-maximum yardstick of the existing tests is asked the same of corruptions 1-3 on the banded case;
  (c) the end-to-end bound of the small-model cases (tail bound + the bundle's own 9c bound pushed through the tail) holds for the
      oracle end to end."""
import numpy as np
import pytest

import rowpass_cases as rc
import rowpass_ref as rr
import tail_cases as tc
import tail_ref as tr
from conftest import rel_norm
from model_cases import KEYS

TILE = 128
ALL_TAGS = rc.BASE_TAGS + list(tc.TAIL_ONLY)
VARIANTS = [(t, "default") for t in ALL_TAGS] + [("D", "bs"), ("D", "strict")]


@pytest.fixture(scope="module")
def refs():
    return tc.references()


# ================================================================================================ the oracle's tail
def plain_tail(prm, prob, u, stats, hooks=None):
    """`so.finish` restated operation by operation in float64 (asserted bit-identical to it below), with named places where a test
    may interfere: hooks[name](q, ...) for name in G, TL, dKmm, rowmask, tr.  Returns the kinds of tail_ref and, under "keep", the
    intermediate arrays per latent."""
    from oracle import svmogp_oracle as so
    hooks = hooks or {}
    Q, M, P, Df = prob["Q"], prob["M"], prob["P"], prob["Df"]
    b = rr.split_bundle(stats, prob)
    W0, k0 = prm.get("W0", prm["W"]), prm.get("kappa0", prm["kappa"])
    out = dict(kl=np.zeros(Q), elbo=np.zeros(1), g_m_u=np.zeros((M, Q)), g_L_u=np.zeros((M * (M + 1) // 2, Q)), dL_dS=np.zeros((Q, M, M)),
               g_variance=np.zeros(Q), g_lengthscale=np.zeros(Q), g_W=np.zeros((Q, Df)), g_kappa=np.zeros((Q, Df)),
               g_Z=np.zeros((M, Q * P)), wv=np.zeros((Q, M)), winv=np.zeros((Q, M, M)), keep=[])
    KL = 0.0
    sgv = b["sgv"]
    strict = bool(prob.get("strict_qf"))
    for q in range(Q):
        H, r, dZs, sa, sl, swk = b["H"][q], b["r"][q], b["dZ"][q], b["sa"][q], b["sl"][q], b["swk"][q]
        Ki, S, L_q, a = u["Kuui"][q], u["S"][q], u["L"][q], u["a"][q]
        m, var, ell = prm["m_u"][:, q], prm["variance"][q], prm["lengthscale"][q]
        trace = hooks["tr"](q, Ki * S) if "tr" in hooks else np.sum(Ki * S)
        klq = 0.5 * trace + 0.5 * m @ a - 0.5 * M + np.sum(np.log(np.abs(np.diag(u["Luu"][q])))) - np.sum(np.log(np.abs(np.diag(L_q))))
        KL += klq
        S_qi, _ = so.potri_sym(L_q)
        if strict and u["strict_two"]:          # the two-solve form: the bundle already holds dVE_dS and dVE_dmu
            G, Kr = H, r
        elif strict:
            import scipy.linalg
            Y1 = scipy.linalg.solve_triangular(u["Luu"][q], H, lower=True, trans="T")
            G = scipy.linalg.solve_triangular(u["Luu"][q], Y1.T, lower=True, trans="T")
            G = 0.5 * (G + G.T)
            Kr = scipy.linalg.solve_triangular(u["Luu"][q], r, lower=True, trans="T")
        else:
            G = Ki @ H @ Ki
            Kr = Ki @ r
        if "G" in hooks:
            G = hooks["G"](q, G)
        KiS = Ki @ S
        GSK = G @ KiS.T
        if "dKmm" in hooks:
            dKmm = hooks["dKmm"](q, G, GSK, Kr, a, Ki, KiS)
        else:
            dVE = G - GSK - GSK.T - np.outer(Kr, a)
            dVE = 0.5 * (dVE + dVE.T)
            dKmm = dVE - (0.5 * Ki - 0.5 * KiS @ Ki - 0.5 * np.outer(a, a))
        dL_dS = G - 0.5 * (Ki - S_qi)
        TL = hooks["TL"](q, dL_dS, L_q) if "TL" in hooks else 2.0 * dL_dS @ L_q
        Zq = prm["Z"][:, q * P:(q + 1) * P]
        r2 = so.rbf_r2_scaled(Zq, Zq, ell, same=True)
        EK = dKmm * (var * np.exp(-0.5 * r2))
        mask = hooks["rowmask"](q, M) if "rowmask" in hooks else np.ones(M)
        gvar = np.sum(EK * mask[:, None]) / var + sa / var + np.sum((W0[q] ** 2 + k0[q]) * sgv)
        gell = np.sum(EK * mask[:, None] * r2) / ell + sl / ell
        gZ = dZs / ell ** 2
        T2 = EK + EK.T
        for pp in range(P):
            gZ[:, pp] += mask * np.sum(T2 * (r2 != 0.0) * (Zq[:, pp][None, :] - Zq[:, pp][:, None]), 1) / ell ** 2
        out["kl"][q], out["g_m_u"][:, q], out["g_L_u"][:, q], out["dL_dS"][q] = klq, Kr - a, so.tril_to_flat(TL), dL_dS
        out["g_variance"][q], out["g_lengthscale"][q], out["g_W"][q], out["g_kappa"][q] = gvar, gell, prm["W"][q] * sgv + swk, sgv
        out["g_Z"][:, q * P:(q + 1) * P] = gZ
        out["wv"][q], out["winv"][q] = a, -u["C"][q]
        out["keep"].append(dict(G=G, GSK=GSK, Kr=Kr, TL=TL, dL_dS=dL_dS, dKmm=dKmm))
    out["elbo"][0] = stats[0] - KL
    return out


def oracle_tail(case, bundle, strict=False, hooks=None):
    from oracle import svmogp_oracle as so
    prm, prob, X, Y, rungs = case
    p = dict(prob, strict_qf="two_solves" if strict == "two" else True) if strict else prob
    u = so.u_algebra(prm, p, rungs)
    assert not strict or u["strict_two"] == (strict == "two")          # True: the one-solve form; "two": the two-solve form, forced
    return plain_tail(prm, p, u, np.asarray(bundle, dtype=np.float64), hooks), u, p


def test_plain_tail_is_the_oracles_finish(refs):
    """The restatement the corruptions are applied to gives the bits of `so.finish` (case B: ragged M, P = 2; D strict)."""
    from oracle import svmogp_oracle as so
    for tag, variant in (("B", "default"), ("D", "strict"), ("D", "strict2")):
        o = refs[tag][variant]
        got, u, p = oracle_tail(refs[tag]["case"], o["bundle"], o["strict"])
        want = so.finish(refs[tag]["case"][0], p, u, np.asarray(o["bundle"], dtype=np.float64))
        for k in ("g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"):
            assert np.array_equal(got[k], want[k]), (tag, k)
        assert got["elbo"][0] == want["elbo"] and np.array_equal(got["dL_dS"], np.stack(want["dL_dS"]))
        assert abs(got["kl"].sum() - want["KL"]) <= 4 * np.finfo(float).eps * abs(want["KL"])


# ================================================================================================ (a) cases and constants
@pytest.mark.parametrize("tag", ALL_TAGS + list(tc.SMALL))
def test_cases_are_dense_and_well_conditioned(refs, tag):
    f = refs[tag]["facts"]
    M = refs[tag]["case"][1]["M"]
    print("[tail] %-7s cond(S_q) = %s   cond(K_uu + jitter) = %s" % (
        tag, " ".join("%.1f" % c for c in f["cond_S"]), " ".join("%.0f" % c for c in f["cond_K"])))
    assert max(f["cond_K"]) <= 2 * (M + 1), f["cond_K"]
    assert max(f["cond_S"]) <= 1e2, f["cond_S"]
    for variant in ("default", "bs", "strict"):
        if variant in refs[tag]:
            tr.assert_scales_dense(tag + " " + variant, refs[tag][variant]["S"])


_MEASURED = {}


def _measure(refs, tag, variant):
    if (tag, variant) not in _MEASURED:
        o = refs[tag][variant]
        got, _, _ = oracle_tail(refs[tag]["case"], o["bundle"], o["strict"])
        _MEASURED[(tag, variant)] = (got, tr.worst_ratios(got, o["R"], o["S"]))
    return _MEASURED[(tag, variant)]


@pytest.mark.parametrize("tag,variant", VARIANTS)
def test_oracle_within_c_oracle(refs, tag, variant):
    """The float64 oracle's tail against R, every kind, every element.  F and M = 576 are no part of the maximum: held to C_KERNEL."""
    o = refs[tag][variant]
    got, _ = _measure(refs, tag, variant)
    C = tr.C_ORACLE if tag in tc.IN_MAXIMUM else tr.c_kernel()
    tr.check("oracle %s %s" % (tag, variant), got, o["R"], o["S"], C)


def test_c_oracle_is_the_remeasured_maximum(refs):
    """C_ORACLE re-measured: the largest ratio per kind over A-E, D's variants and the tail-only shapes with M <= 330, rounded up to a
    power of two, is what tail_ref.C_ORACLE holds (never below it); C_KERNEL follows the rule."""
    worst = {k: 0.0 for k in tr.KINDS}
    for tag, variant in VARIANTS:
        if tag in tc.IN_MAXIMUM:
            w = _measure(refs, tag, variant)[1]
            print("[tail] oracle %-7s %-8s %s" % (tag, variant, " ".join("%s %.3g" % (k, w[k][0]) for k in tr.KINDS)))
            for k in tr.KINDS:
                worst[k] = max(worst[k], w[k][0])
    measured = {k: tr.next_pow2(worst[k]) for k in tr.KINDS}
    print("[tail] C_ORACLE re-measured:", measured)
    ck = tr.c_kernel()
    for k in tr.KINDS:
        c = tr.C_ORACLE[k]
        assert measured[k] <= c, (k, worst[k], c)
        assert c >= 1 and np.log2(c) == int(np.log2(c)) and ck[k] == max(16.0, 4.0 * c)
    assert not tr.KERNEL_EXCEPTIONS


def test_two_solve_tail_within_c_oracle_and_rejects_the_one_solve_bundle(refs):
    """D `strict2`: the bundle holds dVE_dS = A^T diag(beta) A and dVE_dmu = A^T alpha themselves, the tail takes G = H and
    Kr = r.  The oracle's two-solve tail is measured against R: every kind within the present C_ORACLE except dL_dS and g_L_u, which
    get C_ORACLE_TWO = the measured ratio rounded up to a power of two (tail_ref.py says why) and C_KERNEL_TWO = max(16, 4 C_ORACLE_TWO),
    for this variant only.  The one-solve bundle (X^T diag(beta) X, X^T alpha) handed to the two-solve tail lands beyond C_KERNEL_TWO
    by more than 2^10 in dL_dS and g_m_u."""
    o, case = refs["D"]["strict2"], refs["D"]["case"]
    assert o["strict"] == "two"
    tr.assert_scales_dense("D strict2", o["S"])
    got, _, _ = oracle_tail(case, o["bundle"], "two")
    w = tr.check("oracle D strict2", got, o["R"], o["S"], tr.C_ORACLE_TWO)
    moved = {k for k in tr.KINDS if tr.C_ORACLE_TWO[k] != tr.C_ORACLE[k]}
    assert moved == {"dL_dS", "g_L_u"} and all(tr.C_ORACLE_TWO[k] == tr.next_pow2(w[k]) for k in moved)      # the rule, re-measured
    assert all(tr.c_kernel_two()[k] == max(16.0, 4.0 * tr.C_ORACLE_TWO[k]) for k in tr.KINDS)
    print("[strict2] oracle tail D strict2 %s" % " ".join("%s %.3g" % (k, w[k]) for k in tr.KINDS))
    bad, _, _ = oracle_tail(case, refs["D"]["strict"]["bundle"], "two")
    ck = tr.c_kernel_two()
    for kind in ("dL_dS", "g_m_u"):
        ratio = _worst(bad, o, kind)
        print("[strict2] corruption one-solve bundle in the two-solve tail %-6s ratio %.3g (C_KERNEL_TWO = %g)" % (kind, ratio, ck[kind]))
        assert ratio > 1024 * ck[kind], (kind, ratio)


@pytest.mark.parametrize("tag", list(tc.SMALL))
def test_small_model_bound_holds_for_the_oracle_end_to_end(refs, tag):
    """Cases (c): `so.elbo_grad_fused` end to end (its own float64 row pass) within 2^-52 (C_KERNEL S_tail + B)."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y, rungs = refs[tag]["case"]
    u = so.u_algebra(prm, prob, rungs)
    stats, _ = so.local_stats(prm, prob, u, X, Y)
    got = plain_tail(prm, prob, u, stats)
    o = refs[tag]["default"]
    assert all(np.all(np.asarray(o["B"][k]) == 0) for k in ("kl", "wv", "winv"))
    tr.check("oracle e2e " + tag, got, o["R"], o["S"], tr.c_kernel(), B=o["B"])


# ================================================================================================ (b) sharpness
def _tile_not_mirrored(q0):
    def hook(q, G):
        if q == q0:
            G = G.copy()
            G[0:TILE, 2 * TILE:3 * TILE] = 0.0
        return G
    return hook


def _late_k_range(q0):
    def hook(q, dL_dS, L):
        T = 2.0 * dL_dS @ L
        if q == q0:
            T[:, TILE:2 * TILE] = 2.0 * dL_dS[:, 2 * TILE:] @ L[2 * TILE:, TILE:2 * TILE]
        return T
    return hook


def _gsk_not_transposed(q0, i0, j0):
    def hook(q, G, GSK, Kr, a, Ki, KiS):
        ka = np.outer(Kr, a)
        dVE = G - GSK - GSK.T - ka
        dVE = 0.5 * (dVE + dVE.T)
        if q == q0:                    # the mirrored tile read untransposed: s_ji := s_ij inside the tile, in x_ij and in x_ji
            t = (slice(i0, i0 + 32), slice(j0, j0 + 32))
            xij = G[t] - GSK[t] - GSK[t] - ka[t]
            xji = G.T[t] - GSK[t] - GSK[t] - ka.T[t]
            dVE[t] = 0.5 * (xij + xji)
        return dVE - (0.5 * Ki - 0.5 * KiS @ Ki - 0.5 * np.outer(a, a))
    return hook


def _worst(got, o, kind):
    return tr.worst_ratios(got, o["R"], o["S"], (kind,))[kind][0]


def _ceiling(o, kind, Rbad):
    """The largest ratio a corruption can reach: the corruption applied to R itself, |R_bad - R| / (2^-52 S)."""
    return float(rr.ratios(tr.f64(Rbad), o["R"][kind], o["S"][kind]).max())


def test_criterion_rejects_indexing_corruptions(refs):
    """Nine seeded corruptions of the ORACLE's own output, each what an indexing error in a kernel of the tail would leave behind.
    Each must land beyond C_KERNEL * 2^20 of every kind it is listed with.  Where it cannot -- g_variance and g_lengthscale are sums of
    M^2 addends bounded by S(dL_dKmm) K_zz each, of which one row or one 32 x 32 tile is a small part -- the ceiling is derived by
    applying the corruption to R itself in longdouble, and asserted is: beyond C_KERNEL and at least half the ceiling.  The ratios
    reached are recorded in DESIGN 9g."""
    CK = tr.c_kernel()
    q = 1
    reached = []

    def run(tag, what, kinds, hooks=None, edit=None, ceil=None):
        o = refs[tag]["default"]
        got, u, _ = oracle_tail(refs[tag]["case"], o["bundle"], hooks=hooks)
        if edit is not None:
            edit(got, u)
        cl = ceil(refs[tag], o) if ceil else {}
        for kind in kinds:
            reached.append((what, tag, kind, _worst(got, o, kind), o, got, cl.get(kind)))

    run("T330", "1 G tile (0,2) not mirrored", ("dL_dS", "g_L_u"), dict(G=_tile_not_mirrored(q)))
    run("T330", "2 dL_dS L: k-range of column tile 1 one tile late", ("g_L_u",), dict(TL=_late_k_range(q)))

    def ceil3(ref, o):
        prm, prob = ref["case"][0], ref["case"][1]
        P = prob["P"]
        ell = tr.LD(float(prm["lengthscale"][q]))
        GSK = o["extra"][q]["GSK"]
        r2, kz, gate, dz = tr._kzz(prm, prob, q)
        dEK = np.zeros_like(GSK)
        dEK[64:96, 0:32] = (GSK.T - GSK)[64:96, 0:32] * kz[64:96, 0:32]           # d dK_ij = GSK_ji - GSK_ij inside the tile
        gl = o["R"]["g_lengthscale"].copy()
        gl[q] += (dEK * r2).sum() / ell
        gz = o["R"]["g_Z"].copy()
        for p in range(P):
            gz[:, q * P + p] += (np.where(gate, dEK + dEK.T, 0) * dz[p]).sum(1) / (ell * ell)
        return dict(g_lengthscale=_ceiling(o, "g_lengthscale", gl), g_Z=_ceiling(o, "g_Z", gz))
    run("T200", "3 GSK for GSK^T in one 32 x 32 tile of dL_dKmm", ("g_Z", "g_lengthscale"), dict(dKmm=_gsk_not_transposed(q, 64, 0)),
        ceil=ceil3)

    def last_row(qq, M):
        mask = np.ones(M)
        if qq == q:
            mask[M - 1] = 0.0
        return mask

    def ceil4(ref, o):
        prm, prob = ref["case"][0], ref["case"][1]
        P, rows = prob["P"], o["extra"][q]["rows"]
        var, ell = tr.LD(float(prm["variance"][q])), tr.LD(float(prm["lengthscale"][q]))
        gv, gl, gz = o["R"]["g_variance"].copy(), o["R"]["g_lengthscale"].copy(), o["R"]["g_Z"].copy()
        gv[q] -= rows["s1"][-1] / var
        gl[q] -= rows["s2"][-1] / ell
        gz[-1, q * P:(q + 1) * P] -= rows["gz"][-1] / (ell * ell)
        return dict(g_variance=_ceiling(o, "g_variance", gv), g_lengthscale=_ceiling(o, "g_lengthscale", gl), g_Z=_ceiling(o, "g_Z", gz))
    run("T257", "4 last row missing from the kzz_rows sums", ("g_variance", "g_lengthscale", "g_Z"), dict(rowmask=last_row), ceil=ceil4)

    def block_dropped(qq, prod):
        flat = prod.reshape(-1)
        if qq != q:
            return np.sum(prod)
        blk = (np.arange(flat.size) // 256) % tr.KL_BLOCKS
        return np.sum(prod) - np.sum(flat[blk == 5])
    run("T330", "5 one block partial of the trace dropped", ("kl", "elbo"), dict(tr=block_dropped))

    def swap_pack(got, u):
        r = 100
        T = got["keep"][q]["TL"]
        got["g_L_u"][r * (r + 1) // 2:r * (r + 1) // 2 + r + 1, q] = T[:r + 1, r]
    run("T330", "6 pack_gl with (r, c) swapped for one row", ("g_L_u",), edit=swap_pack)

    def swap_gz(got, u):
        got["g_Z"][[100, 101], q] = got["g_Z"][[101, 100], q]
    run("T330", "7 g_Z of two adjacent inducing points exchanged", ("g_Z",), edit=swap_gz)

    def wrong_kr(got, u):
        got["g_m_u"][:, 0] = got["keep"][1]["Kr"] - u["a"][0]
    run("T330", "8 Kr of latent 1 used for latent 0", ("g_m_u",), edit=wrong_kr)

    def plus_c(got, u):
        got["winv"][q, 2 * TILE:, 0:TILE] = -got["winv"][q, 2 * TILE:, 0:TILE]
    run("T330", "9 winv with C for -C in one tile", ("winv",), edit=plus_c)

    for what, tag, kind, ratio, o, got, cl in reached:
        print("[tail] corruption %-52s %-5s %-13s ratio %.3g = %.3g x C_KERNEL%s" % (
            what, tag, kind, ratio, ratio / CK[kind], "" if cl is None else "   (ceiling %.3g)" % cl))
    for what, tag, kind, ratio, o, got, cl in reached:
        if cl is not None and cl < CK[kind] * 2.0 ** 20:
            assert ratio > CK[kind] and ratio >= cl / 2, (what, kind, ratio, cl)
        else:
            assert ratio > CK[kind] * 2.0 ** 20, (what, kind, ratio)
        with pytest.raises(AssertionError):
            tr.check("corrupted: " + what, got, o["R"], o["S"], CK, (kind,))


def test_array_maximum_yardstick_on_the_banded_case():
    """The other side: corruptions 1-3 on the EXISTING style of case (`rc.banded_case()`, M = 384, lengthscale about one inducing
    spacing), judged as `model_cases._parity` judges: max|a - b| / max|b| < 1e-8 on every array of KEYS.  Asserted is the side of
    1e-8 each falls on, as measured (recorded in DESIGN 9g)."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = rc.banded_case()
    u = so.u_algebra(prm, prob)
    stats, _ = so.local_stats(prm, prob, u, X, Y)
    want = plain_tail(prm, prob, u, stats)
    want["elbo"] = want["elbo"][0]
    seen = {}
    for what, hooks in (("1", dict(G=_tile_not_mirrored(1))), ("2", dict(TL=_late_k_range(1))),
                        ("3", dict(dKmm=_gsk_not_transposed(1, 256, 0)))):
        bad = plain_tail(prm, prob, u, stats, hooks)
        bad["elbo"] = bad["elbo"][0]
        seen[what] = max(rel_norm(bad[k], want[k]) for k in KEYS)
        print("[tail] banded M = 384: corruption %s: largest max|a - b| / max|b| over KEYS = %.3g" % (what, seen[what]))
    # 1 and 3 leave the same bits (the far tiles of G and of GSK are exactly 0.0 there): the yardstick is blind.  2 IS caught: a k-range
    # that starts one tile late loses the diagonal block of L (elements of 0.6 ... 1), whatever the lengthscale
    assert seen["1"] < 1e-8 and seen["3"] < 1e-8 and seen["2"] > 1e-8, seen
