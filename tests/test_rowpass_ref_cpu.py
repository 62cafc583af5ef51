"""CPU: the extended-precision reference of the row pass (tests/rowpass_ref.py) against the float64 NumPy oracle.
  (a) the cases are dense and well-conditioned (asserted on R, so that a case cannot silently go banded again), and the oracle sits
      within C_ORACLE of R in every element of every kind -- the measurement C_ORACLE was taken from;
  (b) the element-wise criterion rejects seeded indexing corruptions of the oracle's own output of case D (arithmetic on arrays:
      nothing is run wrongly), while the array-maximum yardstick of the existing tests accepts a far Gram tile that is transposed or
      never written on the banded case of the same shape;
  (c) the references of all cases are built once, in a pool of at most 16 processes (printed: about 50 s on 8 CPUs, 25 s on 16);
  (d) cases G, H, I (3-D / 4-D inputs, eight latents) are held to C_ORACLE_WIDE, and the criterion rejects what a wrong X stride, a dZ
      component at the wrong p, a latent's bundle block at the wrong q or a quadrature that mixes three latents only would leave."""
import numpy as np
import pytest

import rowpass_cases as rc
import rowpass_ref as rr
from conftest import rel_norm

TILE = 128


@pytest.fixture(scope="module")
def refs():
    return rc.references()


def oracle_outputs(prm, prob, X, Y, rungs, bs=None, row_begin=None, row_end=None, strict=False, keep=None):
    """Everything the criterion compares, from the float64 oracle: the bundle (`so.u_algebra` + `so.local_stats`), and from the
    per-row quantities behind it dL_dKmn = a gm^T + 2 w (gv P~)^T, dL_dKdiag = gv, and q(f)."""
    from oracle import svmogp_oracle as so
    p = dict(prob, strict_qf="two_solves" if strict == "two" else True) if strict else prob
    u = so.u_algebra(prm, p, rungs)
    # strict=True: the one-solve form, as the engine picks it at this conditioning; strict="two": the two-solve form, forced
    assert not strict or u["strict_two"] == (strict == "two")
    T, Q, Df = prob["T"], prob["Q"], prob["Df"]
    b = [0] * T if row_begin is None else row_begin
    e = [x.shape[0] for x in X] if row_end is None else row_end
    Xs, Ys = [X[t][b[t]:e[t]] for t in range(T)], [Y[t][b[t]:e[t]] for t in range(T)]
    rows = []
    stats, _ = so.local_stats(prm, p, u, Xs, Ys, bs, rows_out=rows)
    got = rr.split_bundle(stats, prob)
    got.update(dKmn=[[None] * Df for _ in range(Q)], dKdiag=[[None] * Df for _ in range(Q)], m=[None] * Df, v=[None] * Df)
    for o in rows:
        for j, d in enumerate(so._task_functions(prob, o["t"])):
            got["m"][d], got["v"][d] = o["m"][:, j], o["v"][:, j]
            for q in range(Q):
                got["dKmn"][q][d] = u["a"][q][:, None] * o["gm"][:, j][None, :] + 2.0 * prm["W"][q, d] * o["gv"][:, j][None, :] * o["Pt"][q].T
                got["dKdiag"][q][d] = o["gv"][:, j]
    if keep is not None:
        keep.update(u=u, rows=rows, stats=stats)
    return got


def c_oracle(tag):
    return rr.C_ORACLE_WIDE if tag in rc.WIDE_TAGS else rr.C_ORACLE


def variant_outputs(tag, name, **kw):
    """The float64 oracle's outputs of one variant of rc.VARIANTS[tag]."""
    v = dict(rc.VARIANTS[tag][name])
    if "batch_scale" in v:
        v["bs"] = v.pop("batch_scale")
    return oracle_outputs(*rc.dense_case(tag), **v, **kw)


def lower_tiles(M):
    return [(i, j) for i in range(0, M, TILE) for j in range(0, i + 1, TILE)]


@pytest.mark.parametrize("tag", sorted(rc.CASES))
def test_cases_are_dense_and_well_conditioned(refs, tag):
    """The density conditions of DESIGN 9c, on the reference itself."""
    R, S = refs[tag]["default"]
    f = refs[tag]["facts"]
    M, Q = rc.CASES[tag]["M"], rc.CASES[tag]["Q"]
    assert max(f["cond"]) <= 2 * (M + 1), f["cond"]
    assert float(R["nneg"][0]) == 0.0 and all(float(np.min(v)) > 0 for v in R["v"])
    assert f["gate_all"]                                     # no exactly-zero distance: quirk Q10's gate never drops a term
    assert all(g < 0 for g in f["gv_max"][1:]), f["gv_max"]  # every beta_n < 0 on the Poisson / Bernoulli rows (w^2 > 0)
    qd = rc.dense_latent(tag)
    H = np.abs(R["H"][qd]).astype(np.float64)
    worst = min(H[i:i + TILE, j:j + TILE].min() for i, j in lower_tiles(M)) / H.max()
    print("[rowpass] %s 100 h latent: min over lower tiles of min|H| / max|H| = %.3g, cond = %s" % (
        tag, worst, " ".join("%.0f" % c for c in f["cond"])))
    assert worst >= 1e-3
    for kind in ("H", "r", "dZ"):
        s = S[kind][qd]
        assert s.min() >= 1e-8 * s.max(), (kind, s.min(), s.max())
    for q in range(Q):
        for s in S["dKmn"][q]:
            if s is not None and s.size:
                assert np.all(s.min(axis=1) >= 1e-8 * s.max(axis=1)), (q, "a row of dL_dKmn went sparse")


@pytest.mark.parametrize("tag", sorted(rc.CASES))
def test_oracle_within_c_oracle(refs, tag):
    """The float64 oracle against R, every kind, every element: the measurement behind rowpass_ref.C_ORACLE (cases A-E with the batch-scale
    and shard variants and the strict form of D define it; F is held to the same constants) and behind C_ORACLE_WIDE (G, H, I with the
    batch-scale and strict variants of G and the shard and strict variants of H)."""
    prm, prob, X, Y, rungs = rc.dense_case(tag)
    R, S = refs[tag]["default"]
    C = c_oracle(tag)
    rr.check("oracle " + tag, oracle_outputs(prm, prob, X, Y, rungs), R, S, C, rr.KINDS)
    names = {"bs": "batch_scale", "shard": "row shard", "strict": "strict"}
    for name in ("bs", "shard", "strict"):
        if name in rc.VARIANTS.get(tag, {}):
            kinds = rr.BUNDLE_KINDS if name == "strict" else rr.KINDS
            rr.check("oracle %s %s" % (tag, names[name]), variant_outputs(tag, name), *refs[tag][name], C, kinds)


@pytest.mark.parametrize("tag", rc.STRICT2_TAGS)
def test_oracle_two_solve_form_within_c_oracle(refs, tag):
    """The float64 oracle's two-solve restatement (A = dpotrs, H = A^T diag(beta) A, r = A^T alpha in the bundle; q(f) through
    p = A m and c = rowsum((A L)^2) - rowsum(A .* K^)) against the `strict2` reference, every element of the bundle kinds and of m, v:
    B, D (also its row shard) and J within the present C_ORACLE, G and H within C_ORACLE_WIDE -- so the strict2 variants are held to
    the present C_KERNEL / C_KERNEL_WIDE and nothing is widened (the measured table is in DESIGN 9x)."""
    kinds = rr.BUNDLE_KINDS + ("m", "v")
    for name in sorted(n for n in rc.VARIANTS[tag] if n.startswith("strict2")):
        w = rr.check("oracle %s %s" % (tag, name), variant_outputs(tag, name), *refs[tag][name], c_oracle(tag), kinds)
        print("[strict2] oracle %-2s %-13s %s" % (tag, name, " ".join("%s %.3g" % (k, w[k]) for k in kinds)))


def test_constants_follow_the_rule():
    for CO, ck in ((rr.C_ORACLE, rr.c_kernel()), (rr.C_ORACLE_WIDE, rr.c_kernel_wide())):
        for k in rr.KINDS:
            c = CO[k]
            assert c >= 1 and np.log2(c) == int(np.log2(c))          # a power of two
            assert ck[k] == max(16.0, 4.0 * c)
    # the wide set only ever adds to the first: max(C_ORACLE, what G, H, I need); ve and sgv are the two kinds that moved
    assert all(rr.C_ORACLE_WIDE[k] >= rr.C_ORACLE[k] for k in rr.KINDS)
    assert {k for k in rr.KINDS if rr.C_ORACLE_WIDE[k] != rr.C_ORACLE[k]} == {"ve", "sgv"}
    assert not rr.KERNEL_EXCEPTIONS


def _swap_tile(H):
    """Tile (2, 0) of a symmetric H replaced by tile (2, 1), mirrored."""
    H = H.copy()
    H[2 * TILE:3 * TILE, 0:TILE] = H[2 * TILE:3 * TILE, TILE:2 * TILE]
    H[0:TILE, 2 * TILE:3 * TILE] = H[2 * TILE:3 * TILE, 0:TILE].T
    return H


def _transpose_tile(H):
    """Tile (2, 0) of a symmetric H written transposed (its two operand panels exchanged), mirrored."""
    H = H.copy()
    H[2 * TILE:3 * TILE, 0:TILE] = H[2 * TILE:3 * TILE, 0:TILE].T
    H[0:TILE, 2 * TILE:3 * TILE] = H[2 * TILE:3 * TILE, 0:TILE].T
    return H


def _drop_tile(H):
    """Tile (2, 0) of a symmetric H never written (left at the zero the bundle starts from), mirrored."""
    H = H.copy()
    H[2 * TILE:3 * TILE, 0:TILE] = 0.0
    H[0:TILE, 2 * TILE:3 * TILE] = 0.0
    return H


def test_criterion_rejects_indexing_corruptions(refs):
    """Seeded corruptions (five kinds; the far Gram tile in three variants) of the ORACLE's output of case D, each what an indexing error in a kernel would leave behind.  Each must
    land beyond C_KERNEL (the looser of the two constants); the ratios reached are recorded in DESIGN 9c."""
    prm, prob, X, Y, rungs = rc.dense_case("D")
    R, S = refs["D"]["default"]
    keep = {}
    clean = oracle_outputs(prm, prob, X, Y, rungs, keep=keep)
    u, rows = keep["u"], keep["rows"]
    CK = rr.c_kernel()
    q, W = 1, prm["W"]
    reached = {}

    def worst(got, kind):
        return rr.worst_ratios(got, R, S, (kind,))[kind][0]

    # 1. a far Gram tile computed from the wrong column panel
    bad = dict(clean, H=clean["H"].copy())
    bad["H"][q] = _swap_tile(clean["H"][q])
    reached["H tile (2,0) := (2,1)"] = ("H", bad)
    for what, fn in (("H tile (2,0) transposed", _transpose_tile), ("H tile (2,0) not written", _drop_tile)):
        bad = dict(clean, H=clean["H"].copy())
        bad["H"][q] = fn(clean["H"][q])
        reached[what] = ("H", bad)
    # 2. beta read one row off inside one 16-row k-step of the Gram (the Poisson task, rows 256 .. 271: beta varies from row to row)
    o = rows[1]
    beta = o["gv"] @ (W[q, 1:2] ** 2)
    k0 = 256
    shifted = beta.copy()
    shifted[k0:k0 + 16] = np.roll(beta[k0:k0 + 16], 1)
    K = o["K"][q]
    bad = dict(clean, H=clean["H"].copy())
    bad["H"][q] = clean["H"][q] + (K[k0:k0 + 16] * (shifted - beta)[k0:k0 + 16, None]).T @ K[k0:k0 + 16]
    reached["beta shifted in one k-step"] = ("H", bad)
    # 3. the last (ragged) row of task 0 dropped from the Gram and from r
    o = rows[0]
    K, n = o["K"][q], rc.CASES["D"]["Ns"][0] - 1
    alpha, beta = o["gm"] @ W[q, :1], o["gv"] @ (W[q, :1] ** 2)
    bad = dict(clean, H=clean["H"].copy(), r=clean["r"].copy())
    bad["H"][q] = clean["H"][q] - beta[n] * np.outer(K[n], K[n])
    bad["r"][q] = clean["r"][q] - alpha[n] * K[n]
    reached["last row dropped (H)"] = ("H", bad)
    reached["last row dropped (r)"] = ("r", bad)
    # 4. four adjacent columns of K^ missing from the forward of one 128-row block (task 0, rows 128 .. 255, columns 200 .. 203)
    blk = slice(128, 256)
    Kz = K[blk].copy()
    Kz[:, 200:204] = 0.0
    Pt = Kz @ u["C"][q]
    c_bad, c_ok = np.sum(Pt * K[blk], 1), np.sum(o["Pt"][q][blk] * K[blk], 1)
    bad = dict(clean, v=[a.copy() for a in clean["v"]], dKmn=[[a.copy() for a in row] for row in clean["dKmn"]])
    bad["v"][0][blk] = clean["v"][0][blk] + W[q, 0] ** 2 * (c_bad - c_ok)
    bad["dKmn"][q][0][:, blk] = u["a"][q][:, None] * o["gm"][blk, 0][None, :] + 2.0 * W[q, 0] * o["gv"][blk, 0][None, :] * Pt.T
    reached["4 columns of K^ zeroed (v)"] = ("v", bad)
    reached["4 columns of K^ zeroed (dKmn)"] = ("dKmn", bad)
    # 5. dZ of two adjacent inducing points exchanged
    bad = dict(clean, dZ=clean["dZ"].copy())
    bad["dZ"][q, [200, 201]] = clean["dZ"][q, [201, 200]]
    reached["dZ columns exchanged"] = ("dZ", bad)
    for what, (kind, got) in reached.items():
        ratio = worst(got, kind)
        print("[rowpass] corruption %-32s %-5s ratio %.3g (C_KERNEL = %g)" % (what, kind, ratio, CK[kind]))
        assert ratio > CK[kind], (what, ratio)
        with pytest.raises(AssertionError):
            rr.check("corrupted: " + what, got, R, S, CK, (kind,))
    rr.check("uncorrupted D", clean, R, S, CK, rr.KINDS)


def test_criterion_rejects_two_solve_corruptions(refs):
    """Seeded corruptions of the ORACLE's own two-solve output of case D (arithmetic on arrays: nothing is run wrongly), each what an
    indexing error in the two-solve code of the strict mode would leave behind.  Each must land beyond C_KERNEL by a factor 2^10 at
    least; the ratios reached are recorded in DESIGN 9x."""
    import scipy.linalg
    from oracle import likelihoods_oracle as lo
    prm, prob, X, Y, rungs = rc.dense_case("D")
    R, S = refs["D"]["strict2"]
    keep = {}
    clean = oracle_outputs(prm, prob, X, Y, rungs, strict="two", keep=keep)
    u, rows = keep["u"], keep["rows"]
    CK, W, kap, Q, M = rr.c_kernel(), prm["W"], prm["kappa"], prob["Q"], prob["M"]
    reached = []

    def weights(o, q, gm=None, gv=None):
        ds = [d for d in range(prob["Df"]) if prob["f_index"][d] == o["t"]]
        gm, gv = (o["gm"] if gm is None else gm), (o["gv"] if gv is None else gv)
        return gm @ W[q, ds], gv @ (W[q, ds] ** 2)

    # 1. p_q = A_q m_u formed with the m_u of latent 1 - q: m directly, H through the row weights at the wrong m (v does not depend
    #    on p: it cannot move and is asserted unchanged)
    bad = dict(clean, m=[a.copy() for a in clean["m"]], H=np.zeros_like(clean["H"]))
    for o in rows:
        ds = [d for d in range(prob["Df"]) if prob["f_index"][d] == o["t"]]
        mu = np.zeros_like(o["m"])
        for j, d in enumerate(ds):
            for q in range(Q):
                mu[:, j] += W[q, d] * (o["Kg"][q] @ prm["m_u"][:, 1 - q])
            bad["m"][d] = mu[:, j]
        name, kw = prob["specs"][o["t"]]
        _, gm, gv = lo.var_exp_all(name, Y[o["t"]], mu, o["v"], exact=False, **kw)
        for q in range(Q):
            _, beta = weights(o, q, gm, gv)
            bad["H"][q] += (o["Kg"][q] * beta[:, None]).T @ o["Kg"][q]
    reached += [("p_q from m_u of latent 1 - q", k, bad) for k in ("m", "H")]
    assert rr.worst_ratios(bad, R, S, ("v",))["v"][0] == rr.worst_ratios(clean, R, S, ("v",))["v"][0]
    # 2. columns 128 .. 255 of A without the backward update from columns 256 .. 383 (the backward half solves A Luu = X from the last
    #    column block to the first: A_1 = (X_1 - A_2 Luu[2,1]) Luu[1,1]^-1): A_1 keeps A_2 Luu[2,1] Luu[1,1]^-1, A_0 is formed from that A_1
    q = 1
    Lu = u["Luu"][q]
    b0, b1, b2 = slice(0, 128), slice(128, 256), slice(256, 384)
    bad = dict(clean, H=clean["H"].copy(), r=clean["r"].copy())
    bad["H"][q], bad["r"][q] = 0.0, 0.0
    for o in rows:
        A = o["Kg"][q].copy()
        d1 = scipy.linalg.solve_triangular(Lu[b1, b1], (A[:, b2] @ Lu[b2, b1]).T, lower=True, trans="T").T
        A[:, b1] += d1
        A[:, b0] -= scipy.linalg.solve_triangular(Lu[b0, b0], (d1 @ Lu[b1, b0]).T, lower=True, trans="T").T
        alpha, beta = weights(o, q)
        bad["H"][q] += (A * beta[:, None]).T @ A
        bad["r"][q] += A.T @ alpha
    reached += [("A[:, 128:256] misses the update from 256:384", k, bad) for k in ("H", "r")]
    # 3. rowsum(A .* K^) with K^ one row off inside one 16-row group (task 0, rows 256 .. 271)
    o, k0 = rows[0], 256
    A, K = o["Kg"][q][k0:k0 + 16], o["K"][q][k0:k0 + 16]
    bad = dict(clean, v=[a.copy() for a in clean["v"]])
    bad["v"][0][k0:k0 + 16] -= W[q, 0] ** 2 * (np.sum(A * np.roll(K, 1, axis=0), 1) - np.sum(A * K, 1))
    reached.append(("rowsum(A .* K^): K^ one row off in a 16-row group", "v", bad))
    for what, kind, got in reached:
        ratio = rr.worst_ratios(got, R, S, (kind,))[kind][0]
        print("[strict2] corruption %-46s %-3s ratio %.3g (C_KERNEL = %g, x 2^10 = %g)" % (what, kind, ratio, CK[kind], 1024 * CK[kind]))
        assert ratio > 1024 * CK[kind], (what, kind, ratio)
    rr.check("uncorrupted D strict2", clean, R, S, CK, rr.BUNDLE_KINDS + ("m", "v"))


def test_case_K_takes_the_two_solve_form_by_itself(refs):
    """Case K as committed: the condition estimate variance max diag(K_uu^-1) is >= 2e6 on latent 0 and <= 1e3 on latent 1, so
    the strict mode picks the two-solve form with no switch set; float64 Cholesky of the unjittered K_uu succeeds; the neighbour at
    1 h on the same data stays one-solve.  Closeness to R is conditioning-limited here: the float64 two-solve oracle's array-norm distances
    from R are measured, printed and held against rc.K_ORACLE_DIST (and never 16 x below it: the record cannot go stale-loose)."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y, rungs = rc.auto_case()
    u = so.u_algebra(prm, dict(prob, strict_qf=True), rungs)
    est = [float(prm["variance"][q] * np.max(np.diag(u["Kuui"][q]))) for q in range(prob["Q"])]
    cond = float(np.linalg.cond(u["Kuu"][0]))
    print("[strict2] K estimate %s cond(K_uu) of latent 0 %.3g rungs %s (lengthscale / h = %g)" % (
        " ".join("%.3g" % x for x in est), cond, u["rungs"], rc.K_CS))
    assert est[0] >= 2e6 and est[1] <= 1e3 and u["strict_two"] and list(u["rungs"]) == rc.K_RUNGS
    np.linalg.cholesky(u["Kuu"][0])
    near = rc.auto_case(cs0=1.0)
    assert not so.u_algebra(near[0], dict(prob, strict_qf=True), rungs)["strict_two"]
    R, S = refs["K"]["two"]
    assert float(R["nneg"][0]) == 0.0
    got = oracle_outputs(prm, prob, X, Y, rungs, strict="two")
    dist = rc.array_distances(got, R)
    for k in rc.K_KINDS:
        print("[strict2] K oracle %-4s max|oracle - R| / max|R| = %.3g (recorded %.2g)" % (k, dist[k], rc.K_ORACLE_DIST[k]))
    # the two forms' H are different matrices: the reference of one cannot pass for the other
    split = rc.array_distances(dict(H=np.asarray(R["H"], dtype=np.float64)), refs["K"]["one"][0], ("H",))["H"]
    print("[strict2] K max|A^T b A - X^T b X| / max|X^T b X| = %.3g" % split)
    assert split > 0.5
    for k in rc.K_KINDS:
        assert rc.K_ORACLE_DIST[k] / 16 <= dist[k] <= rc.K_ORACLE_DIST[k], (k, dist[k], rc.K_ORACLE_DIST[k])


def test_criterion_rejects_stride_corruptions_at_3d_4d_inputs_and_eight_latents(refs):
    """Seeded corruptions of the ORACLE's output of cases G, H (row shard) and I, each what a wrong stride in P or Q would leave behind
    (arithmetic on arrays: nothing is run wrongly).  Each must land beyond C_KERNEL_WIDE; the ratios reached are recorded in DESIGN 9c."""
    CK = rr.c_kernel_wide()
    reached = []

    # 1. case H, row shard: task 0's rows read at row_begin * 1 doubles where row_begin * 4 is meant -- its K^-dependent outputs formed
    #    again from the 264 x 4 doubles that start 37 doubles into X_0
    prm, prob, X, Y, rungs = rc.dense_case("H")
    b, e = rc.H_SHARD
    Xbad = [x.copy() for x in X]
    Xbad[0][b[0]:e[0]] = X[0].reshape(-1)[b[0]:b[0] + 4 * (e[0] - b[0])].reshape(e[0] - b[0], 4)
    bad = oracle_outputs(prm, prob, Xbad, Y, rungs, row_begin=b, row_end=e)
    for kind in ("r", "dZ", "m"):
        reached.append(("H shard: X_0 offset row_begin * 1", "H", "shard", kind, bad))
    # 2. case G: the p = 1 and p = 2 components of dZ exchanged for one inducing point
    clean = oracle_outputs(*rc.dense_case("G"))
    bad = dict(clean, dZ=clean["dZ"].copy())
    bad["dZ"][1, 100, [1, 2]] = clean["dZ"][1, 100, [2, 1]]
    reached.append(("G: dZ components p = 1, 2 exchanged", "G", "default", "dZ", bad))
    # 3. case I: the bundle blocks of latents 6 and 7 exchanged
    prm, prob, X, Y, rungs = rc.dense_case("I")
    keep = {}
    clean = oracle_outputs(prm, prob, X, Y, rungs, keep=keep)
    bad = dict(clean)
    for k in ("H", "r", "dZ", "sa", "sl", "swk"):
        bad[k] = clean[k].copy()
        bad[k][[6, 7]] = clean[k][[7, 6]]
    for kind in ("H", "r"):
        reached.append(("I: bundle blocks q = 6, 7 exchanged", "I", "default", kind, bad))
    # 4. case I: the quadrature mixes p_q, c_q of the first three latents only
    u, W, kap = keep["u"], prm["W"], prm["kappa"]
    bad = dict(clean, m=[a.copy() for a in clean["m"]], v=[a.copy() for a in clean["v"]])
    for o in keep["rows"]:
        t = o["t"]
        for d in (d for d in range(prob["Df"]) if prob["f_index"][d] == t):
            for q in range(3, prob["Q"]):
                p_q, c_q = o["K"][q] @ u["a"][q], np.sum(o["Pt"][q] * o["K"][q], 1)
                bad["m"][d] -= W[q, d] * p_q
                bad["v"][d] -= (W[q, d] ** 2 + kap[q, d]) * prm["variance"][q] + W[q, d] ** 2 * c_q
    for kind in ("m", "v"):
        reached.append(("I: quadrature over q < 3 only", "I", "default", kind, bad))
    for what, tag, variant, kind, got in reached:
        R, S = refs[tag][variant]
        ratio = rr.worst_ratios(got, R, S, (kind,))[kind][0]
        print("[rowpass] corruption %-36s %-5s ratio %.3g (C_KERNEL_WIDE = %g)" % (what, kind, ratio, CK[kind]))
        assert ratio > CK[kind], (what, ratio)
        with pytest.raises(AssertionError):
            rr.check("corrupted: " + what, got, R, S, CK, (kind,))


def test_array_maximum_yardstick_accepts_far_tile_corruptions_on_the_banded_case():
    """The gap this file closes, on the EXISTING style of case (lengthscale about one inducing spacing) at case D's shape: Gram tile
    (2, 0) of the second latent written transposed, or not written at all, passes `max|a - b| / max|b| < 1e-8` -- on H itself and on
    the ELBO and every gradient computed from it; the same two corruptions of the dense case are rejected above.
    The corruption first proposed for this assertion, tile (2, 0) := tile (2, 1), does NOT pass the old yardstick (0.34 on H): tile
    (2, 1) is a first sub-diagonal tile and holds O(1) elements next to its corner on the banded case too.  That is asserted as
    well, so that the record is what was measured."""
    from oracle import svmogp_oracle as so
    prm, prob, X, Y = rc.banded_case()
    u = so.u_algebra(prm, prob)
    stats, _ = so.local_stats(prm, prob, u, X, Y)
    lay, M = so.stats_layout(prob), prob["M"]
    o = lay["NG"] + lay["per_q"]
    H = stats[o:o + M * M].reshape(M, M).copy()
    want = so.finish(prm, prob, u, stats)
    frac = np.mean(np.abs(H) < 1e-12 * np.abs(H).max())
    print("[rowpass] banded M = 384: %.0f %% of H_1 below 1e-12 max|H|" % (100 * frac))
    assert frac > 0.8
    for what, fn in (("transposed", _transpose_tile), ("not written", _drop_tile)):
        bad = stats.copy()
        bad[o:o + M * M] = fn(H).reshape(-1)
        # (the far tile of the banded case is so small -- exactly 0.0 where exp underflows -- that the corrupted bundle may be the same bits)
        worst = rel_norm(bad[o:o + M * M], H.reshape(-1))
        out = so.finish(prm, prob, u, bad)
        for k in ("elbo", "g_m_u", "g_L_u", "g_variance", "g_lengthscale", "g_W", "g_kappa", "g_Z"):
            worst = max(worst, rel_norm(out[k], want[k]))
        print("[rowpass] banded M = 384: tile (2,0) %s: largest max|a - b| / max|b| over H and the outputs = %.3g" % (what, worst))
        assert worst < 1e-8, what
    literal = rel_norm(_swap_tile(H).reshape(-1), H.reshape(-1))
    print("[rowpass] banded M = 384: tile (2,0) := (2,1): max|a - b| / max|b| on H = %.3g" % literal)
    assert literal > 1e-8
