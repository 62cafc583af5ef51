"""GPU: the M x M side and the strict-mode solves element by element -- `jitchol_inv`, `potri` and `potrs_rows`, called
through the C ABI on the cases of tests/linalg_cases.py, every element of every output held to

    |quantity| <= C_KERNEL[kind] * 2^-52 * max(S, 2^-1022)

with the residual / forward-error quantities and scales of tests/linalg_ref.py (formed in np.longdouble from the kernels' float64
output) and C_KERNEL = max(16, 4 * C_ORACLE) from the plain float64 algorithms (tests/test_linalg_ref_cpu.py).  No exception list.
Every kernel runs twice and has to return identical bits (the chains have a fixed order).  All kernels run first, then ONE pool of at
most 16 processes forms all longdouble residuals (the host work: about 3 M^3 longdouble multiply-adds per latent).

Which kernels each case reaches (launch_potrf_batched / launch_trtri_batched / potrs_rows_inplace, restated in linalg_cases.py and
asserted on the host in tests/test_linalg_ref_cpu.py):

  jitchol_inv   M    Q  potrf                                  trtri (64 x 64 diagonal blocks, merges at s = 64, 128, ...)
                31   2  one ragged panel, no trailing tile     one ragged block, no merge
                32   2  one full panel                          one ragged block
                33   2  panel + 1-row 64-tile + look-ahead     one ragged block
                64   2  two panels, 64-tiles                   one full block, no merge
                65   2  64-tiles, ragged                       s = 64 merge with a right block of 1 (M_last = K_last = 1)
                129  2  64-tiles                               s = 64 full merge, s = 128 merge with M_last = K_last = 1
                200  2  64-tiles, ragged panel (8 columns)     ragged block (8), s = 64: 2 pairs, last right block 8; s = 128: 72
                320  2  64-tiles                               5 blocks: s = 64 merges 2 pairs + 1 single; s = 128, 256: right 64
                576  2  64-tiles (T64 = 9: 45 * 2 <= 512)      s = 128 level with a ragged last 128 (9 blocks)
                704  8  FIRST panel 128-tiles (rem = 672: T64 = 11, 66 * 8 = 528 > 512; 6 tiles per edge, the last 32 wide), every
                        later panel 64-tiles (rem = 640: 440): both variants in one factorisation; W, R, G matrices and three
                        different forced rungs (-1, 0, and 1 on latent 5 alone) across the batch
                768  8  three 128-tile panels (rem = 736, 704, 672), then 64-tiles; same batch mix
  potri         33 ... 576, Q = 2: the trtri paths above on graded factors (L), then ltl
  potrs_rows    (33, 1) (100, 333) (160, 1023) (257, 130): the round-5 path (trsm_diag + GEMM updates; ragged M or n < 1024)
                (128, 1024) (256, 1025) (384, 1153) (512, 2049): trsm_panel_kernel<DIR, 0>, both directions (M % 128 == 0, n >= 1024,
                ragged last row tile of 1); the first 333 rows of each, solved on their own, take the round-5 path again"""
import numpy as np
import pytest

import linalg_cases as lc
import linalg_ref as lf

pytestmark = pytest.mark.gpu

_PINNED = {}


def _solve_groups():
    g = {}
    for t, c in lc.SOLVE.items():
        g.setdefault((c["M"], c["n"], c["mat"]), []).append(t)
    return g


@pytest.fixture(scope="module")
def pinned():
    """{key: ({kind or tag: worst}, facts)} plus {("bits", ...): bool} and {("rungs", tag): list}: every kernel call of this file, each
    made twice, then all residuals in one pool."""
    if _PINNED:
        return _PINNED
    from hetmogp_amd import engine as E
    jobs = []
    for tag in lc.JITCHOL:
        c = lc.jitchol_case(tag)
        L, Ai, rungs = E.jitchol_inv(c["A"], forced_rung=c["rungs"])
        L2, Ai2, _ = E.jitchol_inv(c["A"], forced_rung=c["rungs"])
        _PINNED[("bits", "jitchol", tag)] = bool(np.array_equal(L, L2) and np.array_equal(Ai, Ai2))
        _PINNED[("rungs", tag)] = rungs
        for q, u in enumerate(c["lat"]):
            jobs.append(dict(what="jitchol", key=("jitchol", tag, q), A=u["A"], jitter=u["jitter"], L=L[q], Ainv=Ai[q]))
    for tag in lc.POTRI:
        c = lc.potri_case(tag)
        S = E.potri(c["L"])
        _PINNED[("bits", "potri", tag)] = bool(np.array_equal(S, E.potri(c["L"])))
        for q, u in enumerate(c["lat"]):
            jobs.append(dict(what="potri", key=("potri", tag, q), L=u["L"], Sinv=S[q]))
    for (M, n, mat), tags in _solve_groups().items():
        L = lc.solve_factor(M, mat)["L"]
        pairs = {}
        for t in tags:
            B = lc.solve_case(t)["B"]
            X = E.potrs_rows(L, B)
            _PINNED[("bits", "solve", t)] = bool(np.array_equal(X, E.potrs_rows(L, B)))
            pairs[t] = (B, X)
            if t in lc.SOLVE_SUBSET:
                Bs = np.ascontiguousarray(B[:lc.SUBSET_ROWS])
                pairs[t + "/first"] = (Bs, E.potrs_rows(L, Bs))
        jobs.append(dict(what="solve", key=("solve", M, n, mat), L=L, pairs=pairs))
    _PINNED.update(lc.run_jobs(jobs))
    return _PINNED


def _jitchol_kinds(pinned, tag, kinds):
    c = lc.jitchol_case(tag)
    C = lf.c_kernel()
    bad = []
    for q, u in enumerate(c["lat"]):
        w, facts = pinned[("jitchol", tag, q)]
        assert facts["floor_ok"], (tag, q, "an element of S below 2^-1022 (chol: inside the band)")
        assert set(w) == {"chol", "chol_upper", "kinv"}
        for k in kinds:
            lf.report("kernel  %s q%d %s" % (tag, q, u["kind"]), k, w[k], C[k])
            if not w[k][0] <= C[k]:
                bad.append((q, u["kind"], k, w[k][0], C[k]))
    assert not bad, (tag, "beyond C_KERNEL", bad)


@pytest.mark.parametrize("tag", list(lc.JITCHOL))
def test_jitchol_inv_factor_pinned(pinned, tag):
    """chol: A + jitter I - L^ L^T on the lower triangle; chol_upper: the strictly upper triangle of L^ is exactly 0.0 (the
    out-of-place factor parks reciprocal pivots there, potrf_finalize_kernel clears them).  Per latent, so that neither the batch
    strides nor another latent's jitter can leak; the forced rungs come back as given and two calls return the same bits (factor and
    inverse).  Measured 2026-10-19 on an MI355X: worst chol 15 (M = 576, W) against C_KERNEL = 16; R and G at most 7.8."""
    c = lc.jitchol_case(tag)
    for q, u in enumerate(c["lat"]):
        lc.assert_latent_conditions(tag, q, u)
    assert pinned[("rungs", tag)] == c["rungs"]
    assert pinned[("bits", "jitchol", tag)], "two calls differ"
    _jitchol_kinds(pinned, tag, ("chol", "chol_upper"))


@pytest.mark.parametrize("tag", list(lc.JITCHOL))
def test_jitchol_inv_inverse_pinned(pinned, tag):
    """kinv: Ainv against Linv^T Linv of the kernel's own L^ (longdouble inverse of the float64 factor).

    This test found a defect.  Before the fix, measured 2026-10-19 on an MI355X (C_KERNEL = 16; W latents at most 3.5):
        M = 129 G 34    M = 200 R 38    M = 320 R, G 290    M = 576 G 290    M = 704 / 768 R, G 290, R8 103     (M <= 65: <= 0.98)
    `launch_trtri_batched` merged X21 = -X22 (L21 X11) by two GEMMs with the COMPUTED inverse X22; that product's error is
    gamma |X22| |L21 X11|, not bounded by |Linv| |L| |Linv| when X22 (L21 X11) cancels, as it does for the factor of an RBF K_uu at
    cond 1e7 (a float64 NumPy restatement of the same merges: 11 / 16 / 107 / 287 at M = 129 / 200 / 320 / 576).  The merge now ends
    with one step of refinement in working precision, X21 -= X22 (L21 X11 + L22 X21), whose error |X22| times
    gamma (|L21| |X11| + |L22| |X21|) is the componentwise bound itself (restatement: 0.20 / 0.19 / 0.29 / 0.14; kernel figures in
    DESIGN 9f)."""
    _jitchol_kinds(pinned, tag, ("kinv",))


@pytest.mark.parametrize("tag", list(lc.POTRI))
def test_potri_pinned(pinned, tag):
    """sinv: potri(L) against Linv^T Linv of the longdouble triangular inverse of the given graded factor: trtri_diag_kernel, its
    doubling GEMM merges and ltl, judged by the forward-error bound of the triangular inverse carried through the product."""
    c = lc.potri_case(tag)
    C = lf.c_kernel()
    for q, u in enumerate(c["lat"]):
        lc.assert_l_conditions(tag, q, u)
    assert pinned[("bits", "potri", tag)], "two calls differ"
    for q in range(c["Q"]):
        w, facts = pinned[("potri", tag, q)]
        assert facts["floor_ok"], (tag, q)
        lf.check("kernel  %s q%d L" % (tag, q), w, C)


def _solve_worst(pinned, tag, name):
    c = lc.SOLVE[tag]
    w, facts = pinned[("solve", c["M"], c["n"], c["mat"])]
    assert facts["floor_ok"], (tag, "an element of S below 2^-1022")
    return {"solve": w[name]}


@pytest.mark.parametrize("tag", list(lc.SOLVE))
def test_potrs_rows_pinned(pinned, tag):
    """solve: the row-wise residual X^ (L L^T) - B of the composed two-direction solve against |X^| |L| |L^T|, every row at its own
    scale: right-hand sides (a) random, (b) rows of K_uf, (c) random rows times 2^e, e in [-20, 20]."""
    lc.assert_solve_conditions(tag, lc.solve_case(tag))
    assert pinned[("bits", "solve", tag)], "two calls differ"
    lf.check("kernel  " + tag, _solve_worst(pinned, tag, tag), lf.c_kernel())


@pytest.mark.parametrize("tag", lc.SOLVE_SUBSET)
def test_potrs_rows_first_rows_of_a_panel_case_pinned(pinned, tag):
    """The first 333 rows of a panel-path case, solved on their own by the round-5 kernels: two valid blocked substitutions of the
    same rows, each held to the reference instead of to the other."""
    c = lc.SOLVE[tag]
    assert lc.solve_path(c["M"], c["n"]) == "panel" and lc.solve_path(c["M"], lc.SUBSET_ROWS) == "round-5"
    lf.check("kernel  " + tag + " first %d rows" % lc.SUBSET_ROWS, _solve_worst(pinned, tag, tag + "/first"), lf.c_kernel())
