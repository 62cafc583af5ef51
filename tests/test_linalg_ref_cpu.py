"""CPU: the element-by-element criterion of the M x M side (tests/linalg_ref.py) before any kernel is held to it.
  (a) every case of tests/linalg_cases.py meets its conditions (condition number within its decade, grading >= 2^20), and the launcher's
      own formula, restated, sends the Q = 8 cases through potrf_step_kernel<128>;
  (b) the plain float64 algorithms (column Cholesky, row-by-row triangular inverse, X^T X, forward then backward substitution) sit
      within C_ORACLE on every case with M <= 384 -- the measurement C_ORACLE was taken from -- and LAPACK, printed beside them, within
      C_KERNEL on the W and R cases (another order of summation; under grading dpotrf is not componentwise tight and is only printed);
  (c) the criterion is sharp: eight seeded corruptions of the plain algorithms' own output (arithmetic on arrays: nothing is run
      wrongly) land far beyond C_KERNEL, while the array-maximum yardsticks of the existing tests accept three of them."""
import numpy as np
import pytest
import scipy.linalg as sl
from scipy.linalg import lapack

import linalg_cases as lc
import linalg_ref as lf
from conftest import rel_norm

M_MAX = 384        # C_ORACLE is taken over the cases up to here
MARGIN = 2.0 ** 20


def _jitchol_tags():
    return [t for t in lc.JITCHOL if lc.JITCHOL[t]["M"] <= M_MAX]


def _potri_tags():
    return [t for t in lc.POTRI if lc.POTRI[t]["M"] <= M_MAX]


def _solve_groups():
    g = {}
    for t, c in lc.SOLVE.items():
        if c["M"] <= M_MAX:
            g.setdefault((c["M"], c["n"], c["mat"]), []).append(t)
    return g


def _with_jitter(u):
    return u["A"] + u["jitter"] * np.eye(u["A"].shape[0])


def _lapack_inverse(L):
    S, info = lapack.dpotri(np.tril(L), lower=1)
    assert info == 0
    return np.tril(S) + np.tril(S, -1).T


@pytest.fixture(scope="module")
def measured():
    """{(who, entry point, tag[, q]): ({kind: worst}, facts)} for who = "plain" (the float64 restatement) and "lapack"."""
    jobs = []
    for tag in _jitchol_tags():
        c = lc.jitchol_case(tag)
        for q, u in enumerate(c["lat"]):
            Aj = _with_jitter(u)
            Lp = lf.cholesky_f64(Aj)
            Xp = lf.tri_inverse_f64(Lp)
            jobs.append(dict(what="jitchol", key=("plain", "jitchol", tag, q), A=u["A"], jitter=u["jitter"], L=Lp, Ainv=Xp.T @ Xp))
            Ll = sl.cholesky(Aj, lower=True)
            jobs.append(dict(what="jitchol", key=("lapack", "jitchol", tag, q), A=u["A"], jitter=u["jitter"], L=Ll, Ainv=_lapack_inverse(Ll)))
    for tag in _potri_tags():
        c = lc.potri_case(tag)
        for q, u in enumerate(c["lat"]):
            Xp = lf.tri_inverse_f64(u["L"])
            jobs.append(dict(what="potri", key=("plain", "potri", tag, q), L=u["L"], Sinv=Xp.T @ Xp))
            jobs.append(dict(what="potri", key=("lapack", "potri", tag, q), L=u["L"], Sinv=_lapack_inverse(u["L"])))
    for (M, n, mat), tags in _solve_groups().items():
        L = lc.solve_factor(M, mat)["L"]
        cs = {t: lc.solve_case(t) for t in tags}
        jobs.append(dict(what="solve", key=("plain", "solve", M, n, mat), L=L, pairs={t: (c["B"], lf.solve_f64(L, c["B"])) for t, c in cs.items()}))
        jobs.append(dict(what="solve", key=("lapack", "solve", M, n, mat), L=L,
                         pairs={t: (c["B"], sl.cho_solve((L, True), c["B"].T).T) for t, c in cs.items()}))
    return lc.run_jobs(jobs)


# ================================================================================================ (a) the cases
@pytest.mark.parametrize("tag", sorted(lc.JITCHOL))
def test_jitchol_case_conditions(tag):
    c = lc.jitchol_case(tag)
    conds = [lc.assert_latent_conditions(tag, q, u) for q, u in enumerate(c["lat"])]
    print("[linalg] jitchol %s kinds %s rungs %s cond %s" % (tag, lc.JITCHOL[tag]["kinds"], c["rungs"], " ".join("%.3g" % x for x in conds)))
    if c["Q"] == 8:
        assert len(set(c["rungs"])) == 3 and c["rungs"].count(1) == 1        # one latent on a rung of its own
        assert {"W", "R", "G"} <= set(lc.JITCHOL[tag]["kinds"])


@pytest.mark.parametrize("tag", sorted(lc.POTRI))
def test_potri_case_conditions(tag):
    c = lc.potri_case(tag)
    for q, u in enumerate(c["lat"]):
        lc.assert_l_conditions(tag, q, u)
        assert np.all(np.triu(u["L"], 1) == 0)


@pytest.mark.parametrize("tag", sorted(lc.SOLVE))
def test_solve_case_conditions(tag):
    c = lc.solve_case(tag)
    lc.assert_solve_conditions(tag, c)
    assert c["B"].shape == (c["n"], c["M"]) and np.all(np.triu(c["L"], 1) == 0)


def test_q8_cases_reach_the_128_tile_potrf():
    """launch_potrf_batched, restated: panel j has rem = M - j - min(32, M - j) rows below it, T64 = ceil(rem / 64), and takes
    potrf_step_kernel<64> while T64 (T64 + 1) / 2 * Q <= 512, else potrf_step_kernel<128>.
      M = 704, Q = 8: rem = 672 -> T64 = 11, 66 * 8 = 528 > 512: 128-tiles (6 tiles per edge, the last 32 wide); rem = 640 -> 440: 64.
      M = 768, Q = 8: rem = 736, 704, 672 -> 624, 528, 528: three 128-tile panels, then 64-tiles.
      every Q = 2 case: 64-tiles throughout (M = 576: T64 = 9, 45 * 2 = 90)."""
    t704, t768 = lc.potrf_tiles(704, 8), lc.potrf_tiles(768, 8)
    assert t704[0] == 128 and t704[1:] == [64] * (len(t704) - 1) and (704 - 32) % 128 == 32
    assert t768[:3] == [128] * 3 and t768[3:] == [64] * (len(t768) - 3)
    for tag, c in lc.JITCHOL.items():
        tiles = lc.potrf_tiles(c["M"], c["Q"])
        assert (128 in tiles) == (c["Q"] == 8), (tag, tiles)


def test_solve_shapes_reach_both_paths():
    assert sorted(set(c["path"] for c in lc.SOLVE.values())) == ["panel", "round-5"]
    for M, n, path in lc.SOLVE_SHAPES:
        assert lc.solve_path(M, n) == path
        if path == "panel":
            assert lc.solve_path(M, lc.SUBSET_ROWS) == "round-5"       # the 333-row slice of a panel case takes the other kernels


# ================================================================================================ (b) the constants
def _collect(measured, who, entry):
    """[(label, case kind or None, {kind: worst}, facts)] of one entry point."""
    out = []
    for key, (w, facts) in sorted(measured.items(), key=lambda kv: str(kv[0])):
        if key[0] != who or key[1] != entry:
            continue
        if entry == "jitchol":
            out.append(("%s q%d %s" % (key[2], key[3], lc.JITCHOL[key[2]]["kinds"][key[3]]), lc.JITCHOL[key[2]]["kinds"][key[3]], w, facts))
        elif entry == "potri":
            out.append(("%s q%d L" % (key[2], key[3]), "L", w, facts))
        else:
            for t, x in w.items():
                out.append((t, lc.SOLVE[t]["mat"] + lc.SOLVE[t]["rhs"], {"solve": x}, facts))
    return out


@pytest.mark.parametrize("entry", ["jitchol", "potri", "solve"])
def test_plain_float64_within_c_oracle_and_lapack_beside(measured, entry):
    """The measurement behind C_ORACLE, re-taken: every case with M <= 384, every element; the constant is the measured maximum
    rounded up to a power of two (printed beside it)."""
    Co, Ck = lf.C_ORACLE, lf.c_kernel()
    top = {}
    for label, _, w, facts in _collect(measured, "plain", entry):
        assert facts["floor_ok"], (label, "an element of S below 2^-1022")
        for k, r in lf.check("plain   " + label, w, Co).items():
            top[k] = max(top.get(k, 0.0), r)
    for k, r in top.items():
        print("[linalg] plain float64, %s: worst %s = %.4g -> C_ORACLE %g" % (entry, k, r, lf.next_pow2(r)))
        assert r <= Co[k], (k, r, Co[k])
    for label, mk, w, facts in _collect(measured, "lapack", entry):
        for k, x in w.items():
            lf.report("lapack  " + label, k, x, Ck[k])
        if not mk.startswith("G") and mk != "L":           # graded inputs: printed only
            assert all(x[0] <= Ck[k] for k, x in w.items()), (label, w)


# ================================================================================================ (c) sharpness
def _chol_worst(u, Lhat, kind="chol"):
    return lf.worst(*lf.chol_terms(u["A"], u["jitter"], Lhat)[kind])[0]


def _beyond(name, ratio, C, margin=MARGIN):
    print("[linalg] corruption %-58s ratio %.4g = %.3g x C_KERNEL (needs %.3g x)" % (name, ratio, ratio / C, margin))
    assert ratio >= C * margin, (name, ratio, C * margin)


@pytest.fixture(scope="module")
def chol320():
    c = lc.jitchol_case("M320")
    assert lc.JITCHOL["M320"]["kinds"] == ["R", "G"]
    return [(u, lf.cholesky_f64(_with_jitter(u))) for u in c["lat"]]


def test_corruption_1_tile_misses_a_rank32_update(chol320):
    """The strictly-lower 64 x 64 tile (rows 128..191, columns 64..127) of L^ never received the update of panel 32..63: its
    right-hand side is too large by L[128:192, 32:64] L[64:128, 32:64]^T, and the tile by that times L[64:128, 64:128]^-T.  (A tile
    further from the diagonal would do nothing here: at 4 h both factors are exactly 0.0 beyond 155 columns.)  On the graded
    matrix the yardstick of test_potrf_potri_vs_lapack, max|L - L_lapack| / max|L|, does not move by one bit: 2.6e-11 with the
    tile corrupted and without (measured 2026-10-19).  Its threshold of 1e-12 is not the point of comparison at this conditioning
    -- two correct factors of a matrix with cond 1e7 differ by more than that, which is why that test factors cond-5 matrices --
    so the half asserted here is that the yardstick cannot tell the two factors apart."""
    C = lf.c_kernel()["chol"]
    for u, L in chol320:
        Lc = L.copy()
        dW = L[128:192, 32:64] @ L[64:128, 32:64].T
        Lc[128:192, 64:128] += sl.solve_triangular(L[64:128, 64:128], dW.T, lower=True).T
        assert _chol_worst(u, L) <= lf.C_ORACLE["chol"]
        _beyond("1 (%s) tile misses a rank-32 update" % u["kind"], _chol_worst(u, Lc), C)
        if u["kind"] == "G":
            Ll = sl.cholesky(_with_jitter(u), lower=True)
            clean, old = rel_norm(L, Ll), rel_norm(Lc, Ll)
            print("[linalg] corruption 1 (G): max|L - L_lapack| / max|L| = %.3g corrupted, %.3g clean (threshold 1e-12)" % (old, clean))
            assert old == clean and clean < 1e-9


def test_corruption_2_unrefined_pivots(chol320):
    """The 32 pivots of the diagonal block at 64 are relatively off by 2^-40 and their columns with them (piv = d y and the column
    a y share the reciprocal square root y).  Every term of A - L^ L^T from those columns is then off by 2^-39 of itself, so the
    ratio cannot exceed 2^13 times the block's share of S: the 2^20 margin over C_KERNEL asked of the other corruptions is out of
    reach for a slip of this size whatever the matrix.  Asserted instead: the ratio reaches 2^12 -- at a row whose
    reduction lies mostly inside the block the share is above a half -- which is 2^8 times C_KERNEL."""
    C = lf.c_kernel()["chol"]
    for u, L in chol320:
        Lc = L.copy()
        Lc[:, 64:96] *= 1.0 + 2.0 ** -40
        _beyond("2 (%s) pivots of one block off by 2^-40" % u["kind"], _chol_worst(u, Lc), C, margin=2.0 ** 12 / C)


def test_corruption_3_reciprocal_pivot_left_above_the_diagonal(chol320):
    u, L = chol320[0]
    assert _chol_worst(u, L, "chol_upper") == 0.0
    Lc = L.copy()
    Lc[70, 71] = 1.0 / L[70, 70]
    assert _chol_worst(u, Lc) == _chol_worst(u, L)                 # (the lower triangle does not see it)
    _beyond("3 reciprocal pivot parked at (70, 71)", _chol_worst(u, Lc, "chol_upper"), lf.c_kernel()["chol_upper"])


def _sinv_worst(L, S):
    return lf.worst(*lf.inv_terms(L, S))[0]


def test_corruption_4_block_of_linv_transposed():
    """The off-diagonal block (rows 64..127, columns 0..63) of Linv is transposed before Linv^T Linv, on the graded factor of M = 200.
    The yardstick of test_potrf_potri_vs_lapack, max|Sinv - inv(L L^T)| / max|inv| < 1e-9, catches this one too (3.9e-3, measured
    2026-10-19: the block holds elements next to the diagonal, which are among the largest of Linv), so its figure is printed and
    only asserted to be what it is: caught.  The array maximum stays blind to the smaller elements all the same (corruption 8)."""
    u = lc.potri_case("M200")["lat"][0]
    X = lf.tri_inverse_f64(u["L"])
    Xc = X.copy()
    Xc[64:128, 0:64] = X[64:128, 0:64].T
    assert _sinv_worst(u["L"], X.T @ X) <= lf.C_ORACLE["sinv"]
    _beyond("4 block (1, 0) of Linv transposed", _sinv_worst(u["L"], Xc.T @ Xc), lf.c_kernel()["sinv"])
    old = rel_norm(Xc.T @ Xc, np.linalg.inv(u["L"] @ u["L"].T))
    print("[linalg] corruption 4: max|Sinv - inv| / max|inv| = %.3g (threshold 1e-9: caught by the present yardstick as well)" % old)
    assert old >= 1e-9


def test_corruption_5_ragged_merge_with_full_size_k():
    """M = 129: the last merge X21 = -X22 (L21 X11) has a 1 x 1 X22; with K = 128 instead of K_last = 1 the product folds in one
    more column of X22 and row of T: seeded garbage g0 * g (2^-10 normal) on row 128 of Linv."""
    u = lc.potri_case("M129")["lat"][0]
    X = lf.tri_inverse_f64(u["L"])
    rng = np.random.RandomState(129)
    Xc = X.copy()
    Xc[128, :128] += 2.0 ** -10 * rng.randn() * rng.randn(128)
    _beyond("5 ragged merge with a full-size K", _sinv_worst(u["L"], Xc.T @ Xc), lf.c_kernel()["sinv"])


def _solve_worst(c, X):
    return lf.worst(*lf.solve_terms(c["L"], c["B"], X))[0]


def test_corruption_6_column_group_left_unsubstituted():
    """Rows 16..31, columns 40..43 of the result still hold the backward solve's right-hand side of that group: y L[g, g]."""
    c = lc.solve_case("M100n333-R-a")
    X = lf.solve_f64(c["L"], c["B"])
    assert _solve_worst(c, X) <= lf.C_ORACLE["solve"]
    Xc = X.copy()
    Xc[16:32, 40:44] = X[16:32, 40:44] @ c["L"][40:44, 40:44]
    _beyond("6 a 4-column group of 16 rows unsubstituted", _solve_worst(c, Xc), lf.c_kernel()["solve"])


def test_corruption_7_ragged_row_tile_clamped_to_the_last_row():
    """n = 333 = 20 * 16 + 13: the 13 rows of the ragged last 16-row tile each hold row n - 1 (a clamped load used as a value)."""
    c = lc.solve_case("M100n333-W-a")
    X = lf.solve_f64(c["L"], c["B"])
    Xc = X.copy()
    Xc[320:] = X[332]
    _beyond("7 ragged row tile replaced by row n - 1", _solve_worst(c, Xc), lf.c_kernel()["solve"])


def test_corruption_8_small_row_off_by_1e_3():
    """One of the 2^-20 rows of right-hand sides (c) is relatively off by 1e-3.  Its residual is 1e-3 |b| whatever the matrix and S is
    about cond |b|, so the ratio is 1e-3 / (2^-52 cond): asserted with the 2^20 margin on the control matrix W (cond <= 5); on R
    (cond 1e7) the same slip is still 2^10 times beyond C_KERNEL, which is asserted as that.  The yardstick of test_potrs_rows_vs_lapack,
    max|out - ref| <= max(1e-13, 50 cond 2.2e-16) max|ref|, accepts both."""
    C = lf.c_kernel()["solve"]
    for tag, margin in (("M100n333-W-c", MARGIN), ("M100n333-R-c", 2.0 ** 10)):
        c = lc.solve_case(tag)
        X = lf.solve_f64(c["L"], c["B"])
        r = int(np.argmin(c["exps"]))
        Xc = X.copy()
        Xc[r] *= 1.0 + 1e-3
        assert _solve_worst(c, X) <= lf.C_ORACLE["solve"]
        _beyond("8 (%s) a 2^-20 row off by 1e-3" % tag, _solve_worst(c, Xc), C, margin)
        ref = sl.cho_solve((c["L"], True), c["B"].T).T
        old = np.max(np.abs(Xc - ref)) / np.max(np.abs(ref))
        bound = max(1e-13, 50.0 * c["cond"] * 2.2e-16)
        print("[linalg] corruption 8 (%s): max|out - ref| / max|ref| = %.3g (threshold %.3g)" % (tag, old, bound))
        assert old <= bound
