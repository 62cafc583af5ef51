"""Element-by-element criterion for the M x M side: the Cholesky factor, the inverse through the triangular inverse and
Linv^T Linv, and the composed two-direction triangular solve, each judged by a residual or a forward error formed in np.longdouble from
the float64 output, with one scale per element.  Needs NumPy (mpmath comes in with tests/rowpass_ref.py, whose longdouble conventions,
`cholesky_ld` and `tri_inverse_ld` are used as they are); imports neither the oracle nor the package.

Criterion, in the form of tests/likgrid.py and rowpass_ref.check:

    |quantity| <= C[kind] * 2^-52 * max(S, 2^-1022)   for every element

  kind        quantity                                                   S
  chol        lower triangle of A + jitter I - L^ L^T                    |L^| |L^T|                     (Higham Thm 10.3; floor
                                                                         2^-1022 max(1, max|L^|): see `chol_terms`)
  chol_upper  strictly upper triangle of L^                              exact 0.0 (the floor alone: only 0.0 passes)
  sinv        potri(L) - Linv^T Linv, Linv = tri_inverse_ld(L)           |Linv|^T S_linv + S_linv^T |Linv| + |Linv|^T |Linv|,
                                                                         S_linv = |Linv| |L| |Linv|     (Higham 14, forward error)
  kinv        Ainv of jitchol_inv - Linv^T Linv, Linv from the kernel's  as sinv: the inverse is judged as the inverse of the factor
              own L^                                                     the kernel produced; Cholesky's error is judged under chol
  solve       X^ (L L^T) - B for potrs_rows(L, B)                        |X^| |L| |L^T|                 (Higham Thm 8.5, both
                                                                         directions: their bounds add to at most 2 gamma of this S)

The bounds hold for any order of summation, so the ratios do not grow with the condition number; the a-priori constant gamma is
about (M + 2) / 2 in these units.  Scales are float64 (BLAS): a scale needs no more.  There is no exception list.

Constants.  C_ORACLE[kind] = the largest ratio of a float64 run of the same plain algorithms (`cholesky_f64`, `tri_inverse_f64`,
X^T X, `solve_f64`: below) over all cases of tests/linalg_cases.py with M <= 384, rounded up to the next power of two
(tests/test_linalg_ref_cpu.py re-measures and asserts it).  The kernels get C_KERNEL = max(16, 4 * C_ORACLE), the rule of DESIGN 9a /
9c.  The constants are never fitted to the kernels."""
import numpy as np

from rowpass_ref import EPS, LD, TINY, _ld, cholesky_ld, tri_inverse_ld  # noqa: F401  (re-exported: one definition for both sides)

KINDS = ("chol", "chol_upper", "sinv", "kinv", "solve")

# Largest ratio of the plain float64 algorithms over the cases with M <= 384, rounded up to a power of two (measured 2026-10-19 on the
# CPU; the raw figures per case are in DESIGN 9f).
C_ORACLE = dict(chol=2.0, chol_upper=0.0, sinv=4.0, kinv=2.0, solve=2.0)


def c_kernel():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE.items()}


def next_pow2(x):
    return 0.0 if x <= 0 else float(2.0 ** np.ceil(np.log2(x)))


# ================================================================================================ plain float64 algorithms
def cholesky_f64(A):
    """Column Cholesky in float64 (the algorithm of `cholesky_ld`)."""
    A = np.asarray(A, dtype=np.float64)
    M = A.shape[0]
    L = np.zeros((M, M))
    for j in range(M):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError("not positive definite at column %d" % j)
        L[j, j] = np.sqrt(col[0])
        L[j + 1:, j] = col[1:] / L[j, j]
    return L


def tri_inverse_f64(L):
    """Row-by-row triangular inverse in float64 (the algorithm of `tri_inverse_ld`)."""
    L = np.asarray(L, dtype=np.float64)
    M = L.shape[0]
    X = np.zeros((M, M))
    for i in range(M):
        X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
        X[i, i] = 1.0 / L[i, i]
    return X


def solve_f64(L, B):
    """B (L L^T)^-1 for the rows of B in float64: forward substitution X L^T = B, then backward substitution Y L = X."""
    L, X = np.asarray(L, dtype=np.float64), np.array(B, dtype=np.float64)
    M = L.shape[0]
    for j in range(M):
        X[:, j] = (X[:, j] - X[:, :j] @ L[j, :j]) / L[j, j]
    for j in range(M - 1, -1, -1):
        X[:, j] = (X[:, j] - X[:, j + 1:] @ L[j + 1:, j]) / L[j, j]
    return X


# ================================================================================================ quantities and scales
def chol_terms(A, jitter, Lhat):
    """{"chol": (quantity, S), "chol_upper": (quantity, S)} of a float64 factor L^ of A + jitter I; the lower triangle (row-major
    order of np.tril_indices) and the strictly upper triangle as flat arrays."""
    A, Lh = _ld(A), np.asarray(Lhat, dtype=np.float64)
    M = A.shape[0]
    lo, up = np.tril_indices(M), np.triu_indices(M, 1)
    Ll = np.tril(Lh).astype(LD)
    res = A + np.eye(M, dtype=LD) * LD(float(jitter)) - Ll @ Ll.T
    La = np.abs(np.tril(Lh))
    S = (La @ La.T)[lo]
    # Where float64 ends: an element of L^ in the denormal range is stored to 2^-1075 absolute, and the residual sees that times its
    # partner, up to max|L^| (2^10 under the grading of the G cases).  The floor of this kind is therefore 2^-1022 max(1, max|L^|):
    # unchanged for an ungraded matrix, and felt only by elements whose whole reduction lies within 2^10 of the denormal range
    # (measured without it: 62 and 236 at M = 576 / 768 under grading, bit for bit the same for the plain algorithm, LAPACK and the
    # kernel).
    floor = TINY * max(1.0, float(La.max()))
    return {"chol": (res[lo], np.maximum(S, floor)), "chol_raw_S": S, "chol_upper": (Lh[up].astype(LD), np.zeros(up[0].size))}


def inv_reference(L):
    """(Linv^T Linv in longdouble, its scale in float64) for a float64 lower-triangular L, taken as exact."""
    Ll = np.tril(_ld(L))
    Li = tri_inverse_ld(Ll)
    Lia, La = np.abs(Li).astype(np.float64), np.abs(np.tril(np.asarray(L, dtype=np.float64)))
    S_linv = Lia @ La @ Lia
    G = Lia.T @ S_linv
    return Li.T @ Li, G + G.T + Lia.T @ Lia


def inv_terms(L, got):
    """(quantity, S) of kind sinv / kinv: got - Linv^T Linv on the full matrix."""
    R, S = inv_reference(L)
    return np.asarray(got, dtype=np.float64).astype(LD) - R, S


def solve_products(L):
    """(L L^T in longdouble, |L| |L^T| in float64): formed once per factor."""
    Ll, La = np.tril(_ld(L)), np.abs(np.tril(np.asarray(L, dtype=np.float64)))
    return Ll @ Ll.T, La @ La.T


def solve_terms(L, B, X, products=None):
    """(quantity, S) of kind solve: X^ (L L^T) - B and |X^| |L| |L^T|, [n, M]."""
    K, Ka = solve_products(L) if products is None else products
    X = np.asarray(X, dtype=np.float64)
    return X.astype(LD) @ K - _ld(B), np.abs(X) @ Ka


# ================================================================================================ criterion
def ratios(quantity, S):
    """|quantity| / (2^-52 max(S, 2^-1022)) per element, float64; 0 where the quantity is exactly 0, inf where it is not finite."""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(quantity, dtype=LD))
        r = np.where(d == 0, LD(0), d / (LD(EPS) * np.maximum(np.asarray(S, dtype=LD), LD(TINY)))).astype(np.float64)
    return np.where(np.isfinite(d), r, np.inf)


def worst(quantity, S):
    """(worst ratio, flat index, smallest S, number of elements with S below 2^-1022)."""
    x = ratios(quantity, S).reshape(-1)
    i = int(np.argmax(x))
    S = np.asarray(S)
    return float(x[i]), i, float(S.min()), int((S < TINY).sum())


def report(case, kind, w, C):
    print("[linalg] %-34s %-10s worst |quantity| / (2^-52 S) = %-10.4g (C = %g) at [%d]  min S = %.3g, %d below the floor" % (
        case, kind, w[0], C, w[1], w[2], w[3]))


def check(case, worsts, C):
    """`worsts`: {kind: `worst(...)`}.  Prints every kind before it asserts that each is within C[kind]; returns {kind: ratio}."""
    for k, w in worsts.items():
        report(case, k, w, C[k])
    bad = {k: (w[0], C[k]) for k, w in worsts.items() if not w[0] <= C[k]}
    assert not bad, (case, "beyond C", bad)
    return {k: w[0] for k, w in worsts.items()}
