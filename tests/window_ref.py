"""The exact-zero windows of K^ = k(X, Z) restated: `window_init_kernel`, `window_kernel<P>` and `window_fix_kernel` of
hetmogp_amd/csrc/kuf.hip in float64, operation by operation, and the 50-digit facts they must respect.  Needs NumPy and mpmath only.

  windows(X, Z, ell)      the two integer tables the device must produce, integer for integer, with the intermediate facts the tests use
  exact_support(X, Z, ell)   {(n, m): r2 <= 1490} decided in 50 digits (float64 inputs taken as exact numbers)
  smallest_margin(X, Z, ell) the smallest |d2 / thr - 1| over all (tile, column) pairs, in 50 digits
  exp_image(X, Z, ell)    the float64 image exp(-r2 / 2) in the operation order of the hot-path variant of `rbf_kernel` (rbf_r2_fast)

The device may contract `d2 += d * d` into an FMA; the restatement does not.  The two agree on every decision `!(d2 > thr)` as long as no
(tile, column) pair sits within a few ulps of the threshold: `smallest_margin` >= 1e-7 (asserted per case in tests/test_windows_cpu.py)
leaves nine orders of magnitude over the 2^-52 such a contraction moves d2 by."""
import mpmath
import numpy as np

TILE = 128            # rows per tile and columns per block
GROUP = 16            # granularity of a row window
WINDOW_R2_MAX = 1491.0
SUPPORT_R2 = 1490     # exp(-r2 / 2) is a float64 non-zero only below r2 = 1490.27...: r2 <= 1490 is a subset of the true support
UNSET = 0x7FFFFFFF


def _xz(X, Z):
    X, Z = np.asarray(X, dtype=np.float64), np.asarray(Z, dtype=np.float64)
    X = X.reshape(X.shape[0], -1)
    Z = Z.reshape(Z.shape[0], -1)
    assert X.shape[1] == Z.shape[1]
    return X, Z


def threshold(ell):
    """WINDOW_R2_MAX * ell * ell * (1.0 + 1e-9), left to right."""
    ell = np.float64(ell)
    return np.float64(WINDOW_R2_MAX) * ell * ell * (np.float64(1.0) + np.float64(1e-9))


def boxes(X):
    """Per 128-row tile: (bmin [P], bmax [P], any_nan); fmin / fmax skip NaNs, a tile of NaNs alone keeps +inf / -inf."""
    N, P = X.shape
    out = []
    for r0 in range(0, N, TILE):
        x = X[r0:r0 + TILE]
        with np.errstate(all="ignore"):
            bmin = np.fmin.reduce(x, axis=0, initial=np.inf)
            bmax = np.fmax.reduce(x, axis=0, initial=-np.inf)
        out.append((bmin, bmax, bool(np.isnan(x).any())))
    return out


def box_d2(bmin, bmax, Z):
    """d = fmax(fmax(bmin - z, z - bmax), 0) per dimension, d2 = 0; d2 += d * d over p in order.  [M]"""
    d2 = np.zeros(Z.shape[0])
    with np.errstate(all="ignore"):
        for p in range(Z.shape[1]):
            z = Z[:, p]
            d = np.fmax(np.fmax(bmin[p] - z, z - bmax[p]), 0.0)
            d2 = d2 + d * d
    return d2


def windows(X, Z, ell):
    """dict: rowwin [tiles, 2], colwin [ncb, 2] (int32, what the device must give), fallback (bool), hit [tiles, M] (bool, per column),
    raw_rowwin / raw_colwin (before window_fix), d2 [tiles, M], thr."""
    X, Z = _xz(X, Z)
    N, M = X.shape[0], Z.shape[0]
    tiles, ncb, cap = (N + TILE - 1) // TILE, (M + TILE - 1) // TILE, (M + GROUP - 1) & ~(GROUP - 1)
    thr = threshold(ell)
    zn = np.isnan(Z).any(axis=1)
    rowwin = np.zeros((tiles, 2), dtype=np.int64)
    colwin = np.tile(np.array([UNSET, 0], dtype=np.int64), (ncb, 1))          # window_init_kernel
    hit = np.zeros((tiles, M), dtype=bool)
    d2s = np.zeros((tiles, M))
    for T, (bmin, bmax, any_nan) in enumerate(boxes(X)):
        d2 = box_d2(bmin, bmax, Z)
        d2s[T] = d2
        with np.errstate(all="ignore"):
            h = any_nan | zn | ~(d2 > thr)                                    # NaNs count as "possibly non-zero"
        hit[T] = h
        idx = np.flatnonzero(h)
        if idx.size:                                                          # none ? 0 : ...
            rowwin[T] = (idx[0] & ~(GROUP - 1), min((idx[-1] + 1 + GROUP - 1) & ~(GROUP - 1), cap))
        r0, nr = T * TILE, min(TILE, N - T * TILE)
        for cb in np.unique(idx >> 7):
            colwin[cb] = (min(colwin[cb, 0], r0), max(colwin[cb, 1], r0 + nr))
    raw_rowwin, raw_colwin = rowwin.copy(), colwin.copy()
    blockhit = np.stack([hit[:, cb * TILE:(cb + 1) * TILE].any(axis=1) for cb in range(ncb)], axis=1)     # [tiles, ncb]
    viol = False
    for cb in range(ncb):                                                     # window_fix_kernel
        lo, hi = colwin[cb]
        if lo == UNSET:
            continue
        viol |= not blockhit[lo >> 7:(hi + TILE - 1) >> 7, cb].all()
    if viol:
        rowwin[:] = (0, cap)
        colwin[:] = (0, N)
    else:
        colwin[colwin[:, 0] == UNSET] = (0, 0)
    return dict(rowwin=rowwin.astype(np.int32), colwin=colwin.astype(np.int32), fallback=bool(viol), hit=hit, blockhit=blockhit,
                raw_rowwin=raw_rowwin, raw_colwin=raw_colwin, d2=d2s, thr=thr)


def coverage(rowwin, M):
    """Share of (tile, 16-column group) pairs inside the row windows."""
    groups = (M + GROUP - 1) // GROUP
    return float(np.sum((rowwin[:, 1] - rowwin[:, 0]) // GROUP)) / (rowwin.shape[0] * groups)


def inside(rowwin, colwin, n, m):
    """For index arrays n, m: (inside the row window of n's tile, inside the row hull of m's column block)."""
    n, m = np.asarray(n), np.asarray(m)
    T, cb = n >> 7, m >> 7
    return (rowwin[T, 0] <= m) & (m < rowwin[T, 1]), (colwin[cb, 0] <= n) & (n < colwin[cb, 1])


def exp_image(X, Z, ell):
    """exp(-0.5 r2) in float64 with r2 = fmax(-2 x.z + (|x|^2 + |z|^2), 0) * (1 / ell^2), the order of rbf_r2_fast / sumsq.  [N, M]"""
    X, Z = _xz(X, Z)
    P = X.shape[1]
    xsq, zsq = X[:, 0] * X[:, 0], Z[:, 0] * Z[:, 0]
    dot = X[:, 0][:, None] * Z[:, 0][None, :]
    for p in range(1, P):
        xsq, zsq = xsq + X[:, p] * X[:, p], zsq + Z[:, p] * Z[:, p]
        dot = dot + X[:, p][:, None] * Z[:, p][None, :]
    il2 = 1.0 / (np.float64(ell) * np.float64(ell))
    r2 = np.fmax(-2.0 * dot + (xsq[:, None] + zsq[None, :]), 0.0) * il2
    with np.errstate(under="ignore"):
        return np.exp(-0.5 * r2)


# ================================================================================================ 50 digits
def _mp(x):
    return mpmath.mpf(float(x))


def exact_support(X, Z, ell):
    """Boolean [N, M]: r2 = sum_p (x_p - z_p)^2 / ell^2 <= 1490 with the float64 inputs taken as exact numbers.  A pair whose
    extended-precision r2 lies further than 1e-9 (relative) from 1490 is decided there (its error is below 1e-17); every other pair is
    decided in 50 digits.  Returns (support, number of pairs that needed the 50 digits)."""
    X, Z = _xz(X, Z)
    LD = np.longdouble
    d = X.astype(LD)[:, None, :] - Z.astype(LD)[None, :, :]
    r2 = np.sum(d * d, axis=2) / (LD(float(ell)) * LD(float(ell)))
    sup = np.asarray(r2 <= SUPPORT_R2)
    near = np.argwhere(np.abs(r2 / SUPPORT_R2 - 1) < 1e-9)
    with mpmath.workdps(50):
        l2 = _mp(ell) ** 2
        for n, m in near:
            sup[n, m] = sum((_mp(X[n, p]) - _mp(Z[m, p])) ** 2 for p in range(X.shape[1])) / l2 <= SUPPORT_R2
    return sup, len(near)


def smallest_margin(X, Z, ell):
    """min over (tile, column) of |d2 / thr - 1| in 50 digits, d2 the squared distance from z_m to the tile's box, thr = 1491 ell^2
    (1 + 1e-9) (the float64 constant 1e-9 taken as the exact number it is).  Tiles or columns with a NaN are skipped: their decision
    does not depend on d2.  Returns (margin, (tile, column))."""
    X, Z = _xz(X, Z)
    best, where = mpmath.inf, None
    with mpmath.workdps(50):
        thr = WINDOW_R2_MAX * _mp(ell) ** 2 * (1 + _mp(1e-9))
        for T, (bmin, bmax, any_nan) in enumerate(boxes(X)):
            if any_nan:
                continue
            lo, hi = [_mp(b) for b in bmin], [_mp(b) for b in bmax]
            for m in range(Z.shape[0]):
                if np.isnan(Z[m]).any():
                    continue
                d2 = mpmath.mpf(0)
                for p in range(Z.shape[1]):
                    z = _mp(Z[m, p])
                    d2 += max(lo[p] - z, z - hi[p], 0) ** 2
                g = abs(d2 / thr - 1)
                if g < best:
                    best, where = g, (T, m)
    return float(best), where
