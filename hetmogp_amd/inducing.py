"""Inducing inputs from the data: `select_inducing` picks M of the pooled rows by greedy conditional variance under the model's own
kernels (pivoted incomplete Cholesky of K_ff; Burt, Rasmussen & van der Wilk 2020).  The reference leaves Z to the caller
(its constructor carries a commented-out `kmm_init`, svmogp.py:50).  All arithmetic happens on the device (csrc/zsel.hip)."""
import numpy as np

from . import _lib
from .engine import select_inducing_rows


def select_inducing(X, M, kern_list, tol=0.0, keep=None, device=None, return_info=False):
    """Z (Mout, P), ready for SVMOGP(Z=...).

    X          one (N, P) array or the per-task list; a list is pooled in task order
    M          the most inducing inputs to pick; fewer come back when the stop rule fires (Mout <= M)
    kern_list  the model's RBF objects, or a single one; one Z serves all latents, so the selection runs under their SUM
    tol        stop once the largest conditional variance is at or below tol * k(x, x)
    keep       optional (K0, P) points that must be inducing inputs, K0 <= M: appended to the pool and picked first, in their order
    With return_info also a dict: pivots (rows of the pool), rows ((task, row) pairs, task -1 for a `keep` point), cond_var (the
    conditional variance at each pick), trace (tr(K_ff - Q_ff) before each pick and after the last: how much the next points would still
    buy), chol_diag_min (the smallest Cholesky diagonal of the K_uu the model starts from, i.e. how well conditioned it is) and
    stopped_by_tol (the stop rule fired before M picks: tol, or the floor 2^-40 below which a conditional variance is rounding noise)."""
    tasks = [X] if isinstance(X, np.ndarray) else list(X)
    tasks = [np.asarray(x, dtype=float) for x in tasks]
    tasks = [x.reshape(x.shape[0], -1) for x in tasks]
    if not tasks:
        raise _lib.InvalidArgument("select_inducing: X is empty")
    P = tasks[0].shape[1]
    if any(x.shape[1] != P for x in tasks):
        raise _lib.InvalidArgument("select_inducing: every task's X must have the same number of columns")
    kerns = list(kern_list) if isinstance(kern_list, (list, tuple)) else [kern_list]
    M = int(M)
    pool = list(tasks)
    K0 = 0
    if keep is not None:
        keep = np.asarray(keep, dtype=float)
        if keep.ndim != 2 or keep.shape[1] != P:
            raise _lib.InvalidArgument("select_inducing: keep must have shape (K0, %d), got %s" % (P, keep.shape))
        K0 = keep.shape[0]
        if K0 > M:
            raise _lib.InvalidArgument("select_inducing: keep holds %d points, more than M = %d" % (K0, M))
        pool.append(keep)
    Xp = np.ascontiguousarray(np.vstack(pool))
    N0 = Xp.shape[0] - K0
    forced = np.arange(N0, N0 + K0, dtype=np.int64) if K0 else None
    r = select_inducing_rows(Xp, [float(k.variance[0]) for k in kerns], [float(k.lengthscale[0]) for k in kerns], M, tol=tol,
                             forced=forced, device=device)
    if not return_info:
        return r["Z"]
    starts = np.cumsum([0] + [x.shape[0] for x in tasks])
    piv = r["pivots"]
    task = np.searchsorted(starts, piv, side="right") - 1
    rows = np.stack([np.where(piv >= N0, -1, task), np.where(piv >= N0, piv - N0, piv - starts[np.minimum(task, len(tasks) - 1)])], 1) \
        if len(piv) else np.zeros((0, 2), dtype=np.int64)
    info = dict(pivots=piv, rows=rows.astype(np.int64), cond_var=r["dpiv"], trace=r["trace"],
                chol_diag_min=float(np.sqrt(np.min(r["dpiv"]))) if len(piv) else float("nan"),
                stopped_by_tol=bool(r["Mout"] < min(M, Xp.shape[0])))
    return r["Z"], info
