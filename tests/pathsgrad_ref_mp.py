"""The gradients of posterior sample paths of tests/pathsgrad_ref.py in 50-digit arithmetic (mpmath): what tools/make_pathsgrad_grid.py rounds
to double for tests/golden/pathsgradgrid.npz, and what the GPU suite evaluates from the device's own state.  The float64 state and parameters
are taken exactly; every operation after that carries 50 digits.

  evaluate_grad(st, prm, P, Xnew, idx)   -> (G, scale_G) at the flat indices idx of [S, nD, N, P], from the GIVEN float64 state: the formula
                                            (float64; evaluate_grad_mp: the same, not rounded)
  path(st, prm, P, x, s, j)              -> f_j^s(x) at an mpf point x: the PATH itself, from paths_ref_mp's own pieces (features, _r2)
  numeric_grad(st, prm, P, Xnew, idx)    -> mp.diff of `path` at the same entries: the derivative of the 50-digit path taken numerically,
                                            which closes the formula itself and not only its rounding

The formulas and the scale are those of pathsgrad_ref's docstring with exact squared distances and exact sin / cos of pi t."""
import mpmath as mp
import numpy as np

import joint_ref_mp as jm
import paths_ref_mp as pm

mp.mp.dps = 50
_0 = mp.mpf(0)


def _f(v):
    return np.array([float(x) for x in v])


def evaluate_grad(st, prm, P, Xnew, idx):
    """(G, scale_G) at the flat indices idx of [S, nD, N, P] from the float64 state st (omega, theta, v taken exactly), rounded to double."""
    G, sG = evaluate_grad_mp(st, prm, P, Xnew, idx)
    return _f(G), _f(sG)


def evaluate_grad_mp(st, prm, P, Xnew, idx):
    """The same as lists of 50-digit numbers, not rounded (what `numeric_grad` is held against)."""
    Xnew = np.asarray(Xnew, float).reshape(-1, P)
    Q, K2, S, nD = st["theta"].shape
    Lf, N = K2 // 2, Xnew.shape[0]
    half = mp.mpf(1) / 2
    G, sG = [_0] * len(idx), [_0] * len(idx)
    rows = sorted({(int(i) // P) % N for i in idx})
    for q in range(Q):
        var, ell, Z = pm._kernel_pieces(prm, q, P)
        om = jm._mat(st["omega"][q])
        c = mp.sqrt(var / Lf)
        il2 = 1 / (ell * ell)
        per_row = {}
        for i in rows:
            x = jm._vec(Xnew[i])
            phi, at = pm.features(om, c, x)
            r2 = [jm._r2(x, z, ell) for z in Z]
            a = [var * mp.exp(-half * r) for r in r2]
            canc = [sum(((abs(p1) + abs(p2)) ** 2 for p1, p2 in zip(x, z)), _0) / (ell * ell) for z in Z]
            fold = [abs(ai) * (1 + half * r + half * cc) for ai, r, cc in zip(a, r2, canc)]
            per_row[i] = (x, phi, [c * (1 + mp.pi * t) for t in at] * 2, a, fold)
        for e, flat in enumerate(idx):
            rest, p = divmod(int(flat), P)
            sj, i = divmod(rest, N)
            s, j = divmod(sj, nD)
            x, phi, grow, a, fold = per_row[i]
            th, v = jm._vec(st["theta"][q, :, s, j]), jm._vec(st["v"][q, :, s, j])
            pw = [mp.pi * w[p] for w in om]
            # d phi_l = -pw phi_{Lf + l}, d phi_{Lf + l} = +pw phi_l
            dphi = [-pw[l] * phi[Lf + l] for l in range(Lf)] + [pw[l] * phi[l] for l in range(Lf)]
            dz = [(z[p] - x[p]) * il2 for z in Z]
            G[e] += mp.fdot(dphi, th) + mp.fdot([ai * d for ai, d in zip(a, dz)], v)
            # scale: |phi| folded as c (1 + pi sum |omega x|) against the rotated operand, |a| (1 + r2 / 2 + c / 2) |z - x| / l^2 against v
            rot = [abs(pw[l] * th[Lf + l]) for l in range(Lf)] + [abs(pw[l] * th[l]) for l in range(Lf)]
            sG[e] += mp.fdot(grow, rot) + mp.fdot([f * abs(d) for f, d in zip(fold, dz)], [abs(t) for t in v])
    return G, sG


def path(st, prm, P, x, s, j):
    """f_j^s(x) at the mpf point x [P], from the float64 state: paths_ref_mp's evaluation, one entry, its own pieces."""
    Q, K2 = st["theta"].shape[0], st["theta"].shape[1]
    Lf = K2 // 2
    half = mp.mpf(1) / 2
    f = _0
    for q in range(Q):
        var, ell, Z = pm._kernel_pieces(prm, q, P)
        phi, _ = pm.features(jm._mat(st["omega"][q]), mp.sqrt(var / Lf), x)
        a = [var * mp.exp(-half * jm._r2(x, z, ell)) for z in Z]
        f += mp.fdot(phi, jm._vec(st["theta"][q, :, s, j])) + mp.fdot(a, jm._vec(st["v"][q, :, s, j]))
    return f


def numeric_grad(st, prm, P, Xnew, idx):
    """mp.diff of the 50-digit path along x_p at the flat indices idx of [S, nD, N, P]."""
    Xnew = np.asarray(Xnew, float).reshape(-1, P)
    _, _, S, nD = st["theta"].shape
    N = Xnew.shape[0]
    out = []
    for flat in idx:
        rest, p = divmod(int(flat), P)
        sj, i = divmod(rest, N)
        s, j = divmod(sj, nD)
        x0 = jm._vec(Xnew[i])
        out.append(mp.diff(lambda t: path(st, prm, P, x0[:p] + [t] + x0[p + 1:], s, j), x0[p]))
    return out
