"""The input gradients of tests/xgrad_ref.py in 50-digit arithmetic (mpmath): what tools/make_xgrad_grid.py rounds to double for
tests/golden/xgradgrid.npz.  The float64 inputs are taken exactly; every operation after that carries 50 digits.

  reference(inp, rows)              -> dict(dm, dv, S_dm, S_dv, F_dm, F_dv), each [len(rows), Df, P]  (float64; xgrad_ref's docstring)
  chain_reference(prm, Xnew, rows)  -> the same from the raw parameters (Z, m_u, L_flat, hypers): a = K^-1 m and C = K^-1 S K^-1 - K^-1
                                       formed at 50 digits (the reference of the engine path, default and strict alike)
  mean_var(I, x), grad(I, x)        -> the 50-digit m, v (x-dependent part) and dm, dv at one row x (a list of mpf): the formula itself is
                                       checked by central differences of the former against the latter (tests/test_xgrad_cpu.py)

Squared distances are exact, r^2 = sum_p (x_p - z_p)^2 (no clip is ever needed)."""
import mpmath as mp
import numpy as np

from joint_ref_mp import _mat, _r2, _vec, inverse_spd, matmul, transpose

mp.mp.dps = 50
_0 = mp.mpf(0)
_HALF = mp.mpf(1) / 2


def prepare(inp):
    """The inputs of the building block (xgrad_ref.make_inputs' dict; X is not used) as exact mpf values."""
    W = np.asarray(inp["W"], float)
    Q, Df = W.shape
    Zall = np.asarray(inp["Z"], float)
    P = Zall.shape[1] // Q
    I = dict(Q=Q, Df=Df, P=P, W=_mat(W), lat=[])
    for q in range(Q):
        C = inp["C"][q] if not isinstance(inp["C"][q], list) else None
        Cm = _mat(C) if C is not None else inp["C"][q]
        CT = transpose(Cm)                                  # CT[m] = column m of C: t_m = sum_m' k_m' C[m'][m]
        a = inp["a"][q]
        I["lat"].append(dict(Z=_mat(Zall[:, q * P:(q + 1) * P]), var=mp.mpf(float(inp["variance"][q])), ell=mp.mpf(float(inp["lengthscale"][q])),
                             a=a if isinstance(a, list) else _vec(a), CT=CT, aCT=[[abs(v) for v in col] for col in CT]))
    return I


def _kernel_row(lt, x):
    r2 = [_r2(x, z, lt["ell"]) for z in lt["Z"]]            # already divided by l^2
    return r2, [lt["var"] * mp.exp(-_HALF * r) for r in r2]


def mean_var(I, x):
    """(m [Df], v [Df]): m_d = sum_q W_qd p_q and the x-dependent part of v_d, sum_q W_qd^2 c_q."""
    m, v = [_0] * I["Df"], [_0] * I["Df"]
    for q, lt in enumerate(I["lat"]):
        _, k = _kernel_row(lt, x)
        p = mp.fdot(k, lt["a"])
        c = mp.fdot([mp.fdot(k, col) for col in lt["CT"]], k)
        for d in range(I["Df"]):
            w = I["W"][q][d]
            m[d] += w * p
            v[d] += w * w * c
    return m, v


def grad(I, x, scale=False):
    """(dm, dv) [Df][P] at the row x; with scale=True also (S_dm, S_dv, F_dm, F_dv)."""
    Df, P = I["Df"], I["P"]
    z2 = lambda: [[_0] * P for _ in range(Df)]
    dm, dv, sm, sv, fm, fv = z2(), z2(), z2(), z2(), z2(), z2()
    for q, lt in enumerate(I["lat"]):
        il2 = 1 / (lt["ell"] * lt["ell"])
        r2, k = _kernel_row(lt, x)
        t = [mp.fdot(k, col) for col in lt["CT"]]
        D = [[zj - xj for zj, xj in zip(z, x)] for z in lt["Z"]]
        if scale:
            ax2 = sum((xj * xj for xj in x), _0)
            e = [1 + (ax2 + sum((zj * zj for zj in z), _0) + 2 * sum((abs(xj) * abs(zj) for xj, zj in zip(x, z)), _0)) * _HALF * il2 + r * _HALF
                 for z, r in zip(lt["Z"], r2)]
            ke = [a * b for a, b in zip(k, e)]
            te = [mp.fdot(ke, col) for col in lt["aCT"]]
            csum = [sum(col, _0) for col in lt["aCT"]]
        for j in range(P):
            Dj = [row[j] for row in D]
            gp = il2 * mp.fdot([a * b for a, b in zip(lt["a"], k)], Dj)
            gc = 2 * il2 * mp.fdot([a * b for a, b in zip(t, k)], Dj)
            if scale:
                aD = [abs(v) for v in Dj]
                sgp = il2 * mp.fdot([abs(a) * b for a, b in zip(lt["a"], ke)], aD)
                sgc = 2 * il2 * mp.fdot([a * b for a, b in zip(te, ke)], aD)
                fgp = il2 * mp.fdot([abs(a) for a in lt["a"]], aD)
                fgc = 2 * il2 * lt["var"] * mp.fdot(csum, aD)
            for d in range(Df):
                w = I["W"][q][d]
                dm[d][j] += w * gp
                dv[d][j] += w * w * gc
                if scale:
                    sm[d][j] += abs(w) * sgp
                    sv[d][j] += w * w * sgc
                    fm[d][j] += abs(w) * fgp
                    fv[d][j] += w * w * fgc
    if scale:
        return dm, dv, sm, sv, fm, fv
    return dm, dv


def _rows(I, X, rows):
    f = lambda v: np.array([[[float(x) for x in r] for r in a] for a in v], dtype=float).reshape(len(v), I["Df"], I["P"])
    out = [grad(I, _vec(X[int(i)]), scale=True) for i in rows]
    keys = ("dm", "dv", "S_dm", "S_dv", "F_dm", "F_dv")
    return {k: f([o[n] for o in out]) for n, k in enumerate(keys)}


def reference(inp, rows):
    return _rows(prepare(inp), np.asarray(inp["X"], float), rows)


def chain_prepare(prm, P):
    """The building block's exact inputs from the raw parameters: K = k(Z_q, Z_q), a = K^-1 m_q, C = K^-1 L_q L_q^T K^-1 - K^-1."""
    M, Q = prm["m_u"].shape
    a, C = [], []
    for q in range(Q):
        var, ell = mp.mpf(float(prm["variance"][q])), mp.mpf(float(prm["lengthscale"][q]))
        Z = _mat(prm["Z"][:, q * P:(q + 1) * P])
        K = [[var * mp.exp(-_HALF * _r2(x, z, ell)) for z in Z] for x in Z]
        Ki = inverse_spd(K)
        Lq = [[_0] * M for _ in range(M)]
        for (i, j), v in zip(zip(*np.tril_indices(M)), _vec(prm["L_flat"][:, q])):
            Lq[i][j] = v
        KiS = matmul(Ki, matmul(Lq, transpose(Lq)))
        C.append([[x - y for x, y in zip(r1, r2)] for r1, r2 in zip(matmul(KiS, Ki), Ki)])
        a.append([mp.fdot(row, _vec(prm["m_u"][:, q])) for row in Ki])
    return prepare(dict(Z=prm["Z"], variance=prm["variance"], lengthscale=prm["lengthscale"], a=a, C=C, W=prm["W"]))


def chain_reference(prm, Xnew, rows):
    Xnew = np.asarray(Xnew, float)
    return _rows(chain_prepare(prm, Xnew.shape[1]), Xnew, rows)
