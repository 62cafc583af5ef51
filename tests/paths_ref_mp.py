"""The pathwise posterior samples of tests/paths_ref.py in 50-digit arithmetic (mpmath): what tools/make_paths_grid.py rounds to double for
tests/golden/pathsgrid.npz, and what the GPU suite evaluates from the device's own state.  The float64 parameters are taken exactly; every
operation after that carries 50 digits, so the stored values are the correctly rounded exact results for all purposes of a 2^-52 criterion.

  state(prm, P, functions, S, Lf, seed, idx)  -> dict(zeta, omega (full), theta, u, v and their scales at the flat indices idx[...])   (float64)
  evaluate(st, prm, P, Xnew, idx)              -> (F, scale_F) at the flat indices idx of [S, nD, N], from the GIVEN float64 state

The formulas and scales are those of paths_ref's docstring with exact squared distances (no clip is ever needed) and exact sin / cos of pi t.
omega is ROUNDED TO DOUBLE where it is formed -- the stored value is the contract -- and the features use that double.  Independent of the
float64 code: the draws come from mclp_ref_mp, the linear algebra from joint_ref_mp."""
import mpmath as mp
import numpy as np

import joint_ref_mp as jm
import mclp_ref_mp as mm

mp.mp.dps = 50
_0 = mp.mpf(0)
TAG_FREQ, TAG_PRIOR, TAG_QU, TAG_KAPPA = 1, 2, 3, 4


def _z0(seed, n, s, pair):
    return mm.normal_pair(seed, n, s, pair)[0]


def _f(v):
    return np.array([float(x) for x in v])


def features(om, c, x):
    """(phi [2 Lf], sum_p |omega_lp x_p| [Lf]) of one input: om [Lf][P], x [P] as mpf."""
    cs, sn, at = [], [], []
    for w in om:
        t = mp.fdot(w, x)
        cs.append(c * mp.cospi(t))
        sn.append(c * mp.sinpi(t))
        at.append(sum((abs(a * b) for a, b in zip(w, x)), _0))
    return cs + sn, at


def _kernel_pieces(prm, q, P):
    var, ell = mp.mpf(float(prm["variance"][q])), mp.mpf(float(prm["lengthscale"][q]))
    Z = jm._mat(prm["Z"][:, q * P:(q + 1) * P])
    return var, ell, Z


def _solve(L, LT, b):
    n = len(b)
    y = [_0] * n
    for i in range(n):
        y[i] = (b[i] - mp.fdot(L[i][:i], y[:i])) / L[i][i]
    x = [_0] * n
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - mp.fdot(LT[i][i + 1:], x[i + 1:])) / L[i][i]
    return x


def state(prm, P, functions, S, Lf, seed, idx):
    M, Q = prm["m_u"].shape
    d = list(functions)
    nD, K2 = len(d), 2 * Lf
    half = mp.mpf(1) / 2
    zeta = np.zeros((Q, Lf, P))
    omega = np.zeros((Q, Lf, P))
    want = {k: {int(i): e for e, i in enumerate(idx[k])} for k in ("theta", "u", "v")}
    out = {k: np.zeros(len(idx[k])) for k in ("theta", "u", "v")}
    osc = {k: np.zeros(len(idx[k])) for k in ("theta", "u", "v")}
    for q in range(Q):
        var, ell, Z = _kernel_pieces(prm, q, P)
        for l in range(Lf):
            for p in range(P):
                z = _z0(seed, l, q * 4 + p, TAG_FREQ)
                zeta[q, l, p] = float(z)
                omega[q, l, p] = float(z / (mp.pi * ell))
        om = jm._mat(omega[q])
        c = mp.sqrt(var / Lf)
        K = [[var * mp.exp(-half * jm._r2(a, b, ell)) for b in Z] for a in Z]
        Lk = jm.cholesky(K)
        LkT = jm.transpose(Lk)
        need_v = any(q * M * S * nD <= i < (q + 1) * M * S * nD for i in want["v"])
        aKi = [[abs(x) for x in row] for row in jm.inverse_spd(K)] if need_v else None
        aLL = jm.matmul([[abs(x) for x in r] for r in Lk], [[abs(x) for x in r] for r in LkT]) if need_v else None
        fz = [features(om, c, z) for z in Z]
        PhiZ = [f[0] for f in fz]
        grow = [[1 + mp.pi * a for a in f[1]] * 2 for f in fz]                               # [M][2 Lf]
        Lq = [[_0] * M for _ in range(M)]
        for (i, j), v in zip(zip(*np.tril_indices(M)), jm._vec(prm["L_flat"][:, q])):
            Lq[i][j] = v
        m = jm._vec(prm["m_u"][:, q])
        w = [mp.mpf(float(prm["W"][q, dj])) for dj in d]
        sk = [mp.sqrt(mp.mpf(float(prm["kappa"][q, dj]))) for dj in d]
        for s in range(S):
            th = [_z0(seed, k, s * Q + q, TAG_PRIOR) for k in range(K2)]
            ep = [_z0(seed, mi, s * Q + q, TAG_QU) for mi in range(M)]
            for j in range(nD):
                for k in range(K2):
                    e = want["theta"].get(((q * K2 + k) * S + s) * nD + j)
                    if e is not None:
                        tk = _z0(seed, d[j] * K2 + k, s * Q + q, TAG_KAPPA)
                        out["theta"][e] = float(w[j] * th[k] + sk[j] * tk)
                        osc["theta"][e] = float(abs(w[j] * th[k]) + abs(sk[j] * tk))
            u = [m[i] + mp.fdot(Lq[i][:i + 1], ep[:i + 1]) for i in range(M)]
            su = [abs(m[i]) + mp.fdot([abs(x) for x in Lq[i][:i + 1]], [abs(x) for x in ep[:i + 1]]) for i in range(M)]
            for i in range(M):
                e = want["u"].get((q * S + s) * M + i)
                if e is not None:
                    out["u"][e], osc["u"][e] = float(u[i]), float(su[i])
            if not need_v:
                continue
            v = _solve(Lk, LkT, [u[i] - mp.fdot(PhiZ[i], th) for i in range(M)])
            ath, av = [abs(x) for x in th], [abs(x) for x in v]
            inner = [su[i] + mp.fdot([a * g for a, g in zip([abs(x) for x in PhiZ[i]], grow[i])], ath) + mp.fdot(aLL[i], av) for i in range(M)]
            for i in range(M):
                for j in range(nD):
                    e = want["v"].get(((q * M + i) * S + s) * nD + j)
                    if e is not None:
                        out["v"][e] = float(w[j] * v[i])
                        osc["v"][e] = float(abs(w[j]) * mp.fdot(aKi[i], inner))
    res = dict(zeta=zeta, omega=omega)
    for k in ("theta", "u", "v"):
        res[k], res[k + "_scale"] = out[k], osc[k]
    return res


def evaluate(st, prm, P, Xnew, idx):
    """(F, scale_F) at the flat indices idx of [S, nD, N] from the float64 state st (omega, theta, v taken exactly)."""
    Xnew = np.asarray(Xnew, float).reshape(-1, P)
    Q, K2, S, nD = st["theta"].shape
    Lf, N = K2 // 2, Xnew.shape[0]
    M = st["v"].shape[1]
    half = mp.mpf(1) / 2
    F, sF = [_0] * len(idx), [_0] * len(idx)
    rows = sorted({int(i) % N for i in idx})
    for q in range(Q):
        var, ell, Z = _kernel_pieces(prm, q, P)
        om = jm._mat(st["omega"][q])
        c = mp.sqrt(var / Lf)
        per_row = {}
        for i in rows:
            x = jm._vec(Xnew[i])
            phi, at = features(om, c, x)
            r2 = [jm._r2(x, z, ell) for z in Z]
            a = [var * mp.exp(-half * r) for r in r2]
            canc = [sum(((abs(p1) + abs(p2)) ** 2 for p1, p2 in zip(x, z)), _0) / (ell * ell) for z in Z]
            per_row[i] = (phi, [c * (1 + mp.pi * t) for t in at] * 2, a, [abs(ai) * (1 + half * r + half * cc) for ai, r, cc in zip(a, r2, canc)])
        for e, flat in enumerate(idx):
            sj, i = divmod(int(flat), N)
            s, j = divmod(sj, nD)
            phi, grow, a, aa = per_row[i]
            th, v = jm._vec(st["theta"][q, :, s, j]), jm._vec(st["v"][q, :, s, j])
            F[e] += mp.fdot(phi, th) + mp.fdot(a, v)
            sF[e] += mp.fdot(grow, [abs(t) for t in th]) + mp.fdot(aa, [abs(t) for t in v])
    return _f(F), _f(sF)
