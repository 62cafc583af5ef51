"""The joint posterior of tests/joint_ref.py in 50-digit arithmetic (mpmath): what tools/make_joint_grid.py rounds to double for
tests/golden/jointgrid.npz.  The float64 parameters are taken exactly; every operation after that carries 50 digits, so the stored
values are the correctly rounded exact results for all purposes of a 2^-52 criterion.

  reference(prm, Xnew, functions, ri, ci) -> dict(mean [n], mean_scale [n], cov [len(ri)], cov_scale [len(ri)])   (float64)

The formulas are those of joint_ref's docstring with exact squared distances r2 = |x - x'|^2 / l^2 (no clip is ever needed) and the
explicit C_q = K^-1 S K^-1 - K^-1, K^-1 from the Cholesky factor by substitution."""
import mpmath as mp
import numpy as np

mp.mp.dps = 50
_0 = mp.mpf(0)


def _vec(a):
    return [mp.mpf(float(x)) for x in np.ravel(a)]


def _mat(a):
    return [_vec(row) for row in np.asarray(a, float)]


def cholesky(A):
    n = len(A)
    L = [[_0] * n for _ in range(n)]
    for i in range(n):
        Li = L[i]
        for j in range(i + 1):
            s = A[i][j] - mp.fdot(Li[:j], L[j][:j])
            Li[j] = mp.sqrt(s) if i == j else s / L[j][j]
    return L


def transpose(A):
    return [list(c) for c in zip(*A)]


def inverse_spd(A):
    """A^-1 of a symmetric positive definite matrix: L L^T = A, then two substitutions per unit vector."""
    n = len(A)
    L = cholesky(A)
    LT = transpose(L)
    cols = []
    for e in range(n):
        y = [_0] * n
        for i in range(e, n):                      # L y = e_e (y is zero above e)
            y[i] = ((mp.mpf(1) if i == e else _0) - mp.fdot(L[i][e:i], y[e:i])) / L[i][i]
        x = [_0] * n
        for i in range(n - 1, -1, -1):             # L^T x = y
            x[i] = (y[i] - mp.fdot(LT[i][i + 1:], x[i + 1:])) / L[i][i]
        cols.append(x)
    return [[(cols[i][j] + cols[j][i]) / 2 for j in range(n)] for i in range(n)]


def matmul(A, B):
    BT = transpose(B)
    return [[mp.fdot(a, b) for b in BT] for a in A]


def _r2(x, z, ell):
    return sum(((a - b) ** 2 for a, b in zip(x, z)), _0) / (ell * ell)


def reference(prm, Xnew, functions, ri, ci):
    Xnew = np.asarray(Xnew, float)
    N, P = Xnew.shape
    M, Q = prm["m_u"].shape
    d = list(functions)
    nD = len(d)
    n = nD * N
    ri, ci = np.asarray(ri, int), np.asarray(ci, int)
    rows = range(N)                                # (the mean needs every row)
    X = _mat(Xnew)
    mean, smean = [_0] * n, [_0] * n
    cov, scov = [_0] * len(ri), [_0] * len(ri)
    half = mp.mpf(1) / 2
    for q in range(Q):
        var, ell = mp.mpf(float(prm["variance"][q])), mp.mpf(float(prm["lengthscale"][q]))
        Z = _mat(prm["Z"][:, q * P:(q + 1) * P])
        K = [[var * mp.exp(-half * _r2(a, b, ell)) for b in Z] for a in Z]
        Ki = inverse_spd(K)
        Lq = [[_0] * M for _ in range(M)]
        flat = _vec(prm["L_flat"][:, q])
        for (i, j), v in zip(zip(*np.tril_indices(M)), flat):
            Lq[i][j] = v
        S = matmul(Lq, transpose(Lq))
        KiS = matmul(Ki, S)
        C = [[a - b for a, b in zip(r1, r2)] for r1, r2 in zip(matmul(KiS, Ki), Ki)]
        CT = transpose(C)
        aC = [[abs(v) for v in row] for row in CT]
        alpha = [mp.fdot(row, _vec(prm["m_u"][:, q])) for row in Ki]
        aalpha = [mp.fdot([abs(v) for v in row], [abs(v) for v in _vec(prm["m_u"][:, q])]) for row in Ki]      # |K^-1| |m|
        A, U, aA, aU = {}, {}, {}, {}
        for i in rows:
            r2 = [_r2(X[i], z, ell) for z in Z]
            A[i] = [var * mp.exp(-half * r) for r in r2]
            aA[i] = [abs(v) for v in A[i]]
            U[i] = [mp.fdot(A[i], c) for c in CT]          # a_i C
            aU[i] = [mp.fdot(aA[i], c) for c in aC]        # |a_i| |C|
            p = mp.fdot(A[i], alpha)
            canc = [sum(((abs(a) + abs(b)) ** 2 for a, b in zip(X[i], z)), _0) / (ell * ell) for z in Z]     # what -2 x.z + (|x|^2 + |z|^2) cancels from
            sp = mp.fdot([a * (1 + half * r + half * c) for a, r, c in zip(aA[i], r2, canc)], aalpha)
            for j in range(nD):
                w = mp.mpf(float(prm["W"][q, d[j]]))
                mean[j * N + i] += w * p
                smean[j * N + i] += abs(w) * sp
        for e, (r, c) in enumerate(zip(ri, ci)):
            j, i = divmod(int(r), N)
            jp, ip = divmod(int(c), N)
            wj, wjp = mp.mpf(float(prm["W"][q, d[j]])), mp.mpf(float(prm["W"][q, d[jp]]))
            ww = wj * wjp
            ck = ww + (mp.mpf(float(prm["kappa"][q, d[j]])) if j == jp else _0)
            r2 = _r2(X[i], X[ip], ell)
            k = var * mp.exp(-half * r2)
            cov[e] += ck * k + ww * mp.fdot(U[i], A[ip])
            scov[e] += abs(ck) * k * (1 + half * r2) + abs(ww) * mp.fdot(aU[i], aA[ip])
    f = lambda v: np.array([float(x) for x in v])
    return dict(mean=f(mean), mean_scale=f(smean), cov=f(cov), cov_scale=f(scov))
