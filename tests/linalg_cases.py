"""The seeded cases of DESIGN 9f for `jitchol_inv`, `potri` and `potrs_rows`, the conditions every case has to meet, and the pool
that forms the longdouble residuals (tests/linalg_ref.py) of a set of outputs -- shared by tests/test_linalg_ref_cpu.py (outputs of
the plain float64 algorithms and of LAPACK) and tests/test_linalg_pinned_gpu.py (outputs of the kernels).  Imports neither the oracle
nor the package.

Matrices, per latent
  W   B B^T / M + I, B seeded normal: cond <= 5, the control.
  R   RBF K_uu (variance 1) on the grid 0, 1, ..., M - 1 with lengthscale 4 and forced rung 0: jitter 1e-6, cond about 1e7, the
      workload's conditioning.  "R8": lengthscale 8 and forced rung 1 (jitter 1e-5, cond about 2e6).
  G   D (K_uu + jitter I) D of an R matrix, D = diag(2^e), e seeded integers in [-10, 10] with both ends present, no jitter on top
      (forced rung -1).  Powers of two keep the input exact and the problem the same: any change in the ratios is the kernel's.
  L   (potri) a lower-triangular factor as `L_flat` carries it: D (diag(1 + 0.1 u) + 0.1 N e^{-|i-j|/16}), u uniform, N normal
      strictly lower, D as for G.

Where float64 itself ends.  exp(-d^2 / 32) is below 2^-1074 from d = 155 on: an R matrix with M > 155 holds exact zeros there, its
factor is banded to the same width, and |L^| |L^T| is exactly 0 (or denormal) beyond it.  The condition "no element of S below
2^-1022" can therefore hold for the chol kind of R / G only inside the band; it is asserted for |i - j| <= CHOL_BAND = 140 (where
e^{-d^2/32} 2^-20 is still above 1e-272), and outside the band the floor leaves 2^-1074 C: the residual has to be exact to a few
denormal steps (under grading: that times max|L^|, see linalg_ref.chol_terms).  Every other kind is asserted with no element below
2^-1022."""
import math
import multiprocessing
import os
import time

import numpy as np

CHOL_BAND = 140
NB = 32            # panel width of potrf_step_kernel


# ================================================================================================ matrices
def w_matrix(M, seed):
    B = np.random.RandomState(seed).randn(M, M)
    return B @ B.T / M + np.eye(M)


def rbf(M, ell):
    i = np.arange(M, dtype=np.float64)
    return np.exp(-(i[:, None] - i[None, :]) ** 2 / (2.0 * ell * ell))


def grading(n, seed, span):
    """n seeded integer exponents in [-span, span], both ends present (n >= 2)."""
    rng = np.random.RandomState(seed)
    e = rng.randint(-span, span + 1, n)
    if n >= 2:
        i, j = rng.choice(n, 2, replace=False)
        e[i], e[j] = -span, span
    return e


def ladder_jitter(A, rung):
    """The float64 jitter `jitchol_batched` adds: mean(diag) * 1e-6 * 10^rung with the diagonal summed in order; rung -1: none."""
    if rung < 0:
        return 0.0
    s = 0.0
    for x in np.diag(A):
        s += float(x)
    return s / A.shape[0] * 1e-6 * math.pow(10.0, rung)


R_KINDS = {"R": (4.0, 0), "R8": (8.0, 1)}      # lengthscale, forced rung


def latent_matrix(kind, M, seed):
    """One latent of a jitchol_inv case: dict(A = what the kernel is given, rung, jitter = what it adds, base = the unscaled matrix
    whose condition number is the case's, cond_range, exps)."""
    if kind == "W":
        A = w_matrix(M, seed)
        return dict(kind=kind, A=A, rung=-1, jitter=0.0, base=A, cond_range=(1.0, 10.0), exps=None)
    ell, rung = R_KINDS["R8" if kind == "R8" else "R"]
    K = rbf(M, ell)
    jit = ladder_jitter(K, rung)
    base = K + jit * np.eye(M)
    cr = (1e6, 1e8)
    if kind in ("R", "R8"):
        return dict(kind=kind, A=K, rung=rung, jitter=jit, base=base, cond_range=cr, exps=None)
    assert kind == "G", kind
    e = grading(M, seed, 10)
    d = 2.0 ** e
    return dict(kind=kind, A=d[:, None] * base * d[None, :], rung=-1, jitter=0.0, base=base, cond_range=cr, exps=e)


def l_matrix(M, seed):
    rng = np.random.RandomState(seed)
    i = np.arange(M)
    L0 = np.diag(1.0 + 0.1 * rng.rand(M)) + 0.1 * np.tril(rng.randn(M, M), -1) * np.exp(-np.abs(i[:, None] - i[None, :]) / 16.0)
    e = grading(M, seed + 1, 10)
    return dict(L=(2.0 ** e)[:, None] * L0, base=L0, exps=e)


def spd_cond(A):
    w = np.linalg.eigvalsh(A)
    return float(w[-1] / w[0])


# ================================================================================================ jitchol_inv
_ROT = [("W", "R"), ("R", "G"), ("G", "W")]
_Q8 = ["W", "R", "G", "R", "G", "R8", "G", "W"]     # latent 5 has a forced rung of its own (1; the R latents 0, W and G -1)
JITCHOL = {}     # tag: dict(M, Q, kinds, why)
for _i, (_M, _why) in enumerate([
        (31, "one ragged panel: a single launch, no trailing tile, one ragged trtri block"),
        (32, "exactly one panel"),
        (33, "one panel and a 1-row trailing tile, look-ahead block of 1"),
        (64, "two panels, one full trtri block, no merge"),
        (65, "first trtri merge, ragged right block of 1"),
        (129, "second trtri merge with M_last = K_last = 1; 64-tile potrf"),
        (200, "ragged panel, tile, trtri block and merges; 64-tile potrf"),
        (320, "doubling merges with an odd pair count (5 blocks of 64); 64-tile potrf"),
        (576, "64-tile potrf throughout (T64 = 9: 45 * 2 <= 512), ragged last 128 of the 128-wide merge level")]):
    JITCHOL["M%d" % _M] = dict(M=_M, Q=2, kinds=list(_ROT[_i % 3]), why=_why)
JITCHOL["M704"] = dict(M=704, Q=8, kinds=_Q8, why="first panel rem = 672, T64 = 11, 66 * 8 = 528 > 512: potrf_step_kernel<128> with a "
                       "ragged 32-wide last tile, then 64-tiles (rem = 640: 55 * 8 = 440), in one factorisation")
JITCHOL["M768"] = dict(M=768, Q=8, kinds=_Q8, why="three 128-tile panels (rem = 736, 704, 672), then 64-tiles")


def potrf_tiles(M, Q):
    """Tile edge per panel, the formula of launch_potrf_batched restated: rem = rows below the panel, T64 = ceil(rem / 64),
    64 x 64 tiles while T64 (T64 + 1) / 2 * Q <= 512, else 128 x 128."""
    out = []
    for j in range(0, M, NB):
        rem = M - j - min(NB, M - j)
        T64 = (rem + 63) // 64
        out.append(64 if T64 * (T64 + 1) // 2 * Q <= 512 else 128)
    return out


_CACHE = {}


def jitchol_case(tag):
    """dict(M, Q, A [Q, M, M], rungs, lat = [latent_matrix ...]); built once per process."""
    key = ("jitchol", tag)
    if key not in _CACHE:
        c = JITCHOL[tag]
        lat = [latent_matrix(k, c["M"], 1000 * c["M"] + q) for q, k in enumerate(c["kinds"])]
        _CACHE[key] = dict(M=c["M"], Q=c["Q"], A=np.stack([u["A"] for u in lat]), rungs=[u["rung"] for u in lat], lat=lat)
    return _CACHE[key]


def assert_latent_conditions(tag, q, u):
    lo, hi = u["cond_range"]
    cond = spd_cond(u["base"])
    assert lo <= cond <= hi, (tag, q, u["kind"], "cond", cond)
    if u["exps"] is not None:
        assert u["exps"].max() - u["exps"].min() >= 20, (tag, q, "grading")
    return cond


# ================================================================================================ potri
POTRI = {"M%d" % M: dict(M=M, Q=2, why=why) for M, why in [
    (33, "one ragged trtri block"), (64, "one full block"), (65, "first merge, ragged right block of 1"),
    (129, "second merge with M_last = K_last = 1"), (200, "ragged everything"), (320, "odd pair count"),
    (576, "ragged last 128 of the 128-wide level")]}


def potri_case(tag):
    key = ("potri", tag)
    if key not in _CACHE:
        c = POTRI[tag]
        lat = [l_matrix(c["M"], 2000 * c["M"] + 7 * q) for q in range(c["Q"])]
        _CACHE[key] = dict(M=c["M"], Q=c["Q"], L=np.stack([u["L"] for u in lat]), lat=lat)
    return _CACHE[key]


def assert_l_conditions(tag, q, u):
    cond = float(np.linalg.cond(u["base"]))
    assert cond <= 1e3, (tag, q, "cond of the ungraded factor", cond)
    assert u["exps"].max() - u["exps"].min() >= 20
    return cond


# ================================================================================================ potrs_rows
SOLVE_SHAPES = [(33, 1, "round-5"), (100, 333, "round-5"), (160, 1023, "round-5"), (257, 130, "round-5"),
                (128, 1024, "panel"), (256, 1025, "panel"), (384, 1153, "panel"), (512, 2049, "panel")]
SOLVE = {}       # tag: dict(M, n, mat, rhs, path)
for _M, _n, _path in SOLVE_SHAPES:
    for _mat, _rhss in (("W", "ac"), ("R", "abc")):
        for _rhs in _rhss:
            if _rhs == "c" and _n < 2:
                continue       # one row has no second scale to differ from
            SOLVE["M%dn%d-%s-%s" % (_M, _n, _mat, _rhs)] = dict(M=_M, n=_n, mat=_mat, rhs=_rhs, path=_path)
SUBSET_ROWS = 333
SOLVE_SUBSET = ["M%dn%d-R-c" % (M, n) for M, n, p in SOLVE_SHAPES if p == "panel"]     # first 333 rows: the round-5 kernels


def solve_path(M, n):
    """potrs_rows_inplace / trsm_panel_eligible restated: the one-launch-per-block kernels need M % 128 == 0 and n >= 1024."""
    return "panel" if M % 128 == 0 and n >= 1024 else "round-5"


def solve_factor(M, mat):
    """dict(L float64 = cholesky_ld of the matrix, rounded; cond, cond_range, ell)."""
    key = ("factor", M, mat)
    if key not in _CACHE:
        from linalg_ref import LD, cholesky_ld
        if mat == "W":
            A, ell, cr = w_matrix(M, 3000 + M), None, (1.0, 10.0)
            Al = A.astype(LD)
        else:
            ell, rung = R_KINDS["R8" if M == 128 else "R"]
            K = rbf(M, ell)
            jit = ladder_jitter(K, rung)
            A, cr = K + jit * np.eye(M), (1e6, 1e8)
            Al = K.astype(LD) + np.eye(M, dtype=LD) * LD(jit)
        _CACHE[key] = dict(L=cholesky_ld(Al).astype(np.float64), cond=spd_cond(A), cond_range=cr, ell=ell)
    return _CACHE[key]


def solve_case(tag):
    """dict(M, n, L, B, cond, cond_range, exps)."""
    key = ("solve", tag)
    if key not in _CACHE:
        c = SOLVE[tag]
        M, n = c["M"], c["n"]
        f = solve_factor(M, c["mat"])
        rng = np.random.RandomState(4000 + 7 * M + n + ord(c["rhs"]))
        exps = None
        if c["rhs"] == "a":
            B = rng.randn(n, M)
        elif c["rhs"] == "b":          # rows of K_uf at seeded inputs inside the grid, the same lengthscale: the real operand
            x = rng.uniform(0.0, M - 1.0, n)
            B = np.exp(-(x[:, None] - np.arange(M, dtype=np.float64)[None, :]) ** 2 / (2.0 * f["ell"] ** 2))
        else:
            exps = grading(n, 5000 + M + n, 20)
            B = rng.randn(n, M) * (2.0 ** exps)[:, None]
        _CACHE[key] = dict(M=M, n=n, L=f["L"], B=B, cond=f["cond"], cond_range=f["cond_range"], exps=exps)
    return _CACHE[key]


def assert_solve_conditions(tag, c):
    lo, hi = c["cond_range"]
    assert lo <= c["cond"] <= hi, (tag, "cond", c["cond"])
    assert solve_path(c["M"], c["n"]) == SOLVE[tag]["path"], tag
    if c["exps"] is not None:
        assert c["exps"].max() - c["exps"].min() >= 20, (tag, "row scales")


# ================================================================================================ residual jobs
def _chol_floor_ok(S, M):
    """Every lower-triangle element of S below 2^-1022 lies outside the band |i - j| <= CHOL_BAND."""
    from linalg_ref import TINY
    i, j = np.tril_indices(M)
    low = S < TINY
    return bool(not low.any() or (i - j)[low].min() > CHOL_BAND)


def _job(job):
    """One unit of longdouble work; returns (key, {kind: worst tuple}, {"floor_ok": bool, "seconds": s})."""
    import linalg_ref as lf
    t0 = time.time()
    what, key = job["what"], job["key"]
    out, ok = {}, True
    if what == "jitchol":
        t = lf.chol_terms(job["A"], job["jitter"], job["L"])
        out["chol"], out["chol_upper"] = lf.worst(*t["chol"]), lf.worst(*t["chol_upper"])
        ok = _chol_floor_ok(t["chol_raw_S"], job["A"].shape[0])
        if job.get("Ainv") is not None:
            out["kinv"] = lf.worst(*lf.inv_terms(job["L"], job["Ainv"]))
            ok = ok and out["kinv"][3] == 0
    elif what == "potri":
        out["sinv"] = lf.worst(*lf.inv_terms(job["L"], job["Sinv"]))
        ok = out["sinv"][3] == 0
    else:
        prod = lf.solve_products(job["L"])
        for name, (B, X) in job["pairs"].items():
            out[name] = lf.worst(*lf.solve_terms(job["L"], B, X, prod))
            ok = ok and out[name][3] == 0
    return key, out, dict(floor_ok=ok, seconds=time.time() - t0)


def run_jobs(jobs):
    """{key: ({kind: worst tuple}, facts)} of a list of jobs, in a pool of at most 16 fresh processes, the largest first."""
    if not jobs:
        return {}
    jobs = sorted(jobs, key=lambda j: -j["L"].shape[-1] ** 2 * (j["L"].shape[-1] + sum(p[0].shape[0] for p in j.get("pairs", {}).values())))
    n = max(1, min(16, len(jobs), os.cpu_count() or 1))
    t0 = time.time()
    res = {}
    with multiprocessing.get_context("spawn").Pool(n) as pool:
        for key, out, facts in pool.imap_unordered(_job, jobs):
            res[key] = (out, facts)
    print("[linalg] %d residual jobs in %.1f s on %d processes (%.1f s of work)" % (
        len(jobs), time.time() - t0, n, sum(f["seconds"] for _, f in res.values())))
    return res
