"""The banded cases of DESIGN 9u -- exact-zero windows that really cut -- and their extended-precision references
(tests/rowpass_ref.py), built once per process in a pool of at most 16 fresh worker processes and shared by tests/test_windows_cpu.py and
tests/test_windows_pinned_gpu.py.  tests/rowpass_cases.py and its cases are not touched.

Recipe: `synth`'s seeded case with the lengthscales of the table below (multiples of the inducing spacing), m_u scaled by 0.1 and
forced_rung = 6 for every latent, as the dense cases; what each case pins is listed in DESIGN 9u.

  W1   M 384, rows 1030 / 515 / 17, 1-D, l = (0.5, 1.25) h: three column blocks, both latents banded, tail tiles of 6 and 17 rows
  W1s  W1 with every task's rows shuffled (fixed seed; the 128-row runs change places and each is shuffled inside -- a uniform shuffle
       gives nearly full windows WITHOUT the fallback, see `shuffle_by_tiles`): `window_fix_kernel` must fall back to the full ranges
  W2   M 300 (last block 44 columns, (M + 15) & ~15 = 304 > M), l = (0.5, 100) h: one latent banded, one full, in the same launches
  W3   M 384, task 0 rebuilt: rows 0-255 in [0, 0.3], 256-511 in [0.7, 1], 512-639 in [5, 6]: a row tile with an empty window and a
       column block with an empty hull, still banded
  W4   M 400, 2-D, l = (0.03, 0.06) h, rows sorted by their first coordinate: `window_kernel<2>`, `colstats_kernel<2, ., ., true>`"""
import multiprocessing
import os
import time

import numpy as np

import rowpass_cases as rc
import rowpass_ref as rr

SPECS = rc.SPECS
RUNG = rc.RUNG
CASES = {
    "W1": dict(M=384, Ns=[1030, 515, 17], P=1, Q=2, cs=(0.5, 1.25)),
    "W1s": dict(M=384, Ns=[1030, 515, 17], P=1, Q=2, cs=(0.5, 1.25)),
    "W2": dict(M=300, Ns=[700, 130], P=1, Q=2, cs=(0.5, 100.0)),
    "W3": dict(M=384, Ns=[640, 130], P=1, Q=2, cs=(0.5, 1.0)),
    "W4": dict(M=400, Ns=[700, 130], P=2, Q=2, cs=(0.03, 0.06)),
}
BANDED_TAGS = ["W1", "W2", "W3", "W4"]          # W1s is W1 behind the dense fallback
W1_BATCH_SCALE = rc.D_BATCH_SCALE
W1_SHARD = rc.D_SHARD                          # case D's shard: no begin is a multiple of 16, so the tile grid of every task shifts
W1_CHUNK_ROWS = 512
VARIANTS = {"W1": dict(bs=dict(batch_scale=W1_BATCH_SCALE), shard=dict(row_begin=W1_SHARD[0], row_end=W1_SHARD[1]))}
SHUFFLE_SEED = 20261021
# the stale-read sequence of W1: lengthscales under which K^ has no zero at all, and a variance that makes every entry large
W1_HOT = dict(cs=(16.0, 100.0), variance_scale=1000.0)
W1_Z_SHIFT = 0.2

# Constants (the rule of DESIGN 9c): per kind max(C_ORACLE, the float64 oracle's largest ratio against R over W1-W4, W1s and W1's
# variants rounded up to a power of two); the kernels get max(16, 4 x) that.  Measured on the CPU (tests/test_windows_cpu.py prints and
# asserts it; the raw figures per case are in DESIGN 9u) -- never from what the device produced.
# Every kind moves, and for one reason: at l = 0.5 h (and 0.03 h in 2-D) the float64 K^ itself is 4e5 ulps from the exact one.  GPy's
# distance r2 = (-2 x.z + (|x|^2 + |z|^2)) / l^2 -- the oracle's and the device's form alike -- cancels to an absolute error of
# 2^-53 (|x|^2 + |z|^2) / l^2 = 1.3e-10 at these lengthscales, which exp(-r2 / 2) turns into that relative error of every entry
# (measured: 9.2e-11 on W1, 9.9e-11 on W4); R forms (x - z)^2 in extended precision and S takes K^ as exact.  The dense cases sit at
# l >= 16 h, a thousand times less.  Largest ratios: ve 247.2 (W1 bs), sgv 735.6 (W1), H 1.004e6 (W4), r 5.285e5 (W4), dZ 5.226e5 (W4),
# sa 3.557e4 (W4), sl 5537 (W4), swk 3.558e4 (W4), dKmn 2.282e5 (W3), dKdiag 4.476e4 (W1), m 1.819e5 (W4), v 5.780e4 (W3).
C_ORACLE_WIN = dict(ve=256.0, sgv=1024.0, H=2.0 ** 20, r=2.0 ** 20, dZ=2.0 ** 19, sa=2.0 ** 16, sl=2.0 ** 13, swk=2.0 ** 16,
                    dKmn=2.0 ** 18, dKdiag=2.0 ** 16, m=2.0 ** 18, v=2.0 ** 16)
KERNEL_EXCEPTIONS = {}


def c_kernel_win():
    return {k: max(16.0, 4.0 * c) for k, c in C_ORACLE_WIN.items()}


_CASE = {}


def shuffle_by_tiles(n, rng):
    """A permutation of n sorted rows that makes `window_fix_kernel` fall back: the runs of 128 rows change places and the rows inside
    each run are shuffled.  (A uniform shuffle of all rows cannot: every tile's box then spans the whole domain, every tile touches every
    column block, and the windows are nearly full WITHOUT the fallback -- `uniform_shuffle` below, held to its tables only.)"""
    runs = [np.arange(i, min(i + 128, n)) for i in range(0, n, 128)]
    return np.concatenate([rng.permutation(runs[k]) for k in rng.permutation(len(runs))])


def uniform_shuffle(tag="W1"):
    """[(task, latent, X rows, Z_q, lengthscale_q)] of W1 with every task's rows shuffled uniformly (tables only: no reference)."""
    rng = np.random.RandomState(SHUFFLE_SEED + 1)
    perms = {}
    out = []
    for t, q, X, Z, ell in window_inputs(tag):
        if t not in perms:
            perms[t] = rng.permutation(X.shape[0])
        out.append((t, q, np.ascontiguousarray(X[perms[t]]), Z, ell))
    return out


def segments(n, chunk):
    """The row ranges a windows engine cuts a task of n rows into at chunk_rows = chunk (every segment is a pool of its own)."""
    return [(r0, min(n, r0 + chunk)) for r0 in range(0, n, chunk)]


def banded_case(tag):
    """(prm, prob, X, Y, forced_rungs) of one case."""
    if tag in _CASE:
        return _CASE[tag]
    from model_cases import synth
    c = CASES[tag]
    prm, prob, X, Y = synth(50 + c["M"], SPECS[:len(c["Ns"])], c["Ns"], c["M"], c["Q"], c["P"], c["cs"])
    prm["m_u"] = 0.1 * prm["m_u"]
    if tag == "W1s":
        rng = np.random.RandomState(SHUFFLE_SEED)
        for t in range(len(X)):
            perm = shuffle_by_tiles(X[t].shape[0], rng)
            X[t], Y[t] = np.ascontiguousarray(X[t][perm]), np.ascontiguousarray(Y[t][perm])
    if tag == "W3":
        x = X[0].copy()                   # sorted uniforms on [0, 1]: each group keeps its order, the groups are in order
        x[0:256] = 0.3 * x[0:256]
        x[256:512] = 0.7 + 0.3 * x[256:512]
        x[512:640] = 5.0 + x[512:640]
        X[0] = np.sort(x, axis=0)
    if tag == "W4":
        for t in range(len(X)):
            order = np.argsort(X[t][:, 0], kind="stable")
            X[t], Y[t] = np.ascontiguousarray(X[t][order]), np.ascontiguousarray(Y[t][order])
    _CASE[tag] = (prm, prob, X, Y, [RUNG] * c["Q"])
    return _CASE[tag]


def hot_params(prm, tag="W1", cs=None):
    """A 1-D case's parameters with l = (16, 100) h (or `cs` h) and variance x 1000: K^ has no exact zero and fills the whole workspace
    with large numbers."""
    h = 1.0 / (CASES[tag]["M"] - 1)
    return dict(prm, lengthscale=np.array(W1_HOT["cs"] if cs is None else cs) * h, variance=prm["variance"] * W1_HOT["variance_scale"])


def window_inputs(tag, row_begin=None, row_end=None):
    """[(task, latent, X rows, Z_q, lengthscale_q)] -- one entry per launch_windows call of a full-batch evaluation without row pools."""
    prm, prob, X, _, _ = banded_case(tag)
    P = prob["P"]
    out = []
    for t in range(prob["T"]):
        b = 0 if row_begin is None else row_begin[t]
        e = X[t].shape[0] if row_end is None else row_end[t]
        for q in range(prob["Q"]):
            out.append((t, q, X[t][b:e], np.ascontiguousarray(prm["Z"][:, q * P:(q + 1) * P]), float(prm["lengthscale"][q])))
    return out


def _build(tag):
    t0 = time.time()
    prm, prob, X, Y, rungs = banded_case(tag)
    cache = {}
    out = dict(default=rr.reference(prm, prob, X, Y, rungs, cache=cache))
    for name, kw in VARIANTS.get(tag, {}).items():
        out[name] = rr.reference(prm, prob, X, Y, rungs, cache=cache, **kw)
    side = cache["side"]
    M = prob["M"]
    out["facts"] = dict(cond=[float(np.linalg.cond((u["Kuu"] + np.eye(M) * u["jitter"]).astype(np.float64))) for u in side],
                        seconds=time.time() - t0)
    return tag, out


_REFS = {}


def references():
    """{tag: {"default": (R, S), "facts": {...}[, the variants of VARIANTS[tag]]}} for every case; built on first use."""
    if not _REFS:
        tags = ["W1", "W1s", "W4", "W3", "W2"]          # the longest first
        n = max(1, min(16, len(tags), os.cpu_count() or 1))
        t0 = time.time()
        with multiprocessing.get_context("spawn").Pool(n) as pool:
            for tag, out in pool.imap_unordered(_build, tags):
                _REFS[tag] = out
        print("[windows] references of %d cases in %.1f s (%s)" % (
            len(tags), time.time() - t0, " ".join("%s %.1f" % (t, _REFS[t]["facts"]["seconds"]) for t in sorted(_REFS))))
    return _REFS
