"""The dense, well-conditioned cases of DESIGN 9c and their extended-precision references (tests/rowpass_ref.py), built once per
process in a pool of at most 16 fresh worker processes and shared by tests/test_rowpass_ref_cpu.py and tests/test_rowpass_dense_gpu.py.

Recipe: `synth`'s seeded case with lengthscale = (16, 100) x inducing spacing (K^ dense: every column of a row counts), m_u scaled by
0.1 and forced_rung = 6 for every latent: the jitter is variance * 1e-6 * 10^6 = variance, so cond(K_uu + jitter) <= M + 1.
A case may name its own multipliers of the spacing ("cs", one per latent); the last latent is the dense one (`dense_latent`)."""
import multiprocessing
import os
import time

import numpy as np

SPECS = [("Gaussian", {"sigma": 0.5}), ("Poisson", {}), ("Bernoulli", {})]
RUNG = 6
CASES = {      # tag: M, Ns, P, Q[, cs: lengthscale / h per latent, default (16, 100)] -- the path each pins is listed in DESIGN 9c
    "A": dict(M=64, Ns=[130, 17], P=1, Q=2),
    "B": dict(M=200, Ns=[333, 130, 1], P=2, Q=2),
    "C": dict(M=256, Ns=[777, 130, 1], P=1, Q=2),
    "D": dict(M=384, Ns=[1030, 515, 17], P=1, Q=2),
    "E": dict(M=512, Ns=[1500, 700], P=2, Q=2),
    # F (one latent): 100 h at M = 1024 is a tenth of the input range and K^ falls to e^-50 across it (min|H| / max|H| = 3.9e-12, far
    # tiles numerically zero again); it takes the ABSOLUTE lengthscale of case D's dense latent instead, 100 / 383 = 267 h
    "F": dict(M=1024, Ns=[700, 200], P=1, Q=1, cs=(100.0 * 1023.0 / 383.0,)),
    # 3-D / 4-D inputs and HMOGP_MAXQ latents through the regular kernels (held to the WIDE constants of rowpass_ref)
    "G": dict(M=256, Ns=[777, 130, 1], P=3, Q=2),
    "H": dict(M=203, Ns=[333, 130, 17], P=4, Q=2),
    "I": dict(M=128, Ns=[300, 130, 17], P=2, Q=8, cs=(16.0, 100.0) * 4),
    # the smallest shape the strict mode's panel kernels take (one column block, 1057 rows = 8 row tiles + 33) with an odd number of
    # latents, so that the stride of the interleaved m_u matters; held to C_ORACLE / C_KERNEL
    "J": dict(M=128, Ns=[1040, 17], P=1, Q=3, cs=(16.0, 40.0, 100.0)),
}
BASE_TAGS = ["A", "B", "C", "D", "E", "F"]     # the cases C_ORACLE / C_KERNEL were settled on; the tail (tests/tail_cases.py) takes these
WIDE_TAGS = ["G", "H", "I"]                    # held to C_ORACLE_WIDE / C_KERNEL_WIDE
D_BATCH_SCALE = [1.0, 3.5, 0.25]
D_SHARD = ([37, 5, 3], [1001, 500, 17])      # [row_begin, row_end) per task; no begin is a multiple of 16
H_SHARD = ([37, 5, 3], [301, 120, 17])       # the X offset of a task is row_begin * 4 doubles
# the variants of a case, each with a reference of its own: name -> keyword arguments of rowpass_ref.reference
# (strict: the one-solve form of the strict q(f) mode; strict2, strict2_shard: its two-solve form)
VARIANTS = {
    "B": dict(strict2=dict(strict="two")),
    "D": dict(bs=dict(batch_scale=D_BATCH_SCALE), shard=dict(row_begin=D_SHARD[0], row_end=D_SHARD[1]), strict=dict(strict=True),
              strict2=dict(strict="two"), strict2_shard=dict(row_begin=D_SHARD[0], row_end=D_SHARD[1], strict="two")),
    "G": dict(bs=dict(batch_scale=D_BATCH_SCALE), strict=dict(strict=True), strict2=dict(strict="two")),
    "H": dict(shard=dict(row_begin=H_SHARD[0], row_end=H_SHARD[1]), strict=dict(strict=True), strict2=dict(strict="two")),
    "J": dict(strict=dict(strict=True), strict2=dict(strict="two")),
}
STRICT2_TAGS = ["B", "D", "G", "H", "J"]


def dense_latent(tag):
    """Index of the 100 h latent."""
    return CASES[tag]["Q"] - 1


def dense_case(tag):
    """(prm, prob, X, Y, forced_rungs) of one case."""
    from model_cases import synth
    c = CASES[tag]
    prm, prob, X, Y = synth(50 + c["M"], SPECS[:len(c["Ns"])], c["Ns"], c["M"], c["Q"], c["P"], c.get("cs", (16.0, 100.0)))
    prm["m_u"] = 0.1 * prm["m_u"]
    return prm, prob, X, Y, [RUNG] * c["Q"]


# Case K: the strict mode picks its two-solve form BY ITSELF -- latent 0 at 2 h without jitter (cond(K_uu) about 2e8, the
# engine's estimate variance max diag(K_uu^-1) about 4e6 > 1e6, float64 Cholesky succeeds), latent 1 at 100 h and rung 6 (estimate 1).
# Not one of CASES: it is ill-conditioned on purpose, closeness to R is conditioning-limited there.
K_CS = 2.0                    # lengthscale / h of latent 0 (the draw reaches the estimate 2e6 at 2.0: nothing had to be raised)
K_RUNGS = [-1, 6]
K_KINDS = ("ve", "sgv", "H", "r", "dZ", "sa", "sl", "swk", "m", "v")
# max|oracle - R| / max|R| per kind of the float64 oracle's two-solve restatement on case K, rounded up to a power of two like every
# C_ORACLE (measured 2026-10-21 on the CPU: ve 2.2e-6, sgv 5.8e-8, H 6.0e-6, r 9.3e-6, dZ 5.7e-5, sa 6.9e-5, sl 8.3e-7, swk 3.8e-5,
# m 1.7e-5, v 9.2e-6; tests/test_rowpass_ref_cpu.py asserts the oracle within it and no more than 16 x below it).  The kernels get
# 16 x, the margin tests/test_small_model_gpu.py gives a conditioning-limited comparison.
K_ORACLE_DIST = dict(ve=2.0 ** -18, sgv=2.0 ** -24, H=2.0 ** -17, r=2.0 ** -16, 
                     dZ=2.0 ** -14, sa=2.0 ** -13, sl=2.0 ** -20, swk=2.0 ** -14, m=2.0 ** -15, v=2.0 ** -16)


def auto_case(cs0=K_CS, m_scale=0.1):
    """(prm, prob, X, Y, forced_rungs) of case K; cs0 = 1.0 gives the well-conditioned neighbour (one-solve form) on the same data."""
    from model_cases import synth
    prm, prob, X, Y = synth(50 + 256, SPECS[:2], [1040, 130], 256, 2, 1, (cs0, 100.0))
    prm["m_u"] = m_scale * prm["m_u"]
    return prm, prob, X, Y, list(K_RUNGS)


def array_distances(got, R, kinds=K_KINDS):
    """{kind: max|got - R| / max|R|} over the whole kind (H: the lower triangles of every latent; m, v: every function)."""
    import rowpass_ref as rr
    out = {}
    for k in kinds:
        parts = rr.pairs(k, got[k], R[k], R[k])
        g = np.concatenate([np.asarray(x, dtype=np.float64).reshape(-1) for _, x, _, _ in parts])
        r = np.concatenate([np.asarray(x).reshape(-1) for _, _, x, _ in parts])
        out[k] = float(np.max(np.abs(g.astype(np.longdouble) - r)) / np.max(np.abs(r)))
    return out


def _build_auto():
    import rowpass_ref as rr
    t0 = time.time()
    prm, prob, X, Y, rungs = auto_case()
    cache = {}
    out = dict(two=rr.reference(prm, prob, X, Y, rungs, cache=cache, strict="two"),
               one=rr.reference(prm, prob, X, Y, rungs, cache=cache, strict=True))
    out["facts"] = dict(seconds=time.time() - t0)
    return out


def banded_case(M=384, Ns=(1030, 515, 17)):
    """The EXISTING style of case (lengthscale about one inducing spacing, free ladder) at case D's shape."""
    from model_cases import synth
    return synth(50 + M, SPECS[:len(Ns)], list(Ns), M, 2, 1, (1.0, 1.25))


def _build(tag):
    import rowpass_ref as rr
    t0 = time.time()
    prm, prob, X, Y, rungs = dense_case(tag)
    cache = {}
    out = dict(default=rr.reference(prm, prob, X, Y, rungs, cache=cache))
    for name, kw in VARIANTS.get(tag, {}).items():
        out[name] = rr.reference(prm, prob, X, Y, rungs, cache=cache, **kw)
    side, rows = cache["side"], cache["rows"]
    M = prob["M"]
    facts = dict(
        cond=[float(np.linalg.cond((u["Kuu"] + np.eye(M) * u["jitter"]).astype(np.float64))) for u in side],
        gate_all=all(bool(lat["gate"].all()) for o in rows for lat in o["lat"]),
        gv_max=[float(o["gv"].max()) if o["N"] else -np.inf for o in rows],
        seconds=time.time() - t0)
    out["facts"] = facts
    out["side"] = side          # the M x M side, for the references of the tail (tests/tail_cases.py)
    return tag, out


_REFS = {}


def references():
    """{tag: {"default": (R, S), "facts": {...}, "side": [...][, the variants of VARIANTS[tag]]}} for every case, and under "K" the
    two references {"two": (R, S), "one": (R, S)} of case K; built on first use."""
    if not _REFS:
        tags = ["F", "E", "D", "G", "I", "H", "C", "B", "J", "A"]          # the longest first
        n = max(1, min(16, len(tags), os.cpu_count() or 1))
        t0 = time.time()
        with multiprocessing.get_context("spawn").Pool(n) as pool:
            auto = pool.apply_async(_build_auto)
            for tag, out in pool.imap_unordered(_build, tags):
                _REFS[tag] = out
            _REFS["K"] = auto.get()
        print("[rowpass] references of %d cases in %.1f s (%s)" % (
            len(_REFS), time.time() - t0, " ".join("%s %.1f" % (t, _REFS[t]["facts"]["seconds"]) for t in sorted(_REFS))))
    return _REFS
