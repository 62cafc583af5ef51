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
}
BASE_TAGS = ["A", "B", "C", "D", "E", "F"]     # the cases C_ORACLE / C_KERNEL were settled on; the tail (tests/tail_cases.py) takes these
WIDE_TAGS = ["G", "H", "I"]                    # held to C_ORACLE_WIDE / C_KERNEL_WIDE
D_BATCH_SCALE = [1.0, 3.5, 0.25]
D_SHARD = ([37, 5, 3], [1001, 500, 17])      # [row_begin, row_end) per task; no begin is a multiple of 16
H_SHARD = ([37, 5, 3], [301, 120, 17])       # the X offset of a task is row_begin * 4 doubles
# the variants of a case, each with a reference of its own: name -> keyword arguments of rowpass_ref.reference
VARIANTS = {
    "D": dict(bs=dict(batch_scale=D_BATCH_SCALE), shard=dict(row_begin=D_SHARD[0], row_end=D_SHARD[1]), strict=dict(strict=True)),
    "G": dict(bs=dict(batch_scale=D_BATCH_SCALE), strict=dict(strict=True)),
    "H": dict(shard=dict(row_begin=H_SHARD[0], row_end=H_SHARD[1]), strict=dict(strict=True)),
}


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
    """{tag: {"default": (R, S), "facts": {...}, "side": [...][, the variants of VARIANTS[tag]]}} for every case; built on first use."""
    if not _REFS:
        tags = ["F", "E", "D", "G", "I", "H", "C", "B", "A"]          # the longest first
        n = max(1, min(16, len(tags), os.cpu_count() or 1))
        t0 = time.time()
        with multiprocessing.get_context("spawn").Pool(n) as pool:
            for tag, out in pool.imap_unordered(_build, tags):
                _REFS[tag] = out
        print("[rowpass] references of %d cases in %.1f s (%s)" % (
            len(tags), time.time() - t0, " ".join("%s %.1f" % (t, _REFS[t]["facts"]["seconds"]) for t in sorted(_REFS))))
    return _REFS
