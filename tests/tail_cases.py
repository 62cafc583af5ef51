"""The cases of DESIGN 9g and their extended-precision references (tests/tail_ref.py), built once per process and shared by
tests/test_tail_ref_cpu.py and tests/test_tail_pinned_gpu.py.

(a) The dense cases A-F of tests/rowpass_cases.py (D also with its batch-scale and strict variants).  Bundle = `rr.pack_bundle(R, prob)`
    of the row-pass reference rounded to float64 and then taken as exact: the tail is isolated from row-pass error.  The row-pass
    references and the M x M side come from `rc.references()`, the same process cache: nothing is computed twice.
(b) Tail-only shapes, M = 33, 65, 129, 200, 257, 330, 576 (Q = 2, P = 1) and M = 144 with P = 2.  u-side from the 9c recipe (rung 6,
    lengthscales (16, 100) h, m_u scaled by 0.1), one 17-row Gaussian task so that `step_begin` runs, and a seeded DENSE bundle:
    H_q = -B^T B / n + 0.1 N with N symmetric (no Toeplitz structure), random r, dZ, sa, sl, swk, sgv, ve.  The tail is linear in the
    bundle, so no row reference is needed.
(c) Small-model shapes M = 33, 50, 64 with Ns = (130, 17), the 9c recipe, END TO END through `hmogp_elbo_grad` (the fused path cannot
    take an injected bundle).  Reference: the tail of the row-pass reference's own longdouble bundle.  Bound of an element:

        2^-52 (C[kind] S_tail + B),     B = the tail's linear maps in absolute value applied to the bundle's own 9c bound,

    i.e. `tail_ref.scales(..., const=False)` evaluated at c_kernel()[k] S_k (k = ve, sgv, H, r, dZ, sa, sl, swk: rowpass_ref's
    constants and scales) in place of |ve|, |sgv|, |H|, ...: every output of the tail is a sum of products of ONE bundle element with
    factors that do not depend on the bundle (K^-1, S, L, a, K_zz, z_j - z_m, 1 / l, W), so a bundle within c_k 2^-52 S_k of its
    reference moves an output by at most that sum over |factors| c_k 2^-52 S_k.  kl, wv, winv do not depend on the bundle: B = 0.

The M^3 longdouble products are formed by row ranges in a pool of at most 16 fresh processes (tests/tail_ref.py: heavy_rows)."""
import multiprocessing
import os
import time

import numpy as np

import rowpass_cases as rc
import rowpass_ref as rr
import tail_ref as tr

TAIL_ONLY = {"T33": (33, 1), "T65": (65, 1), "T129": (129, 1), "T144p2": (144, 2), "T200": (200, 1), "T257": (257, 1), "T330": (330, 1),
             "T576": (576, 1)}
SMALL = {"S33": 33, "S50": 50, "S64": 64}
SMALL_NS = [130, 17]
IN_MAXIMUM = ["A", "B", "C", "D", "E"] + [t for t, (M, _) in TAIL_ONLY.items() if M <= 330]      # the cases C_ORACLE is taken over


def tail_only_case(tag):
    """(prm, prob, X, Y, rungs, bundle) of one tail-only shape."""
    from model_cases import synth
    M, P = TAIL_ONLY[tag]
    prm, prob, X, Y = synth(50 + M, rc.SPECS[:1], [17], M, 2, P, (16.0, 100.0))
    prm["m_u"] = 0.1 * prm["m_u"]
    rng = np.random.RandomState(9000 + M)
    Q, Df = prob["Q"], prob["Df"]
    Rb = dict(ve=10.0 * rng.randn(1), nneg=np.zeros(1), sgv=rng.randn(Df), H=np.zeros((Q, M, M)), r=rng.randn(Q, M),
              dZ=rng.randn(Q, M, P), sa=rng.randn(Q), sl=rng.randn(Q), swk=rng.randn(Q, Df))
    for q in range(Q):
        B, N = rng.randn(M, M), rng.randn(M, M)
        Rb["H"][q] = -B.T @ B / M + 0.1 * (N + N.T) / 2
        Rb["H"][q] = tr.sym_lower(Rb["H"][q])
    return prm, prob, X, Y, [rc.RUNG] * Q, rr.pack_bundle(Rb, prob)


def small_case(tag):
    from model_cases import synth
    M = SMALL[tag]
    prm, prob, X, Y = synth(50 + M, rc.SPECS[:2], SMALL_NS, M, 2, 1, (16.0, 100.0))
    prm["m_u"] = 0.1 * prm["m_u"]
    return prm, prob, X, Y, [rc.RUNG, rc.RUNG]


def dense_bundle(refs, tag, variant="default"):
    prob = rc.dense_case(tag)[1]
    return tr.f64(rr.pack_bundle(refs[tag][variant][0], prob))


def _heavy(job):
    key, j = job
    return key, tr.heavy_rows(j)


def _linv(job):
    key, L = job
    return key, tr.tri_inverse_ld(L)


def _facts(side):
    M = side[0]["L"].shape[0]
    return dict(cond_S=[float(np.linalg.cond(tr.f64(u["S"]))) for u in side],
                cond_K=[float(np.linalg.cond(tr.f64(u["Kuu"]) + np.eye(M) * u["jitter"])) for u in side])


def _complete(tag, d, Linvs, joined):
    """The entry of one case from its heavy products: the light part of the reference, per variant."""
    prm, prob, X, Y, rungs = d["case"]
    names = sorted(d["variants"])
    out = dict(case=d["case"], side=d["side"], facts=_facts(d["side"]))
    for i, name in enumerate(names):
        bundle, strict = d["variants"][name]
        R, S, extra = tr.reference(prm, prob, d["side"], bundle, strict, heavy=([j[i] for j in joined], Linvs))
        out[name] = dict(R=R, S=S, extra=extra, bundle=bundle, strict=strict)
    if "nine" in d:
        R9, S9 = d["nine"]
        ck = rr.c_kernel()
        absb = {k: ck[k] * np.asarray(S9[k], dtype=np.float64) for k in tr.BUNDLE_KEYS}
        out["default"]["B"] = tr.scales(prm, prob, d["side"], [np.abs(tr.f64(x)) for x in Linvs], absb, const=False)
    return out


def _own_case(tag):
    """A tail-only or small-model case from nothing, in one worker: it needs nothing of the row-pass references."""
    t0 = time.time()
    if tag in TAIL_ONLY:
        c = tail_only_case(tag)
        d = dict(case=c[:5], side=rr.u_side(c[0], c[1], c[4]), variants={"default": (c[5], False)})
    else:
        c = small_case(tag)
        cache = {}
        R9, S9 = rr.reference(*c, cache=cache)
        d = dict(case=c, side=cache["side"], variants={"default": (rr.pack_bundle(R9, c[1]), False)}, nine=(R9, S9))
    Linvs, joined = [], []
    for q, u in enumerate(d["side"]):
        H = tr.as_ld(tr.sym_lower(rr.split_bundle(d["variants"]["default"][0], d["case"][1])["H"][q]))
        Linv, jobs = tr.heavy_jobs(u, [(H, False)], block=1 << 30)
        Linvs.append(Linv), joined.append(tr.heavy_join([tr.heavy_rows(j) for j in jobs], 1)[0])
    out = _complete(tag, d, Linvs, joined)
    out["seconds"] = time.time() - t0
    return tag, out


_REFS = {}


def references():
    """{tag: {variant: dict(R, S, extra, bundle, strict[, B]), "case": (prm, prob, X, Y, rungs), "side", "facts"}}; variants: "default"
    everywhere, "bs", "strict" and "strict2" (the two-solve form) on D.  Built on first use.  The tail-only and small-model cases are whole jobs of their own in the
    pool that forms the products of A-F by row ranges."""
    if _REFS:
        return _REFS
    t0 = time.time()
    n = max(1, min(16, os.cpu_count() or 1))
    refs = rc.references()
    t1 = time.time()
    size = dict({t: M for t, (M, _) in TAIL_ONLY.items()}, **SMALL)
    with multiprocessing.get_context("spawn").Pool(n) as pool:
        own = [pool.apply_async(_own_case, (tag,)) for tag in sorted(size, key=lambda t: -size[t])]
        todo = {}          # tag -> dict(case, side, variants {name: (bundle, strict)})
        for tag in rc.BASE_TAGS:
            v = {"default": (dense_bundle(refs, tag), False)}
            if tag == "D":
                v["bs"] = (dense_bundle(refs, tag, "bs"), False)
                v["strict"] = (dense_bundle(refs, tag, "strict"), True)
                v["strict2"] = (dense_bundle(refs, tag, "strict2"), "two")          # G = H and Kr = r: no M x M solve
            todo[tag] = dict(case=rc.dense_case(tag), side=refs[tag]["side"], variants=v)
        # the triangular inverses first, the largest first; the row-range jobs of a latent are issued as soon as its inverse is back
        Ls = [((tag, q), u["L"]) for tag, d in todo.items() for q, u in enumerate(d["side"])]
        Ls.sort(key=lambda x: -x[1].shape[0])
        Linv, pending, parts = {}, [], {}
        for (tag, q), inv in pool.imap_unordered(_linv, Ls):
            Linv[(tag, q)] = inv
            d, u = todo[tag], todo[tag]["side"][q]
            Hs = []
            for name in sorted(d["variants"]):
                bundle, strict = d["variants"][name]
                Hs.append((tr.as_ld(tr.sym_lower(rr.split_bundle(bundle, d["case"][1])["H"][q])), strict))
            M = u["L"].shape[0]
            step = M if M < 512 else 128
            base = dict(Ki=u["Kuui"], S=u["S"], L=u["L"], Linv=inv, Li=u["Li"] if any(st for _, st in Hs) else None, Hs=Hs)
            pending += [pool.apply_async(_heavy, (((tag, q), dict(base, r0=r0, r1=min(M, r0 + step))),)) for r0 in range(0, M, step)]
        for p in pending:
            key, out = p.get()
            parts.setdefault(key, []).append(out)
        t2 = time.time()
        for tag, d in todo.items():
            Q = d["case"][1]["Q"]
            joined = [tr.heavy_join(parts[(tag, q)], len(d["variants"]))[0] for q in range(Q)]
            _REFS[tag] = _complete(tag, d, [Linv[(tag, q)] for q in range(Q)], joined)
        t3 = time.time()
        for p in own:
            tag, out = p.get()
            _REFS[tag] = out
    print("[tail] references of %d cases in %.1f s (row-pass references %.1f s; A-F: products in a pool of %d %.1f s, the rest %.1f s; "
          "tail-only and small cases beside them, longest %.1f s, waited for %.1f s)" % (
              len(_REFS), time.time() - t0, t1 - t0, n, t2 - t1, t3 - t2, max(_REFS[t]["seconds"] for t in list(TAIL_ONLY) + list(SMALL)),
              time.time() - t3))
    return _REFS
