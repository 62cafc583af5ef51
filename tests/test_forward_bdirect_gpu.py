"""The edges of the plain forward's B-direct main loop (gemm_rowpass.hip: C_q's fragments straight from L2 into a ring of
registers BD_D = 2 k4-steps ahead, A image at BK = 32) -- element by element against the extended-precision reference of
tests/rowpass_ref.py under the per-element bound of DESIGN 9c, unchanged:

    |got - R| <= C_KERNEL[kind] * 2^-52 * S.

Operands are dense (the recipe of tests/rowpass_cases.py, forced rung 6), so every k4-step of every column tile carries numbers a
wrong ring slot, a fragment consumed before it landed or a wrong batch stride moves far beyond the bound.  dL_dKmn of the
inner-protocol export carries P~ per element; ve, sgv, r, sa, sl, swk carry the fused row statistics.

Lengthscales.  The pools here are SHORT row ranges of the sorted inputs (down to one row), so an inducing point can be the whole input
range away from every row of the pool.  K^ = exp(-t), t = r^2 / (2 l^2), carries the rounding of t amplified by t itself, which the
condition scale S does not count: with the 16-spacing latent of rowpass_cases (t up to 127 at M = 256) the float64 NumPy oracle is
234 x 2^-52 S away from R in dZ on the one-row pool, C_ORACLE being 4.  Every latent here therefore takes an ABSOLUTE lengthscale (as
case F does) of 0.26, 0.37, 0.5 of the input range: t <= 7.4 for every pair of a row and an inducing point.  Membership in the family
C_ORACLE / C_KERNEL were settled on is checked the way DESIGN 9c defines it -- the float64 oracle within C_ORACLE on every case and
pool of this file (`test_oracle_within_c_oracle_on_these_cases`, CPU).

  * M = 128: one column tile, four k-steps of 32 -- prologue and drain of the fragment ring make up half the loop;
  * M = 256, M = 384: 2 and 3 column tiles, tile counts that are no multiples of 8 (no XCD remap); the 512-row pool makes it 8 tiles
    at M = 256, the remap branch;
  * pools of 1, 127, 128, 129, 300, 512 rows: clamped last rows, a single partial panel, one row beyond a panel, full panels only;
  * Q = 1 and Q = 3: the batch strides of A, C_q (the base of the buffer resource) and P~;
  * a row shard [37, 166) off the 16-row grid;
  * one strict-mode evaluation at M = 256 over 4200 rows: the C -= A B updates of the blocked solves (k-extents that are multiples
    of 16 only) and the unpaired products keep the staged loop, the fs_k / fs_sq epilogues are shared by both."""
import multiprocessing
import time

import numpy as np
import pytest

import rowpass_ref as rr

SPECS = [("Gaussian", {"sigma": 0.5})]
RUNG = 6
NROWS = 512
SHAPES = [(128, 1), (128, 3), (256, 1), (256, 3), (384, 1), (384, 3)]           # (M, Q)
POOLS = [(0, 1), (0, 127), (0, 128), (0, 129), (0, 300), (0, 512), (37, 166)]            # [row_begin, row_end) of the one task
STRICT = (256, 1, 4200)                                                           # M, Q, rows: >= 4096 rows take the update kernel
KINDS = rr.BUNDLE_KINDS + ("dKmn", "dKdiag")
LENGTHSCALES = (0.26, 0.37, 0.5)                                                  # of the input range, per latent (see above)


def make(M, Q, n):
    """(prm, prob, X, Y, forced_rungs): one Gaussian task of n rows, dense K^ (tests/rowpass_cases.py's recipe)."""
    from model_cases import synth
    cs = tuple(f * (M - 1) for f in LENGTHSCALES[:Q])
    prm, prob, X, Y = synth(90 + M + Q, SPECS, [n], M, Q, 1, cs)
    prm["m_u"] = 0.1 * prm["m_u"]
    return prm, prob, X, Y, [RUNG] * Q


def _build(key):
    t0 = time.time()
    M, Q, n = key
    prm, prob, X, Y, rungs = make(M, Q, n)
    cache = {}
    if key == STRICT:
        out = {"strict": rr.reference(prm, prob, X, Y, rungs, strict=True, cache=cache)}
    else:
        out = {p: rr.reference(prm, prob, X, Y, rungs, row_begin=[p[0]], row_end=[p[1]], cache=cache) for p in POOLS}
    return key, out, time.time() - t0


_REFS = {}


@pytest.fixture(scope="module")
def refs():
    """Every reference of this file, computed once in fresh worker processes."""
    if not _REFS:
        keys = [STRICT] + [(M, Q, NROWS) for M, Q in sorted(SHAPES, reverse=True)]      # the longest first
        t0 = time.time()
        with multiprocessing.get_context("spawn").Pool(len(keys)) as pool:
            for key, out, sec in pool.imap_unordered(_build, keys):
                _REFS[key] = out
                print("[bdirect] reference M=%d Q=%d n=%d in %.1f s" % (key + (sec,)))
        print("[bdirect] all references in %.1f s" % (time.time() - t0))
    return _REFS


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e, _, _, _ in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def engine(key, **kw):
    if key not in _ENGINES:
        from hetmogp_amd.engine import Engine
        prm, prob, X, Y, rungs = make(*key)
        e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
        e.set_data(X, Y)
        _ENGINES[key] = (e, prm, prob, rungs)
    return _ENGINES[key]


def evaluate(key, raw=True, **kw):
    e, prm, prob, rungs = engine(key)
    e.step_begin(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                 W=prm["W"], kappa=prm["kappa"], forced_rung=rungs, **kw)
    stats = e.stats_read()
    out = e.step_finish()
    assert out["rungs"] == rungs and not out["v_negative"]
    got = rr.split_bundle(stats, prob)
    if raw:
        n = kw["row_end"][0] - kw["row_begin"][0] if "row_end" in kw else key[2]
        g = e.debug_raw_grads([n])
        got["dKmn"], got["dKdiag"] = g["dL_dKmn"], g["dL_dKdiag"]
    return got


@pytest.mark.parametrize("M,Q", SHAPES)
def test_oracle_within_c_oracle_on_these_cases(refs, M, Q):
    """CPU: the float64 oracle against R on every pool of the case -- the cases belong to the family the constants were settled on."""
    from test_rowpass_ref_cpu import oracle_outputs
    key = (M, Q, NROWS)
    prm, prob, X, Y, rungs = make(*key)
    for pool in POOLS:
        got = oracle_outputs(prm, prob, X, Y, rungs, row_begin=[pool[0]], row_end=[pool[1]])
        rr.check("oracle M=%d Q=%d rows [%d, %d)" % (M, Q, pool[0], pool[1]), got, *refs[key][pool], rr.C_ORACLE, KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "rows%d-%d" % p)
@pytest.mark.parametrize("M,Q", SHAPES)
def test_forward_edges_vs_extended_precision(refs, M, Q, pool):
    key = (M, Q, NROWS)
    R, S = refs[key][pool]
    got = evaluate(key, row_begin=[pool[0]], row_end=[pool[1]])
    rr.check("bdirect M=%d Q=%d rows [%d, %d)" % (M, Q, pool[0], pool[1]), got, R, S, rr.c_kernel(), KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Q", SHAPES)
def test_forward_same_bits_after_other_pools(M, Q):
    """The 300-row pool, another pool, the 300-row pool again: the same bits."""
    key = (M, Q, NROWS)
    a = evaluate(key, row_begin=[0], row_end=[300])
    evaluate(key, row_begin=[37], row_end=[166])
    b = evaluate(key, row_begin=[0], row_end=[300])
    for k in KINDS:
        for (label, x, _, _), (_, y, _, _) in zip(rr.pairs(k, a[k], a[k], a[k]), rr.pairs(k, b[k], b[k], b[k])):
            assert np.array_equal(np.asarray(x), np.asarray(y)), ("not bit-identical", k, label)


@pytest.mark.gpu
def test_strict_mode_keeps_the_staged_loop_users_working(refs):
    """strict_qf=True at M = 256 over 4200 rows: the bundle's H and r hold X^T diag(beta) X and X^T alpha with X = K^ Luu^-T."""
    R, S = refs[STRICT]["strict"]
    engine(STRICT, strict_qf=True)
    got = evaluate(STRICT, raw=False)
    rr.check("bdirect strict M=256 n=4200", got, R, S, rr.c_kernel(), rr.BUNDLE_KINDS)
