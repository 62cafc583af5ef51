"""The edges of the weighted Gram's direct main loop (gemm_rowpass.hip, gram_tile: the unscaled operand's fragments straight from
global memory into a ring of registers G_D = 2 k4-steps ahead, the scaled operand as a k-major image at BK = 32, wave tile 16 x 128)
-- element by element against the extended-precision reference of tests/rowpass_ref.py under the per-element bound of DESIGN 9c,
unchanged:

    |got - R| <= C_KERNEL[kind] * 2^-52 * S.

Operands are dense (the recipe of tests/rowpass_cases.py, forced rung 6), so every k4-step of every tile carries numbers that a wrong
ring slot, a fragment consumed before it landed, a row of the 16-row tail that kept its scale or a wrong band of the diagonal deal
moves far beyond the bound.  H of the bundle is the Gram itself; r, dZ and the scalars come from the kernels that run beside it.

Lengthscales: absolute, 0.26 / 0.37 / 0.5 of the input range per latent, for the reason tests/test_forward_bdirect_gpu.py gives (short
pools of the sorted inputs; t = r^2 / 2 l^2 <= 7.4), and the float64 oracle is held to C_ORACLE on every case and pool of this file
(`test_oracle_within_c_oracle_on_these_cases`, CPU).

  * M = 128: one tile, diagonal only (the deal of the eight 16-row bands, 36 of 64 sub-tiles); M = 256: one strictly-lower tile and
    two diagonal ones; M = 384: six tiles, no multiple of 8;
  * Q = 1 and Q = 3: the batch strides of K^, beta and the slabs (the base of the buffer resource);
  * pools (rows -> row ranges, engine_linalg.hip's gram_ksplit; a k-step of the loop is 32 rows, a range a multiple of 16):
      1, 15       one ragged k4-step / four of them, the ring longer than the range, the lane rows clamped to K - 1
      16          the 16-row tail alone (second half of the image at scale 0)
      17, 31      a ragged second half
      32, 33      one full step; one row behind it
      127, 128    four steps, ragged and full; 129: a tail behind four full steps (9 k-steps of 16)
      300         two ranges of 160 + 140 rows: a 16-row tail behind four full steps; a ragged range off the matrix's end
      512         four ranges of 128 rows
      [37, 166)   a shard off the 16-row grid
  * 4200 rows at M = 256, Q = 1: 32 ranges of 9 k-steps (144 rows: every range ends half-way into a step), the ksplit >= 8 XCD branch,
    a last ragged range of 24 rows and two empty ones, which still write their zero slab tile;
  * one strict-mode evaluation at M = 256 over 4200 rows: the Gram of X = K^ Luu^-T runs the same kernel."""
import multiprocessing
import time

import numpy as np
import pytest

import rowpass_ref as rr

SPECS = [("Gaussian", {"sigma": 0.5})]
RUNG = 6
NROWS = 512
SHAPES = [(128, 1), (128, 3), (256, 1), (256, 3), (384, 1), (384, 3)]           # (M, Q)
POOLS = [(0, 1), (0, 15), (0, 16), (0, 17), (0, 31), (0, 32), (0, 33), (0, 127), (0, 128), (0, 129), (0, 300), (0, 512),
         (37, 166)]                                                               # [row_begin, row_end) of the one task
LONG = (256, 1, 4200)                                                             # M, Q, rows: 32 row ranges of 9 k-steps
KINDS = rr.BUNDLE_KINDS
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
    prm, prob, X, Y, rungs = make(*key)
    cache = {}
    if key == LONG:
        out = {"all": rr.reference(prm, prob, X, Y, rungs, cache=cache),
               "strict": rr.reference(prm, prob, X, Y, rungs, strict=True, cache=cache)}
    else:
        out = {p: rr.reference(prm, prob, X, Y, rungs, row_begin=[p[0]], row_end=[p[1]], cache=cache) for p in POOLS}
    return key, out, time.time() - t0


_REFS = {}


@pytest.fixture(scope="module")
def refs():
    """Every reference of this file, computed once in fresh worker processes."""
    if not _REFS:
        keys = [LONG] + [(M, Q, NROWS) for M, Q in sorted(SHAPES, reverse=True)]        # the longest first
        t0 = time.time()
        with multiprocessing.get_context("spawn").Pool(len(keys)) as pool:
            for key, out, sec in pool.imap_unordered(_build, keys):
                _REFS[key] = out
                print("[gram direct] reference M=%d Q=%d n=%d in %.1f s" % (key + (sec,)))
        print("[gram direct] all references in %.1f s" % (time.time() - t0))
    return _REFS


_ENGINES = {}


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for e, _, _, _ in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def engine(key, **kw):
    ek = key + tuple(sorted(kw.items()))
    if ek not in _ENGINES:
        from hetmogp_amd.engine import Engine
        prm, prob, X, Y, rungs = make(*key)
        e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
        e.set_data(X, Y)
        _ENGINES[ek] = (e, prm, prob, rungs)
    return _ENGINES[ek]


def evaluate(key, engine_kw=None, **kw):
    e, prm, prob, rungs = engine(key, **(engine_kw or {}))
    e.step_begin(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                 W=prm["W"], kappa=prm["kappa"], forced_rung=rungs, **kw)
    stats = e.stats_read()
    out = e.step_finish()
    assert out["rungs"] == rungs and not out["v_negative"]
    return rr.split_bundle(stats, prob)


def test_row_ranges_are_the_ones_the_cases_are_named_for():
    """CPU: gram_ksplit (engine_linalg.hip) and the kernel's partition, restated: the ranges the docstring counts on."""
    def ranges(n, M, ks_max=256):
        tiles = (M + 127) // 128
        ntl, ksteps = tiles * (tiles + 1) // 2, (n + 15) // 16
        floor8 = (((4 * 256 + 128 + ntl - 1) // ntl + 7) // 8) * 8
        want = max(floor8, min((8 * 256 + ntl - 1) // ntl, n // 2048), n // 8192)
        want = min(ks_max, max(1, ksteps // 32), want)
        if ntl * want < 256:
            want = max(want, min(ks_max, max(1, ksteps // 8), 256 // ntl))
        ksplit = (want // 8) * 8 if want >= 8 else max(1, want)
        per = (ksteps + ksplit - 1) // ksplit
        return [max(0, min(n, (s + 1) * per * 16) - s * per * 16) for s in range(ksplit)]
    for M in (128, 256, 384):
        assert ranges(300, M) == [160, 140] and ranges(512, M) == [128] * 4
        assert all(ranges(n, M) == [n] for n in (1, 15, 16, 17, 31, 32, 33, 127, 128, 129))
    assert ranges(4200, 256) == [144] * 29 + [24, 0, 0]


@pytest.mark.parametrize("M,Q", SHAPES)
def test_oracle_within_c_oracle_on_these_cases(refs, M, Q):
    """CPU: the float64 oracle against R on every pool of the case -- the cases belong to the family the constants were settled on."""
    from test_rowpass_ref_cpu import oracle_outputs
    key = (M, Q, NROWS)
    prm, prob, X, Y, rungs = make(*key)
    for pool in POOLS:
        got = oracle_outputs(prm, prob, X, Y, rungs, row_begin=[pool[0]], row_end=[pool[1]])
        rr.check("oracle M=%d Q=%d rows [%d, %d)" % (M, Q, pool[0], pool[1]), got, *refs[key][pool], rr.C_ORACLE, KINDS)


def test_oracle_within_c_oracle_on_the_long_case(refs):
    """CPU: the same for the 4200-row case."""
    from test_rowpass_ref_cpu import oracle_outputs
    prm, prob, X, Y, rungs = make(*LONG)
    got = oracle_outputs(prm, prob, X, Y, rungs)
    rr.check("oracle M=256 Q=1 n=4200", got, *refs[LONG]["all"], rr.C_ORACLE, KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("pool", POOLS, ids=lambda p: "rows%d-%d" % p)
@pytest.mark.parametrize("M,Q", SHAPES)
def test_gram_edges_vs_extended_precision(refs, M, Q, pool):
    key = (M, Q, NROWS)
    R, S = refs[key][pool]
    got = evaluate(key, row_begin=[pool[0]], row_end=[pool[1]])
    rr.check("gram direct M=%d Q=%d rows [%d, %d)" % (M, Q, pool[0], pool[1]), got, R, S, rr.c_kernel(), KINDS)


@pytest.mark.gpu
def test_gram_many_short_ranges_vs_extended_precision(refs):
    """4200 rows at M = 256: 29 ranges that end half-way into a step, a ragged one, two empty ones."""
    R, S = refs[LONG]["all"]
    got = evaluate(LONG)
    rr.check("gram direct M=256 Q=1 n=4200", got, R, S, rr.c_kernel(), KINDS)


@pytest.mark.gpu
@pytest.mark.parametrize("M,Q", SHAPES)
def test_gram_same_bits_after_other_pools(M, Q):
    """The 300-row pool, another pool, the 300-row pool again: the same bits (no stale image row or slab tile is read)."""
    key = (M, Q, NROWS)
    a = evaluate(key, row_begin=[0], row_end=[300])
    evaluate(key, row_begin=[37], row_end=[166])
    b = evaluate(key, row_begin=[0], row_end=[300])
    for k in KINDS:
        for (label, x, _, _), (_, y, _, _) in zip(rr.pairs(k, a[k], a[k], a[k]), rr.pairs(k, b[k], b[k], b[k])):
            assert np.array_equal(np.asarray(x), np.asarray(y)), ("not bit-identical", k, label)


@pytest.mark.gpu
def test_strict_mode_gram_of_the_solved_operand(refs):
    """strict_qf=True at M = 256 over 4200 rows: the bundle's H and r hold X^T diag(beta) X and X^T alpha with X = K^ Luu^-T."""
    R, S = refs[LONG]["strict"]
    got = evaluate(LONG, engine_kw=dict(strict_qf=True))
    rr.check("gram direct strict M=256 n=4200", got, R, S, rr.c_kernel(), KINDS)
