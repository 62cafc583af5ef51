"""GPU: the exact-zero windows mode where its windows really cut (cases: tests/window_cases.py).
  1. tables   `kuf_windows_rows` (the engine's own window kernels) equals the float64 restatement of tests/window_ref.py integer for
              integer, and every non-zero the hot-path `rbf_kernel` produces lies inside its tile's row window and its block's row hull;
  2. elements a windows engine on every case and variant through `rowpass_ref.check` against the extended-precision reference, every
              element of the bundle and of q(f) -- and a dense engine through the same check, so that a failure names the mode or the case;
  3. empty    W3: the rows of the tile with the empty window give m == 0.0 and the dense engine's v bit for bit; the rows and columns of
              H and the entries of r and dZ of the column block no tile touches are exact zeros;
  4. stale    the reductions are deterministic, so a windows engine gives the same bits whatever it evaluated before -- after an
              evaluation that filled the whole K^ workspace with large numbers, after moved inducing points, a row shard, an E-step;
  5. fallback W1s (unsorted rows) through 2., its tables the full ranges.
Every check-2 test prints its worst ratios as `[rowpass] <case> <kind> ...`."""
import numpy as np
import pytest

import rowpass_ref as rr
import window_cases as wc
import window_ref as wr
from model_cases import KEYS

pytestmark = pytest.mark.gpu

KINDS = rr.BUNDLE_KINDS + ("m", "v")      # (every segment is a pool of its own: the inner-protocol export, which needs one pool, is left out)


@pytest.fixture(scope="module")
def refs():
    return wc.references()


def engine(tag, **kw):
    from hetmogp_amd.engine import Engine
    prm, prob, X, Y, _ = wc.banded_case(tag)
    e = Engine(prob["specs"], prob["Q"], prob["M"], prob["P"], **kw)
    e.set_data(X, Y)
    return e


def evaluate(e, tag, prm=None, predict=True, healthy=True, **kw):
    """One evaluation at the forced rung through the split step -> the bundle by kind, q(f) of the evaluated rows, and every output of
    hmogp_step_finish (KEYS), all as copies."""
    prm0, prob, X, Y, rungs = wc.banded_case(tag)
    prm = prm0 if prm is None else prm
    T, Df = prob["T"], prob["Df"]
    args = dict(Z=prm["Z"], m_u=prm["m_u"], L_flat=prm["L_flat"], variance=prm["variance"], lengthscale=prm["lengthscale"],
                W=prm["W"], kappa=prm["kappa"], forced_rung=rungs)
    args.update(kw)
    e.step_begin(**args)
    stats = e.stats_read()
    out = e.step_finish()
    assert out["rungs"] == rungs
    if healthy:
        assert not out["v_negative"]
    got = {k: np.array(v, copy=True) for k, v in rr.split_bundle(stats, prob).items()}
    got["out"] = {k: np.array(out[k], copy=True) for k in KEYS}
    if predict:
        b = kw.get("row_begin") or [0] * T
        en = kw.get("row_end") or [x.shape[0] for x in X]
        got["m"], got["v"] = [None] * Df, [None] * Df
        for t in range(T):
            m, v = e.predict_f(X[t][b[t]:en[t]])
            for d in range(Df):
                if prob["f_index"][d] == t:
                    got["m"][d], got["v"][d] = m[:, d].copy(), v[:, d].copy()
    return got


def same_bits(what, a, b, kinds=KINDS):
    for k in kinds:
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        for i, (x, y) in enumerate(zip(xs, ys)):
            assert np.array_equal(np.asarray(x), np.asarray(y)), (what, "not bit-identical", k, i)
    for k in KEYS:
        assert np.array_equal(a["out"][k], b["out"][k]), (what, "not bit-identical", k)


# ------------------------------------------------------------------------------------------------ 1. tables
def launches():
    out = []
    for tag in wc.CASES:
        for t, q, X, Z, ell in wc.window_inputs(tag):
            out.append(("%s t%d q%d" % (tag, t, q), tag, X, Z, ell))
    for t, q, X, Z, ell in wc.window_inputs("W1", *wc.W1_SHARD):
        out.append(("W1 shard t%d q%d" % (t, q), "W1", X, Z, ell))
    for t, q, X, Z, ell in wc.window_inputs("W1"):
        for b, e in wc.segments(X.shape[0], wc.W1_CHUNK_ROWS):
            out.append(("W1 rows %d:%d t%d q%d" % (b, e, t, q), "W1", X[b:e], Z, ell))
    for t, q, X, Z, ell in wc.uniform_shuffle():
        out.append(("W1 uniform shuffle t%d q%d" % (t, q), "W1u", X, Z, ell))
    return out


def test_window_tables_equal_the_restatement_and_hold_every_nonzero():
    """Check 1 (and the tables of check 5), for every launch of the window kernels the cases give rise to.  One test: a launch takes
    milliseconds.  The comparison is exact: no (tile, column) decision of these cases lies within 1e-7 of the threshold
    (tests/test_windows_cpu.py), so an FMA in d2 += d * d decides nothing."""
    from hetmogp_amd import engine as E
    seen_fallback = 0
    for label, tag, X, Z, ell in launches():
        want = wr.windows(X, Z, ell)
        rw, cw = E.kuf_windows_rows(X, Z, ell)
        assert rw.dtype == np.int32 and cw.dtype == np.int32
        assert np.array_equal(rw, want["rowwin"]), (label, "rowwin", rw.tolist(), want["rowwin"].tolist())
        assert np.array_equal(cw, want["colwin"]), (label, "colwin", cw.tolist(), want["colwin"].tolist())
        n, m = np.nonzero(E.rbf_cross_cov(X, Z, 1.0, ell, exact=False))
        in_row, in_col = wr.inside(rw, cw, n, m)
        assert in_row.all(), (label, "non-zeros outside the row window of their tile", int((~in_row).sum()))
        assert in_col.all(), (label, "non-zeros outside the row hull of their block", int((~in_col).sum()))
        if tag == "W1s" and X.shape[0] > 128:             # 5. the fallback: full ranges
            M = Z.shape[0]
            assert want["fallback"] and np.all(rw == (0, (M + 15) & ~15)) and np.all(cw == (0, X.shape[0])), label
            seen_fallback += 1
    assert seen_fallback == 4


def test_kuf_windows_with_a_leading_dimension_and_refusals():
    """Z read in place from the parameter layout [M, Q P] (ldz = Q P) gives the tables of the contiguous copy; bad arguments are refused."""
    import ctypes as C
    from hetmogp_amd import _lib
    from hetmogp_amd import engine as E
    prm, prob, X, _, _ = wc.banded_case("W4")
    P, Q, M = prob["P"], prob["Q"], prob["M"]
    Zall = np.ascontiguousarray(prm["Z"], dtype=np.float64)
    x = np.ascontiguousarray(X[0], dtype=np.float64)
    dp, ip = _lib.c_double_p, _lib.c_int32_p
    for q in range(Q):
        rw = np.zeros(((x.shape[0] + 127) // 128, 2), dtype=np.int32)
        cw = np.zeros(((M + 127) // 128, 2), dtype=np.int32)
        zq = C.cast(Zall.ctypes.data + 8 * q * P, dp)
        _lib.check(_lib.lib.hmogp_kuf_windows(0, x.ctypes.data_as(dp), x.shape[0], P, zq, Q * P, M, float(prm["lengthscale"][q]),
                                              rw.ctypes.data_as(ip), cw.ctypes.data_as(ip)))
        want = E.kuf_windows_rows(x, Zall[:, q * P:(q + 1) * P], prm["lengthscale"][q])
        assert np.array_equal(rw, want[0]) and np.array_equal(cw, want[1])
    with pytest.raises(_lib.InvalidArgument):
        E.kuf_windows_rows(np.zeros((4, 5)), np.zeros((3, 5)), 1.0)             # P = 5
    with pytest.raises(_lib.InvalidArgument):
        E.kuf_windows_rows(np.zeros((4, 1)), np.zeros((8193, 1)), 1.0)          # M > 8192
    with pytest.raises(_lib.InvalidArgument):
        E.kuf_windows_rows(np.zeros((0, 1)), np.zeros((3, 1)), 1.0)             # no rows


# ------------------------------------------------------------------------------------------------ 2. / 5. element by element
RUNS = [("W1", "default", {}, {}), ("W1", "bs", dict(batch_scale=wc.W1_BATCH_SCALE), {}),
        ("W1", "shard", dict(row_begin=list(wc.W1_SHARD[0]), row_end=list(wc.W1_SHARD[1])), {}),
        ("W1", "default", {}, dict(chunk_rows=wc.W1_CHUNK_ROWS)), ("W1s", "default", {}, {}), ("W2", "default", {}, {}),
        ("W3", "default", {}, {}), ("W4", "default", {}, {})]


@pytest.mark.parametrize("tag,variant,kw,ekw", RUNS, ids=["%s-%s%s" % (r[0], r[1], "-chunk" if r[3] else "") for r in RUNS])
def test_banded_case_vs_extended_precision(refs, tag, variant, kw, ekw):
    """The windows engine and the dense engine, each against R in every element of the bundle and of q(f), under the constants of
    window_cases (the rule of DESIGN 9c over the float64 oracle's own error on these cases)."""
    R, S = refs[tag][variant]
    name = "%s %s%s" % (tag, variant, " chunk_rows=%d" % ekw["chunk_rows"] if ekw else "")
    failed = {}
    for mode, on in (("windows", True), ("dense", False)):
        e = engine(tag, exact_zero_windows=on, **ekw)
        got = evaluate(e, tag, **kw)
        e.close()
        try:
            rr.check("%s %s" % (name, mode), got, R, S, wc.c_kernel_win(), KINDS)
        except AssertionError as err:
            failed[mode] = str(err)[:400]
    assert not failed, ("the mode is at fault" if "dense" not in failed else "the dense engine fails too: the case's conditioning", failed)


# ------------------------------------------------------------------------------------------------ 3. empty windows
def test_W3_empty_row_window_and_untouched_column_block():
    """Task 0 alone (task 1, uniform on [0, 1], would touch every block): rows 512-639 lie at [5, 6], 4 to 5 units -- thousands of
    lengthscales -- from every inducing point, and no row lies within 38.6 lengthscales of the inducing points 128-255."""
    prm, prob, X, _, _ = wc.banded_case("W3")
    M, Q = prob["M"], prob["Q"]
    for q in range(Q):                                   # the premise, from the restatement: tile 4 empty, block 1 untouched
        w = wr.windows(X[0], prm["Z"][:, q:q + 1], prm["lengthscale"][q])
        assert w["rowwin"][4].tolist() == [0, 0] and w["colwin"][1].tolist() == [0, 0] and not w["fallback"]
    kw = dict(row_begin=[0, 0], row_end=[X[0].shape[0], 0])
    ew, ed = engine("W3", exact_zero_windows=True), engine("W3")
    # (first an evaluation that leaves large numbers in every part of the K^ workspace the skipped blocks could be read from)
    # (l = 2000 h and 3000 h: 5 and 8 units, so that the rows at [5, 6] leave non-zeros too)
    evaluate(ew, "W3", prm=wc.hot_params(prm, "W3", cs=(2000.0, 3000.0)), predict=False, healthy=False, **kw)
    got, dense = evaluate(ew, "W3", **kw), evaluate(ed, "W3", **kw)
    ew.close(), ed.close()
    far = slice(512, 640)
    assert np.all(got["m"][0][far] == 0.0), "m of the rows with an empty window"
    assert np.array_equal(got["v"][0][far], dense["v"][0][far]), "v of the rows with an empty window"
    want_v = sum((prm["W"][q, 0] ** 2 + prm["kappa"][q, 0]) * prm["variance"][q] for q in range(Q))
    assert np.all(np.abs(got["v"][0][far] - want_v) <= 4 * 2.0 ** -52 * want_v)       # v = k(x, x): a sum of Q products
    blk = slice(128, 256)
    for q in range(Q):
        assert np.all(got["H"][q][blk, :] == 0.0) and np.all(got["H"][q][:, blk] == 0.0), ("H", q)
        assert np.all(got["r"][q][blk] == 0.0) and np.all(got["dZ"][q][blk] == 0.0), ("r / dZ", q)
    # the touched blocks are not zero: the assertion above is about block 1, not about an empty bundle
    assert all(np.abs(got["H"][q][:128, :128]).max() > 0 and np.abs(got["r"][q][256:]).max() > 0 for q in range(Q))
    # ... and the windows engine stays within the dense engine's reach everywhere (a norm: the element-wise comparison is check 2)
    for k in ("H", "r", "dZ"):
        assert np.max(np.abs(got[k] - dense[k])) <= 1e-9 * np.max(np.abs(dense[k])), k


# ------------------------------------------------------------------------------------------------ 4. stale reads
def _fresh(tag, ekw, **kw):
    e = engine(tag, exact_zero_windows=True, **ekw)
    got = evaluate(e, tag, **kw)
    return e, got


@pytest.mark.parametrize("ekw", [{}, dict(chunk_rows=wc.W1_CHUNK_ROWS)], ids=["one-pool-per-task", "chunk_rows=512"])
def test_windows_engine_gives_the_same_bits_whatever_it_evaluated_before(ekw):
    """One engine through: W1 with l = (16, 100) h and variance x 1000 (every entry of the K^ workspace a large non-zero), W1, W1 with
    the inducing points moved by +0.2, W1 under the row shard, W1 again, an E-step (GROUP_QU), predict_f on 16 rows -- each result equal,
    bit for bit, to that of an engine that evaluated nothing before.  `rbf_kernel` leaves the blocks outside a tile's window unwritten:
    a consumer reading one group too far would pick up what the evaluation before left there.  With chunk_rows = 512 the segments of a
    task overwrite one another at offset 0 as well."""
    from hetmogp_amd import _lib
    prm, prob, X, _, _ = wc.banded_case("W1")
    shifted = dict(prm, Z=prm["Z"] + wc.W1_Z_SHIFT)
    shard = dict(row_begin=list(wc.W1_SHARD[0]), row_end=list(wc.W1_SHARD[1]))
    estep = dict(group_mask=_lib.GROUP_QU, predict=False)
    x16 = X[0][500:516]
    e = engine("W1", exact_zero_windows=True, **ekw)
    evaluate(e, "W1", prm=wc.hot_params(prm), predict=False, healthy=False)
    seq = [("W1", {}), ("W1 with Z + 0.2", dict(prm=shifted)), ("W1 row shard", shard), ("W1 again", {}), ("E-step", estep)]
    for what, kw in seq:
        got = evaluate(e, "W1", **kw)
        f, want = _fresh("W1", ekw, **kw)
        same_bits(what, got, want, kinds=KINDS if kw.get("predict", True) else rr.BUNDLE_KINDS)
        if what == "E-step":
            m, v = e.predict_f(x16)
            mf, vf = f.predict_f(x16)
            assert np.array_equal(m, mf) and np.array_equal(v, vf), "predict_f on 16 rows"
        f.close()
    e.close()
