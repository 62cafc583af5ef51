"""CPU: the exact-zero windows restated (tests/window_ref.py) and the banded cases of tests/window_cases.py.
For every launch of the window kernels a case gives rise to -- every (task, latent) of W1-W4 and W1s, W1 under the row shard, W1's
segments at chunk_rows = 512, W1 uniformly shuffled:
  (a) the restated windows contain the 50-digit support {r2 <= 1490};
  (b) they contain every non-zero of the float64 exp image;
  (c) no (tile, column) decision is a knife edge: the smallest |d2 / thr - 1| in 50 digits is >= 1e-7, so a device that contracts
      d2 += d * d into an FMA takes the same decisions and the integer comparison of the GPU test is exact;
  (d) the cases are not vacuous: the windows cut (coverage), W3 has an empty row window and an empty column hull per latent without
      the fallback, W1s falls back, W2's long latent is full.
The float64 oracle against the extended-precision references of these cases is the measurement behind window_cases.C_ORACLE_WIN."""
import numpy as np
import pytest

import rowpass_ref as rr
import window_cases as wc
import window_ref as wr
from test_rowpass_ref_cpu import oracle_outputs


def launches():
    """[(label, X rows, Z_q, lengthscale_q)] of every window launch the GPU tests compare."""
    out = []
    for tag in wc.CASES:
        for t, q, X, Z, ell in wc.window_inputs(tag):
            out.append(("%s t%d q%d" % (tag, t, q), X, Z, ell))
    for t, q, X, Z, ell in wc.window_inputs("W1", *wc.W1_SHARD):
        out.append(("W1 shard t%d q%d" % (t, q), X, Z, ell))
    for t, q, X, Z, ell in wc.window_inputs("W1"):
        for b, e in wc.segments(X.shape[0], wc.W1_CHUNK_ROWS):
            out.append(("W1 rows %d:%d t%d q%d" % (b, e, t, q), X[b:e], Z, ell))
    for t, q, X, Z, ell in wc.uniform_shuffle():
        out.append(("W1 uniform shuffle t%d q%d" % (t, q), X, Z, ell))
    return out


LAUNCHES = launches()


@pytest.fixture(scope="module")
def refs():
    return wc.references()


@pytest.mark.parametrize("label,X,Z,ell", LAUNCHES, ids=[x[0] for x in LAUNCHES])
def test_windows_contain_the_support_and_no_decision_is_a_knife_edge(label, X, Z, ell):
    w = wr.windows(X, Z, ell)
    N, M = X.shape[0], Z.shape[0]
    rw, cw = w["rowwin"], w["colwin"]
    # the shape of the tables: 16-column granularity, the cap, row hulls on the tile grid
    assert np.all(rw % 16 == 0) and np.all(rw[:, 0] <= rw[:, 1]) and rw.max() <= ((M + 15) & ~15)
    assert np.all(cw[:, 0] % 128 == 0) and np.all((cw[:, 1] % 128 == 0) | (cw[:, 1] == N)) and cw.max() <= N
    # (a) the 50-digit support
    sup, near = wr.exact_support(X, Z, ell)
    n, m = np.nonzero(sup)
    in_row, in_col = wr.inside(rw, cw, n, m)
    assert in_row.all() and in_col.all(), (label, "support outside the windows", int((~in_row).sum()), int((~in_col).sum()))
    # (b) the float64 exp image
    n, m = np.nonzero(wr.exp_image(X, Z, ell))
    in_row, in_col = wr.inside(rw, cw, n, m)
    assert in_row.all() and in_col.all(), (label, "non-zeros outside the windows", int((~in_row).sum()), int((~in_col).sum()))
    assert n.size >= sup.sum()
    # (c) the margin
    margin, where = wr.smallest_margin(X, Z, ell)
    print("[windows] %-28s coverage %.3f fallback %d smallest |d2 / thr - 1| = %.3g at (tile, column) %s; %d pairs decided in 50 digits" % (
        label, wr.coverage(rw, M), w["fallback"], margin, where, near))
    assert margin >= 1e-7, (label, margin, where)
    # the nesting the consumers rely on: `rbf_kernel` writes block cb of tile T only if T's row window overlaps the block, the Gram and
    # the column statistics read block cb on every row of its hull -- so every tile inside a hull must have written the block; and a
    # tile that hit a block lies inside the block's hull
    for cb in range(cw.shape[0]):
        for T in range(cw[cb, 0] >> 7, (cw[cb, 1] + 127) >> 7):
            assert rw[T, 0] < (cb + 1) * 128 and cb * 128 < rw[T, 1], (label, "block read but not written", T, cb)
        for T in np.flatnonzero(w["blockhit"][:, cb]):
            assert cw[cb, 0] <= T * 128 and min(N, (T + 1) * 128) <= cw[cb, 1], (label, "hit outside the hull", T, cb)


def _facts(tag):
    M = wc.CASES[tag]["M"]
    return {(t, q): (wr.windows(X, Z, ell), M) for t, q, X, Z, ell in wc.window_inputs(tag)}


def test_cases_are_not_vacuous():
    """(d), from the restatement alone."""
    cov = {}
    for tag in wc.BANDED_TAGS:
        for (t, q), (w, M) in _facts(tag).items():
            cov[tag, t, q] = wr.coverage(w["rowwin"], M)
            assert not w["fallback"], (tag, t, q)
    print("[windows] coverage of task 0: " + "  ".join("%s %s" % (tag, " / ".join("%.2f" % cov[tag, 0, q] for q in range(2)))
                                                        for tag in wc.BANDED_TAGS))
    for q in range(2):
        assert cov["W1", 0, q] <= 0.45 and cov["W3", 0, q] <= 0.45 and cov["W4", 0, q] <= 0.5
    assert cov["W2", 0, 0] <= 0.45
    # W2's long latent is full, on every task
    for (t, q), (w, M) in _facts("W2").items():
        if q == 1:
            assert np.all(w["rowwin"] == (0, 304)) and cov["W2", t, q] == 1.0 and not w["fallback"]
            assert np.all(w["colwin"][:, 0] == 0) and np.all(w["colwin"][:, 1] == wc.CASES["W2"]["Ns"][t])
    # W3: an empty row window and an empty column hull per latent, no fallback
    for q in range(2):
        w, _ = _facts("W3")[0, q]
        empty_rows = np.flatnonzero(w["rowwin"][:, 1] == 0)
        empty_cols = np.flatnonzero(w["colwin"][:, 1] == 0)
        assert empty_rows.tolist() == [4] and empty_cols.tolist() == [1] and not w["fallback"], (q, empty_rows, empty_cols)
        assert w["raw_colwin"][1, 0] == wr.UNSET                                 # left at its initial value by every tile
    # W1s falls back wherever a launch has more than one tile (one tile alone cannot violate a hull)
    for (t, q), (w, M) in _facts("W1s").items():
        N = wc.CASES["W1s"]["Ns"][t]
        assert w["fallback"] == (N > 128), (t, q)
        if w["fallback"]:
            assert np.all(w["rowwin"] == (0, 384)) and np.all(w["colwin"] == (0, N))
            assert wr.coverage(w["raw_rowwin"], M) < 0.6                          # ... and not because its windows were full anyway
    # the uniform shuffle: nearly full windows WITHOUT the fallback
    for t, q, X, Z, ell in wc.uniform_shuffle():
        w = wr.windows(X, Z, ell)
        assert not w["fallback"] and wr.coverage(w["rowwin"], 384) > 0.9


def test_restatement_edges():
    """NaNs count as hits, an empty tile gives [0, 0), the cap is (M + 15) & ~15, hulls follow the tile grid."""
    Z = np.linspace(0, 1, 300)[:, None]
    X = np.sort(np.random.RandomState(3).rand(300, 1), axis=0)
    ell = 0.5 / 299
    w = wr.windows(X, Z, ell)
    assert w["rowwin"][-1, 1] == 304 and w["colwin"][-1, 1] == 300 and not w["fallback"]
    Xn = X.copy()
    Xn[130] = np.nan                                       # a NaN row: its tile hits every column; the hull of block 0 then skips no tile
    wn = wr.windows(Xn, Z, ell)
    assert wn["hit"][1].all() and wn["rowwin"][1].tolist() == [0, 304]
    Zn = Z.copy()
    Zn[299] = np.nan                                       # a NaN inducing point is hit by every tile -> tile 0's window spans all columns
    wz = wr.windows(X, Zn, ell)
    assert wz["hit"][:, 299].all() and wz["rowwin"][0].tolist() == [0, 304]
    Xf = X.copy()
    Xf[256:] += 10.0                                       # the last tile far from every inducing point
    wf = wr.windows(Xf, Z, ell)
    assert wf["rowwin"][2].tolist() == [0, 0] and not wf["fallback"]
    assert not wr.exp_image(Xf, Z, ell)[256:].any()


_ORACLE = {}


def oracle_default(tag):
    if tag not in _ORACLE:
        _ORACLE[tag] = oracle_outputs(*wc.banded_case(tag))
    return _ORACLE[tag]


@pytest.mark.parametrize("tag", sorted(wc.CASES))
def test_oracle_within_c_oracle_win(refs, tag):
    """The float64 oracle against R on the banded cases, every kind, every element: the measurement behind C_ORACLE_WIN."""
    prm, prob, X, Y, rungs = wc.banded_case(tag)
    R, S = refs[tag]["default"]
    print("[windows] %s cond(K_uu + jitter) = %s" % (tag, " ".join("%.1f" % c for c in refs[tag]["facts"]["cond"])))
    rr.check("oracle " + tag, oracle_default(tag), R, S, wc.C_ORACLE_WIN, rr.KINDS)
    for name, kw in wc.VARIANTS.get(tag, {}).items():
        kw = dict(kw)
        if "batch_scale" in kw:
            kw["bs"] = kw.pop("batch_scale")
        rr.check("oracle %s %s" % (tag, name), oracle_outputs(prm, prob, X, Y, rungs, **kw), *refs[tag][name], wc.C_ORACLE_WIN, rr.KINDS)


def test_criterion_still_rejects_indexing_corruptions_under_the_wider_constants(refs):
    """C_KERNEL_WIN is 2^10 to 2^18 times C_KERNEL (the float64 K^ is that far from the exact one at these lengthscales).  Seeded
    corruptions of the ORACLE's output of W1 (arithmetic on arrays: nothing is run wrongly), each what a wrong window or index would
    leave behind, must still land beyond it: a Gram tile next to the diagonal never written, dZ of two adjacent inducing points
    exchanged.  (What these constants cannot see -- entries near e^-700 dropped by a window one group too narrow, a stale read where
    an exact zero belongs -- is what the integer tables, the exact zeros and the bit comparisons of the GPU file are for.)"""
    R, S = refs["W1"]["default"]
    clean = oracle_default("W1")
    CK = wc.c_kernel_win()
    q = 1
    reached = []
    bad = dict(clean, H=clean["H"].copy())
    bad["H"][q][128:256, 0:128] = 0.0
    bad["H"][q][0:128, 128:256] = 0.0
    reached.append(("H tile (1, 0) not written", "H", bad))
    bad = dict(clean, dZ=clean["dZ"].copy())
    bad["dZ"][q, [200, 201]] = clean["dZ"][q, [201, 200]]
    reached.append(("dZ columns exchanged", "dZ", bad))
    for what, kind, got in reached:
        ratio = rr.worst_ratios(got, R, S, (kind,))[kind][0]
        print("[windows] corruption %-32s %-5s ratio %.3g (C_KERNEL_WIN = %g)" % (what, kind, ratio, CK[kind]))
        assert ratio > CK[kind], (what, ratio)


def test_constants_follow_the_rule():
    ck = wc.c_kernel_win()
    for k in rr.KINDS:
        c = wc.C_ORACLE_WIN[k]
        assert c >= rr.C_ORACLE[k] and np.log2(c) == int(np.log2(c))
        assert ck[k] == max(16.0, 4.0 * c)
    assert not wc.KERNEL_EXCEPTIONS


def test_reference_build_is_no_longer_than_the_dense_cases(refs):
    """Printed the same way as tests/rowpass_cases.py prints its own; the per-case seconds are recorded in DESIGN 9u."""
    secs = {t: refs[t]["facts"]["seconds"] for t in refs}
    print("[windows] reference seconds per case: " + " ".join("%s %.1f" % kv for kv in sorted(secs.items())))
    assert set(secs) == set(wc.CASES)
