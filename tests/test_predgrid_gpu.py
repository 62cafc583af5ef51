"""GPU: `hmogp_predictive` element by element against the high-precision grid tests/golden/predgrid.npz: every family, every
row, both rule orders, |got - R| <= C 2^-52 max(S, 2^-1022) with C = max(16, 4 C_ORACLE_PRED) and the class rule on the rows that
overflow float64 -- and a row's bits do not depend on where it stands in the batch.

Kernel figures, worst |kernel - R| / (2^-52 S) per family, class and output, measured on an MI355X: DESIGN 9o."""
import numpy as np
import pytest

import predgrid as pg

pytestmark = pytest.mark.gpu

G = pg.load()
TAGS = sorted(G)


def _engine_fn(name, m, v, T, **kw):
    from hetmogp_amd import engine
    return engine.predictive(name, m, v, gh_T=T, **kw)


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("tag", TAGS)
def test_predictive_on_the_high_precision_grid(tag):
    g = G[tag]
    for T in g.Ts:
        exc = [(r, c) for (t, r, c) in pg.KERNEL_EXCEPTIONS.get(tag, []) if t == T]
        assert len(exc) <= 0.01 * g.R[T].size and not any(g.cls[r] == pg.BULK for r, _ in exc)
        cex = {(r, c): cl for (t, r, c), cl in pg.KERNEL_CLASS_EXCEPTIONS.get(tag, {}).items() if t == T}
        assert len(exc) + len(cex) <= 0.01 * g.R[T].size and not any(g.cls[r] == pg.BULK for r, _ in cex)
        pg.assert_rows(g, T, g.evaluate(_engine_fn, T), pg.c_kernel(pg.family_key(g)), tag + " kernel", exceptions=exc, class_exceptions=cex)


@pytest.mark.parametrize("tag", TAGS)
def test_row_position_does_not_matter(tag):
    """A row gives the same bits evaluated alone, as the last of 4 k + 1 rows (the wave-per-row kernels put four rows in a block, the
    lane-per-row ones 256 in a ragged last block) and in a permuted batch.  Families with a per-row parameter are launched per value: the
    rows of the most frequent one are used."""
    g = G[tag]
    p = g.param if g.param_name else np.zeros(g.n)
    vals, cnt = np.unique(p, return_counts=True)
    u = vals[np.argmax(cnt)]
    rows = np.where(p == u)[0]
    kw = g.kw(u)
    n = len(rows)
    for T in g.Ts:
        run = lambda idx: np.hstack([np.reshape(a, (len(idx), -1)) for a in _engine_fn(g.name, g.m[rows[idx]], g.v[rows[idx]], T, **kw)])
        base = run(np.arange(n))
        perm = np.random.RandomState(11).permutation(n)
        assert _same_bits(run(perm), base[perm]), (tag, T, "permutation")
        edge = np.where(g.cls[rows] == pg.EDGE)[0]
        probes = np.concatenate([edge[:: max(1, len(edge) // 6)][:6], np.arange(0, n, max(1, n // 6))[:6]])
        for j, r in enumerate(probes):
            assert _same_bits(run(np.array([r])), base[[r]]), (tag, T, "alone", int(r))
            k = (1, 2, 16, 64, 65, 300)[j % 6]
            idx = np.concatenate([(np.arange(4 * k) * 7 + 3 + j) % n, [r]])          # the last of 4 k + 1 rows
            assert _same_bits(run(idx), base[idx]), (tag, T, "last of", 4 * k + 1, int(r))
