"""GPU: the per-likelihood quadrature kernels (`lik_device.h` through `hmogp_var_exp_ex`), row by row, against the
high-precision grids tests/golden/likgrid_*.npz: every output element within C * 2^-52 * S of the 50-digit value
of the reference's rule, S the element's own condition scale, C = max(16, 4 C_oracle) per family, output kind and row class
(tests/likgrid.py); rows that overflow after the reference's own clips by class (finite / +inf / -inf / NaN).  And: the
result of a row must not depend on where in the launch it sits."""
import numpy as np
import pytest

import likgrid as lg

pytestmark = pytest.mark.gpu

FILES = lg.grid_files()
IDS = [lg.tag_of(p) for p in FILES]
OFFSETS = (0, 1, 63, 64, 65, 255, 256, 257)
LENGTHS = (1, 63, 64, 65, 257, 1000, 70001)


@pytest.fixture(scope="module")
def E():
    from hetmogp_amd import engine
    return engine


def same_bits(a, b):
    return np.array_equal(np.asarray(a, float).view(np.uint64) | (np.isnan(a) * np.uint64(2 ** 63 - 1)),
                          np.asarray(b, float).view(np.uint64) | (np.isnan(b) * np.uint64(2 ** 63 - 1)))


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_grid_reference_quirks(E, path):
    g = lg.LikGrid(path)
    got = g.evaluate(E.var_exp)
    lg.assert_rows(got, g.R, g.S, g.nonfinite, g.col_kind(), g.cls, lg.c_kernel(g.name), g.tag + " kernel",
                   exceptions=lg.KERNEL_EXCEPTIONS.get((g.tag, "reference"), ()))


@pytest.mark.parametrize("path", [p for p in FILES if lg.LikGrid(p).has_exact], ids=[t for p, t in zip(FILES, IDS) if lg.LikGrid(p).has_exact])
def test_grid_exact_mode(E, path):
    """quirks = "exact": Gamma / Beta without the second division by sqrt(pi) (Q1), Categorical with the true d/dm (Q2)."""
    g = lg.LikGrid(path)
    got = g.evaluate(E.var_exp, quirks="exact")
    lg.assert_rows(got, g.R_exact, g.S_exact, g.nonfinite_exact, g.col_kind(), g.cls, lg.c_kernel(g.name, "exact"),
                   g.tag + " kernel, exact mode", exceptions=lg.KERNEL_EXCEPTIONS.get((g.tag, "exact"), ()))


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_row_position_does_not_matter(E, path):
    """The same rows permuted, and embedded at offsets 0 .. 257 of arrays of 1 .. 70 001 rows filled with other grid rows, give
    bit-identical results per row (per-wave LDS tables of the wave-per-row families, ragged last block of the lane-per-row ones).
    Families with a per-row parameter (sigma, deg_free) are launched per value: the rows of the most frequent one are used."""
    g = lg.LikGrid(path)
    kw, rows = max(g.param_groups(), key=lambda t: len(t[1]))
    y, m, v = g.y[rows], g.m[rows], g.v[rows]
    n = len(rows)
    run = lambda idx: lg.pack(*E.var_exp(g.name, y[idx], m[idx], v[idx], **kw), len(idx))
    base = run(np.arange(n))
    rng = np.random.RandomState(11)
    perm = rng.permutation(n)
    assert same_bits(run(perm), base[perm]), (g.tag, "permutation")
    edge = np.where(g.cls[rows] == lg.EDGE)[0]
    for L in LENGTHS:
        for off in OFFSETS:
            if off >= L:
                continue
            idx = (np.arange(L) * 7 + 3 + off) % n                              # filler: other rows of the grid
            k = min(L - off, 130, n)                                              # a block that crosses a wave and a half
            idx[off:off + k] = np.concatenate([edge, np.arange(n)])[(np.arange(k) * 5 + L) % n]
            assert same_bits(run(idx), base[idx]), (g.tag, "length", L, "offset", off)
