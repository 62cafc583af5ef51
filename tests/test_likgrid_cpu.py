"""CPU: the float64 NumPy oracle, row by row, against the high-precision grids tests/golden/likgrid_*.npz -- and the
grids against their generator.  The criterion and its constants live in tests/likgrid.py; the 50-digit restatement in
tests/lik_ref_mp.py (needs mpmath, which the development machines carry: its import is asserted, not skipped)."""
import glob
import os

import numpy as np
import pytest

import likgrid as lg
from oracle import likelihoods_oracle as lo

FILES = lg.grid_files()
IDS = [lg.tag_of(p) for p in FILES]


def oracle_fn(name, y, m, v, exact=False, **kw):
    with np.errstate(all="ignore"):
        return lo.var_exp_all(name, y[:, None], m, v, exact=exact, **kw)


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_oracle_within_c_oracle(path):
    """Every element of every row, no element left out: |oracle - R| <= C_oracle * 2^-52 * S; marked rows by class."""
    g = lg.LikGrid(path)
    got = g.evaluate(oracle_fn)
    lg.assert_rows(got, g.R, g.S, g.nonfinite, g.col_kind(), g.cls, lg.c_oracle(g.name), g.tag + " oracle")
    if g.has_exact:
        got = g.evaluate(oracle_fn, exact=True)
        lg.assert_rows(got, g.R_exact, g.S_exact, g.nonfinite_exact, g.col_kind(), g.cls, lg.c_oracle(g.name, "exact"),
                       g.tag + " oracle, exact mode")


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_grid_sample_recomputed_exactly(path):
    """A fixed 5 % of the rows (every 20th, from row 3) recomputed with the mpmath restatement equals the file bit for bit."""
    try:
        import lik_ref_mp
    except ImportError as e:                             # pragma: no cover
        raise AssertionError("mpmath is needed to check the grids against their generator") from e
    g = lg.LikGrid(path)
    rows = np.arange(3, g.n, 20)
    assert len(rows) >= 1
    for r in rows:
        R, S, Rx, Sx = lik_ref_mp.row_both(g.name, float(g.y[r]), [float(a) for a in g.m[r]], [float(a) for a in g.v[r]],
                                           **g.kw(g.param[r]))
        for got, want in ((R, g.R[r]), (S, g.S[r]), (Rx, g.R_exact[r]), (Sx, g.S_exact[r])):
            assert np.array_equal(got, want, equal_nan=True), (g.tag, int(r), got, want)


@pytest.mark.parametrize("path", FILES + [os.path.join(lg.GOLDEN, "lik_scales.npz")], ids=IDS + ["lik_scales"])
def test_file_within_size_bound(path):
    assert os.path.getsize(path) < lg.SIZE_BOUND


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_grid_shape_and_nonfinite_share(path):
    g = lg.LikGrid(path)
    w = 1 + 2 * g.J
    assert g.R.shape == g.S.shape == g.nonfinite.shape == g.R_exact.shape == g.nonfinite_exact.shape == (g.n, w)
    assert set(np.unique(g.cls)) == {lg.BULK, lg.EDGE}
    for nf, R, S in ((g.nonfinite, g.R, g.S), (g.nonfinite_exact, g.R_exact, g.S_exact)):
        marked = np.any(nf != 0, axis=1)
        assert marked.mean() <= lg.NONFINITE_SHARE, (g.tag, float(marked.mean()))
        assert not np.any(marked & (g.cls == lg.BULK))
        fin = ~marked
        assert np.all(np.isfinite(R[fin])) and np.all(np.isfinite(S[fin])) and np.all(S[fin] >= np.abs(R[fin]) * (1 - 1e-15))


def test_every_family_and_student_nu_has_a_grid():
    names = {lg.LikGrid(p).name for p in FILES}
    assert names == {"Gaussian", "Bernoulli", "HetGaussian", "Poisson", "Exponential", "Gamma", "Beta", "Student", "Categorical"}
    assert {lg.LikGrid(p).kw0.get("K") for p in FILES if "categorical" in p} == {3, 4, 5, 6}
    st = lg.LikGrid(os.path.join(lg.GOLDEN, "likgrid_student.npz"))
    assert set(np.unique(st.param)) == {0.1, 1.0, 2.0, 5.0, 63.9, 64.0, 64.1, 1e3, 1e8}


def test_scales_cover_every_reference_fixture():
    sc = lg.load_scales()
    for path in lg.reference_fixtures():
        key = os.path.basename(path)[:-4]
        f = np.load(path)
        w = 1 + 2 * f["m"].shape[1]
        assert sc[key + "__S"].shape == sc[key + "__R"].shape == (f["y"].shape[0], w)
        assert np.all(sc[key + "__S"] >= np.abs(sc[key + "__R"]) * (1 - 1e-15))
