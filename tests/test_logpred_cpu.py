"""CPU: the deterministic log predictive density of DESIGN 9j -- the float64 restatement (tests/logpred_ref.py) against the 50-digit grid
tests/golden/lpgrid.npz, the grid's regeneration, closed forms and exact limits, the accuracy envelope of the fixed rule against the integral
itself, and the two new C-ABI symbols."""
import ctypes
import os
import sys

import numpy as np
import pytest
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import likgrid as lg            # noqa: E402
import logpred_ref as lr        # noqa: E402

LIB = os.path.join(ROOT, "hetmogp_amd", "libhetmogp_hip.so")
ENVELOPE_SEED = 9000
ENVELOPE_ROWS = {1: 256, 2: 64, 3: 64}       # by the family's dimensions: the 20-node rules are cheap, their dense integral too
BANDS = ((0.0, 0.25), (0.25, 1.0), (1.0, 4.0))


def _y(b, rows=None):
    y = b.y if rows is None else b.y[rows]
    return y[:, 0] if y.shape[1] == 1 else y


@pytest.fixture(scope="module")
def grid():
    return lr.load_grid()


def test_grid_covers_every_family_and_stays_small(grid):
    assert sorted({b.name for b in grid}) == sorted(lr.FAMILIES)
    assert os.path.getsize(lr.GRID) < lg.SIZE_BOUND
    for name in lr.FAMILIES:
        cls = np.concatenate([b.cls for b in grid if b.name == name])
        assert (cls == lr.BULK).any() and (cls == lr.EDGE).any(), name
    gamma = next(b for b in grid if b.tag == "gamma")
    assert np.isneginf(gamma.R[:, 0]).sum() == 1 and np.isnan(gamma.R[:, 1]).sum() == 1     # the all-nodes-zero row
    assert all(np.isposinf(b.R[:, 1]).all() for b in grid if b.name == "Gaussian")


def test_oracle_against_grid(grid):
    """logpred_ref within C_ORACLE of the 50-digit value on every element; only the class where R is -inf / NaN / +inf."""
    for b in grid:
        a, e = lr.lpd(b.name, _y(b), b.m, b.v, **b.kw)
        lr.assert_block(a, e, b, lr.c_oracle(b.name), "logpred_ref %s" % b.tag)
        S = lr.lpd_scale(b.name, _y(b), b.m, b.v, **b.kw)
        fin = np.isfinite(b.R[:, 0])
        np.testing.assert_allclose(S[fin], b.S[fin], rtol=1e-6)        # the float64 scale is the grid's


def test_grid_regenerates_bit_for_bit(grid):
    """The rows of every block are what the generator lays out today, and a seeded subset of their 50-digit values comes out bit for bit."""
    import make_logpred_grid as mk
    assert [[b.tag, b.name, b.kw] for b in grid] == [[k[0], k[1], k[2]] for k in mk.BLOCKS]
    rng = np.random.RandomState(77)
    for b, blk in zip(grid, mk.BLOCKS):
        y, m, v, cls = mk.rows_of(blk)
        for want, got in ((y, b.y), (m, b.m), (v, b.v), (cls, b.cls)):
            assert want.shape == got.shape and want.tobytes() == got.tobytes(), b.tag
        few = 1 if lr.default_T(b.name) ** lr.dim_f(b.name, **b.kw) > 1000 else 3
        for i in rng.choice(b.n, size=min(few, b.n), replace=False):
            R, S = mk.value_of(blk, y[i], m[i], v[i])
            assert R.tobytes() == b.R[i].tobytes() and np.float64(S).tobytes() == b.S[i].tobytes(), (b.tag, int(i))


def test_corruption_is_caught(grid):
    """One result moved by 2 C 2^-52 S fails the criterion."""
    b = next(k for k in grid if k.tag == "gamma")
    a, e = lr.lpd(b.name, _y(b), b.m, b.v, **b.kw)
    C = lr.c_oracle(b.name)
    i = int(np.where((b.cls == lr.BULK) & np.isfinite(b.R[:, 0]))[0][3])
    bad = a.copy()
    bad[i] = b.R[i, 0] + 2.0 * C[lr.BULK][0] * lg.EPS * b.S[i]
    with pytest.raises(AssertionError):
        lr.assert_block(bad, e, b, C, "corrupted lpd")
    bad_e = e.copy()
    bad_e[i] = b.R[i, 1] * (1.0 + 2.0 * 4.0 * C[lr.BULK][1] * lg.EPS * b.S[i])
    with pytest.raises(AssertionError):
        lr.assert_block(a, bad_e, b, C, "corrupted ess")


def test_closed_forms_and_limits():
    rng = np.random.RandomState(3)
    n = 40
    # Gaussian: log N(y; m, sigma^2 + v) with the task's sigma
    y, m, v = rng.randn(n), rng.randn(n, 1), np.exp(rng.uniform(-5, 2, (n, 1)))
    for s in (0.5, 2.0):
        a, e = lr.lpd("Gaussian", y, m, v, sigma=s)
        np.testing.assert_allclose(a, stats.norm.logpdf(y, m[:, 0], np.sqrt(s * s + v[:, 0])), rtol=1e-13, atol=1e-13)
        assert np.isposinf(e).all()
    # HetGaussian at v1 = 0: log N(y; m0, v0 + e^m1), exact in v0 (up to 100)
    m, v = rng.uniform(-2, 2, (n, 2)), np.stack([np.exp(rng.uniform(np.log(1e-3), np.log(100.0), n)), np.zeros(n)], 1)
    a, e = lr.lpd("HetGaussian", y, m, v)
    np.testing.assert_allclose(a, stats.norm.logpdf(y, m[:, 0], np.sqrt(v[:, 0] + np.exp(m[:, 1]))), rtol=1e-13, atol=1e-13)
    # every family at v = 0: log p(y | m)
    for name in lr.FAMILIES:
        kw = lr.BULK_KW.get(name, {})
        y, m, _ = lr.bulk_rows(name, n, 11, **kw)
        a, e = lr.lpd(name, y, m, np.zeros_like(m), **kw)
        np.testing.assert_allclose(a, lr.logpdf(name, y, m, **kw), rtol=1e-12, atol=1e-12, err_msg=name)
    # Weibull with k = 1 (f1 = 0) and an observed row is the Exponential value: scale e^f0 there, rate e^f here, so f = -f0 (the nodes mirror)
    m0, v0 = rng.uniform(-2, 2, n), np.exp(rng.uniform(-4, 0, n))
    t = rng.exponential(1.0, n) + 1e-3
    aw, _ = lr.lpd("Weibull", np.stack([t, np.ones(n)], 1), np.stack([m0, np.zeros(n)], 1), np.stack([v0, np.zeros(n)], 1))
    ae, _ = lr.lpd("Exponential", t, -m0[:, None], v0[:, None])
    np.testing.assert_allclose(aw, ae, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("name", lr.FAMILIES)
def test_accuracy_envelope(name):
    """The fixed rule against the integral itself (logpred_ref.dense at two node counts; a row is used where they agree to 1e-4) on seeded bulk
    rows, per band of the largest v of the row.  The envelope is a property of the rule, printed for DESIGN 9j, not a pass criterion.  What
    IS asserted: every row whose error exceeds 1e-2 has ess below the family's LPD_ESS_WARN, so the facade's warning flags it, and that
    constant flags at most 10 % of the rows that are within 1e-4."""
    from hetmogp_amd.likelihoods import lpd_ess_warn
    kw = lr.BULK_KW.get(name, {})
    warn = lpd_ess_warn(name, **kw)
    n = ENVELOPE_ROWS[1 if name == "HetGaussian" else min(lr.dim_f(name, **kw), 3)]
    y, m, v = lr.bulk_rows(name, n, ENVELOPE_SEED + lr.FAMILIES.index(name), **kw)
    a, e = lr.lpd(name, y, m, v, **kw)
    d, _, ok = lr.dense_checked(name, y, m, v, **kw)
    err, vmax = np.abs(a - d), v.max(1)
    assert ok.mean() >= 0.5, (name, "the dense integral settles on %d of %d rows only" % (ok.sum(), len(ok)))
    for lo_, hi_ in BANDS:
        sel = ok & (vmax > lo_) & (vmax <= hi_)
        if sel.any():
            print("[envelope] %-12s v in (%.2g, %.2g]: %3d rows, |rule - integral| max %.1e median %.1e, min ess %6.2f, rows > 1e-2: %2d, "
                  "> 1e-4: %2d" % (name, lo_, hi_, sel.sum(), err[sel].max(), np.median(err[sel]), e[sel].min(), (err[sel] > 1e-2).sum(),
                                   (err[sel] > 1e-4).sum()))
    bad, good = ok & (err > 1e-2), ok & (err <= 1e-4)
    print("[envelope] %-12s rows used %d of %d; largest ess of a row beyond 1e-2: %s (LPD_ESS_WARN %.1f); rows within 1e-4 it flags: %d of %d"
          % (name, ok.sum(), len(ok), "%.3f" % e[bad].max() if bad.any() else "none", warn, (e[good] < warn).sum(), good.sum()))
    assert (e[bad] < warn).all(), (name, err[bad], e[bad])
    assert (e[good] < warn).mean() <= 0.10, (name, "the constant flags more than 10 % of the rows within 1e-4")


def test_abi_symbols():
    """Fails without the feature: the two symbols are new.  ABI version 8 stays."""
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "hmogp_log_predictive_gh") and hasattr(lib, "hmogp_predict_log_density")
    lib.hmogp_abi_version.restype = ctypes.c_int
    assert lib.hmogp_abi_version() == 8
    from hetmogp_amd import _lib
    one = np.zeros(1)
    p = one.ctypes.data_as(_lib.c_double_p)
    assert _lib.lib.hmogp_predict_log_density(None, 0, p, p, 1, 0, p, p) == _lib.E_INVALID          # NULL handle
    import torch
    if not torch.cuda.is_available():
        assert _lib.lib.hmogp_log_predictive_gh(0, _lib.LIK_GAMMA, 0.0, 0, 1, p, p, p, p, p) == _lib.E_NO_DEVICE
        # (an engine cannot be created without a device: hmogp_create itself answers HMOGP_E_NO_DEVICE, so no handle exists to pass)
        from hetmogp_amd import engine
        with pytest.raises(_lib.HetMOGPError) as ei:
            engine.log_predictive_density_rows("Beta", np.full(2, 0.3), np.zeros((2, 2)), np.ones((2, 2)))
        assert ei.value.code == _lib.E_NO_DEVICE
