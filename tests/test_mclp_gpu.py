"""GPU: the Monte-Carlo log predictive density (`hmogp_log_predictive`: `log_predictive_kernel<LIK>`, `dirichlet_log_predictive_kernel<K>`)
draw by draw and row by row -- every row of tests/golden/mclpgrid.npz against its 50-digit estimate, the generator pinned
draw by draw at S = 1, position and repeatability, a NaN row, and the facade's sum over tasks."""
import numpy as np
import pytest

import mclp_ref as mr

pytestmark = pytest.mark.gpu
BULK, EDGE = mr.BULK, mr.EDGE
EPS = mr.EPS
N_PIN = 200000


def _E():
    from hetmogp_amd import engine
    return engine


@pytest.fixture(scope="module")
def grid():
    return {b.tag: b for b in mr.load_grid()}


TAGS = [b.tag for b in mr.load_grid()]


# ------------------------------------------------------------------------------------------------ every grid row
@pytest.mark.parametrize("tag", TAGS)
def test_grid_every_row(grid, tag):
    """|kernel - R| <= C_KERNEL 2^-52 Sc on every row of every call of the block (S = 1 .. 1000, four seeds, row counts that are no multiple
    of the 4 rows per block); R = -inf is compared exactly -- the rows whose samples have log p = -inf are in `exponential`."""
    E = _E()
    b = grid[tag]
    C = mr.c_kernel(b.name)
    worst = {BULK: 0.0, EDGE: 0.0}
    for c in b.calls:
        got = E.log_predictive_rows(b.name, c.y_arg(), c.m, c.v, num_samples=c.S, seed=c.seed, **b.kw)
        exc = [row for (t, ci, row) in mr.KERNEL_EXCEPTIONS if t == tag and ci == c.index]
        w = mr.assert_call(got, c, C, "kernel %s" % tag, exc)
        worst = {k: max(worst[k], w[k]) for k in worst}
    print("[mclp] %-14s kernel against the grid: bulk %.3g (C_KERNEL %g)  edge %.3g (C_KERNEL %g)" % (tag, worst[BULK], C[BULK], worst[EDGE], C[EDGE]))


def test_kernel_exceptions_are_named_and_few(grid):
    """Expected to be empty.  Otherwise: every element named with its cause, at most 1 % of the rows, no bulk row, no -inf row."""
    total = sum(len(b.cls) for b in grid.values())
    assert len(mr.KERNEL_EXCEPTIONS) <= total // 100
    for (tag, ci, row), cause in mr.KERNEL_EXCEPTIONS.items():
        c = grid[tag].calls[ci]
        assert cause and c.cls[row] == EDGE and np.isfinite(c.R[row])


# ------------------------------------------------------------------------------------------------ draw by draw
def _pin(name, y, m, v, seed, what, **kw):
    E = _E()
    got = E.log_predictive_rows(name, y, m, v, num_samples=1, seed=seed, **kw)
    want = mr.estimate(name, y, m, v, 1, seed, **kw)
    Sc = mr.scale(name, y, m, v, 1, seed, **kw)
    C = mr.c_sum(name)[BULK]
    r = np.abs(got - want) / (EPS * Sc)
    print("[mclp] draw-by-draw %-34s %d rows: %.1f %% equal to the bit, worst |kernel - float64| / (2^-52 Sc) = %.3g (bound %g)" % (
        what, len(got), 100.0 * np.mean(got == want), r.max(), C))
    assert np.isfinite(got).all()
    assert (r <= C).all(), (what, int(r.argmax()), r.max())
    return got


def test_draw_by_draw_gaussian_z0():
    """S = 1: out = -log(2 pi)/2 - (y - m - sqrt(v) z0)^2 / 2, z0 of pair 0, one row per draw."""
    rng = np.random.RandomState(901)
    m, v = rng.uniform(-3, 3, (N_PIN, 1)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N_PIN, 1)))
    got = _pin("Gaussian", m[:, 0] + 2.0 + rng.randn(N_PIN), m, v, 2 ** 63 + 5, "Gaussian (z0 of pair 0)", sigma=0.5)
    assert np.unique(got).size > 0.99 * N_PIN


def test_draw_by_draw_hetgaussian_z1():
    """S = 1, v0 = 0, y = m0: out = -log(2 pi)/2 - f1 / 2, f1 = m1 + sqrt(v1) z1 of pair 0."""
    rng = np.random.RandomState(902)
    m, v = rng.uniform(-3, 3, (N_PIN, 2)), np.exp(rng.uniform(np.log(1e-3), np.log(4.0), (N_PIN, 2)))
    v[:, 0] = 0.0
    got = _pin("HetGaussian", m[:, 0].copy(), m, v, 1, "HetGaussian v0 = 0 (z1 of pair 0)")
    z1 = mr.draws(1, np.arange(N_PIN), 1, 2)[:, 0, 1]
    want = -0.5 * np.log(2.0 * np.pi) - 0.5 * (m[:, 1] + np.sqrt(v[:, 1]) * z1)
    scale = 1.0 + np.abs(want) + 0.5 * (np.abs(m[:, 1]) + 4.0 * np.sqrt(v[:, 1]) * np.abs(z1))
    assert (np.abs(got - want) <= mr.c_sum("HetGaussian")[BULK] * EPS * scale).all()      # the closed form: z1 alone, in f1 alone


@pytest.mark.parametrize("j", range(8))
def test_draw_by_draw_categorical_k9(j):
    """S = 1, K = 9 (J = 8 = HMOGP_MAXJ), v non-zero in dimension j alone, the label j + 1: member j & 1 of pair j >> 1."""
    rng = np.random.RandomState(910 + j)
    m = rng.uniform(-3, 3, (N_PIN, 8))
    v = np.zeros((N_PIN, 8))
    v[:, j] = np.exp(rng.uniform(np.log(1e-3), np.log(4.0), N_PIN))
    _pin("Categorical", np.full(N_PIN, j + 1.0), m, v, 2 ** 32, "Categorical K = 9, v_%d alone (pair %d member %d)" % (j, j >> 1, j & 1), K=9)


# ------------------------------------------------------------------------------------------------ position and repeatability
@pytest.mark.parametrize("tag", ["poisson", "weibull", "binomial", "dirichlet3", "categorical6"])
def test_position_and_repeatability(grid, tag):
    """A row's bits depend on (its inputs, its index, the seed, S) alone: the S = 65 call's rows in front of a longer call (another N, so
    another stride of the [2][N] / [3][N] / [K][N] image and another grid) keep their bits; moved to other indices they draw differently;
    two identical calls are bit-identical."""
    E = _E()
    b = grid[tag]
    c = next(k for k in b.calls if k.S == 65)
    long = next(k for k in b.calls if k.S == 1)
    y, m, v = np.concatenate([c.y, long.y, c.y]), np.concatenate([c.m, long.m, c.m]), np.concatenate([c.v, long.v, c.v])
    ya = y[:, 0] if y.shape[1] == 1 else y
    a0 = E.log_predictive_rows(b.name, c.y_arg(), c.m, c.v, num_samples=c.S, seed=c.seed, **b.kw)
    a1 = E.log_predictive_rows(b.name, c.y_arg(), c.m, c.v, num_samples=c.S, seed=c.seed, **b.kw)
    full = E.log_predictive_rows(b.name, ya, m, v, num_samples=c.S, seed=c.seed, **b.kw)
    assert np.array_equal(a0, a1, equal_nan=True)
    assert np.array_equal(full[:c.n], a0, equal_nan=True)                      # same index, same seed: same bits
    moved = full[c.n + long.n:]
    bulk = c.cls == BULK
    assert (moved[bulk] != a0[bulk]).all()                                     # same inputs at another index: other draws
    if tag != "binomial":                                                      # (no float64 scale is stated for Binomial)
        rows = np.arange(c.n + long.n, 2 * c.n + long.n)
        want = mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, rows=rows, **b.kw)
        Sc = mr.scale(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, rows=rows, **b.kw)
        assert (np.abs(moved - want) <= mr.c_sum(b.name)[EDGE] * EPS * Sc).all()   # the moved rows are the restatement's at their new indices
    other = E.log_predictive_rows(b.name, c.y_arg(), c.m, c.v, num_samples=c.S, seed=c.seed + 1, **b.kw)
    assert (other[bulk] != a0[bulk]).all()


# ------------------------------------------------------------------------------------------------ NaN
@pytest.mark.parametrize("S", [1, 65, 1000])
def test_nan_mean_gives_nan(grid, S):
    """The entry point accepts a NaN in m (it checks y alone): that row's every sample has log p = NaN and the row is NaN -- not -inf, which
    is what a row of samples with p = 0 gives --, the rows beside it keep their bits.  Gaussian and Poisson: their log p is linear in f
    somewhere.  (A family whose f passes only through safe_exp / clip, Dirichlet for one, turns a NaN f into the clip's bound -- fmin and
    fmax drop a NaN -- so the Dirichlet kernel's NaN branch cannot be reached through the entry point, which also refuses a NaN y.)"""
    E = _E()
    for tag in ("poisson", "gaussian"):
        b = grid[tag]
        c = next(k for k in b.calls if k.S == 65)
        m = c.m.copy()
        m[1, 0] = np.nan
        clean = E.log_predictive_rows(b.name, c.y_arg(), c.m, c.v, num_samples=S, seed=3, **b.kw)
        got = E.log_predictive_rows(b.name, c.y_arg(), m, c.v, num_samples=S, seed=3, **b.kw)
        assert np.isnan(got[1]), (tag, S, got[1])
        keep = np.arange(c.n) != 1
        assert np.array_equal(got[keep], clean[keep])


# ------------------------------------------------------------------------------------------------ the facade
def test_facade_sums_tasks_with_seed_plus_task():
    """HetLikelihood.negative_log_predictive = -sum_t (1 / num_samples) sum_n est_t[n] with the seed of task t = seed + t
    (the reference's 1 / num_samples factor on the sum over test points included); tolerance: the rows' summed bounds."""
    from hetmogp_amd import likelihoods as L
    rng = np.random.RandomState(77)
    N, S, seed = 203, 100, 41
    specs = [("Bernoulli", {}), ("HetGaussian", {})]
    Y, M, V = [], [], []
    for name, kw in specs:
        y, m, v = mr.lr.bulk_rows(name, N, rng.randint(1 << 30), **kw)
        Y.append(np.asarray(y, float).reshape(N, -1)), M.append(m), V.append(v)
    het = L.HetLikelihood([L.Bernoulli(), L.HetGaussian()])
    got = het.negative_log_predictive(Y, M, V, het.generate_metadata(), S, seed=seed)
    want, bound = 0.0, 0.0
    for t, (name, kw) in enumerate(specs):
        est = mr.estimate(name, Y[t], M[t], V[t], S, seed + t, **kw)
        want -= est.sum() / S
        bound += (mr.c_sum(name)[BULK] * EPS * mr.scale(name, Y[t], M[t], V[t], S, seed + t, **kw)).sum() / S
    same_seed = -sum(mr.estimate(name, Y[t], M[t], V[t], S, seed, **kw).sum() / S for t, (name, kw) in enumerate(specs))
    print("[mclp] facade: got %.17g, restated %.17g, |difference| %.3g, bound %.3g" % (got, want, abs(got - want), bound))
    assert abs(got - want) <= bound
    assert abs(got - same_seed) > 1e3 * bound            # (the second task does draw with seed + 1)
