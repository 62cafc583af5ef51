"""CPU: the references of the Monte-Carlo log predictive density against each other and against seeded defects -- the float64
restatement tests/mclp_ref.py against the 50-digit grid tests/golden/mclpgrid.npz (the raw figures behind C_ORACLE), the restated generator
against splitmix64 worked in Python integers and against the normal law, the corruptions the criterion and the statistics must reject, and
the kernels' own (max, sum-exp) update emulated in NumPy on the rows whose samples have log p = -inf."""
import json
import os

import numpy as np
import pytest

import mclp_ref as mr
import mclp_ref_mp as mmp

BULK, EDGE = mr.BULK, mr.EDGE
STAT_SEEDS = (0, 12345, 2 ** 63 + 5)
STAT_PAIRS = (0, 1, 2)


@pytest.fixture(scope="module")
def grid():
    return mr.load_grid()


def _block(grid, tag):
    return next(b for b in grid if b.tag == tag)


def _call(grid, tag, S):
    return next(c for c in _block(grid, tag).calls if c.S == S)


# ------------------------------------------------------------------------------------------------ the generator, value by value
def test_literal_of_u1_is_two_to_the_53():
    assert 9007199254740993.0 == 2.0 ** 53 and 9007199254740992.0 == 2.0 ** 53


def test_generator_first_values_against_python_integers():
    """u1, u2 of the restatement equal the hash worked in Python integers, and z0, z1 the 50-digit Box-Muller values to a few ulps."""
    import mpmath
    worst = 0.0
    for seed in mr.SEEDS:
        for n in (0, 1, 5, 2 ** 31 + 7):
            for s in (0, 1, 64, 999):
                for pair in (0, 1, 3):
                    z0, z1 = mr.normal_pair(seed, n, s, pair)
                    u1, u2 = mmp.uniforms(seed, n, s, pair)
                    assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
                    with mpmath.mp.workdps(50):
                        w0, w1 = mmp.normal_pair(seed, n, s, pair)
                        r = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(u1)))
                        for got, want in ((float(z0), w0), (float(z1), w1)):
                            worst = max(worst, float(abs(got - want) / (mr.EPS * max(r, mpmath.mpf(1e-300)))))
    print("[mclp] normal_pair float64 against 50 digits: worst |z - Z| / (2^-52 r) = %.3g" % worst)
    assert worst <= 4.0            # log, sqrt, cos / sin and the product: four roundings of at most an ulp of r each (measured: 0.851)
    h = mmp.splitmix64(0)
    assert h == 0xE220A8397B1DCDAF  # splitmix64's published first output for the state 0


def test_u1_equal_to_one_gives_zero():
    """u1 = 1 (h >> 11 = 2^53 - 1) is inside the generator's range: r = 0 and both draws are 0."""
    u1 = (float(2 ** 53 - 1) + 1.0) * (1.0 / 9007199254740993.0)
    assert u1 == 1.0 and np.sqrt(-2.0 * np.log(u1)) == 0.0


# ------------------------------------------------------------------------------------------------ the grid and the float64 restatement
def test_grid_covers_what_the_issue_names(grid):
    fam = {}
    evaluations = 0
    for b in grid:
        fam.setdefault(b.name, []).append(b.kw)
        assert tuple(c.S for c in b.calls) == mr.SAMPLE_COUNTS
        assert {c.seed for c in b.calls} == set(mr.SEEDS)
        for c in b.calls:
            assert c.n % 4 != 0, (b.tag, c.S)
            evaluations += c.n * c.S
            assert (c.cls[c.cls == EDGE].size > 0) == (c.S == 65 or (b.tag == "exponential" and c.S in (1, 64, 1000)))
    assert set(fam) == set(mr.FAMILIES)
    assert sorted(k["deg_free"] for k in fam["Student"]) == [0.5, 5.0, 300.0]
    assert sorted(k["K"] for k in fam["Ordinal"]) == [2, 5, 11]
    assert sorted(k["K"] for k in fam["Categorical"]) == [2, 3, 6, 9]
    assert sorted(k["K"] for k in fam["Dirichlet"]) == [2, 3, 4]
    w = _block(grid, "weibull")
    assert set(np.unique(w.y[:, 1])) == {0.0, 1.0}
    assert evaluations <= 300000
    assert os.path.getsize(mr.GRID) <= 1 << 20
    e = _block(grid, "exponential")
    inf_rows = [(c.S, float(c.m[i, 0])) for c in e.calls for i in np.flatnonzero(np.isneginf(c.R))]
    assert sorted(inf_rows) == [(1, 30.0), (65, 30.0)]
    mixed = [c.S for c in e.calls for i in np.flatnonzero((c.y[:, 0] == 1e300) & (c.v[:, 0] == 4.0))]
    assert sorted(mixed) == [64, 1000]
    print("[mclp] grid: %d blocks, %d rows, %d sample evaluations" % (len(grid), sum(len(b.cls) for b in grid), evaluations))


def test_float64_restatement_against_grid(grid):
    """The raw figures behind mclp_ref.C_ORACLE: per family and class the largest |float64 - R| / (2^-52 Sc); each constant is that figure
    rounded up to a power of two."""
    worst = {}
    for b in grid:
        cur = worst.setdefault(b.name, {BULK: 0.0, EDGE: 0.0})
        for c in b.calls:
            r = mr.ratios(mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, **b.kw), c)
            assert np.isfinite(r).all(), (b.tag, c.S)
            for cls in (BULK, EDGE):
                if (c.cls == cls).any():
                    cur[cls] = max(cur[cls], float(r[c.cls == cls].max()))
    for name, w in worst.items():
        C = mr.c_oracle(name)
        print("[mclp] %-13s float64 against the grid: bulk %.3g (C_ORACLE %g)  edge %.3g (C_ORACLE %g)  -> C_KERNEL %g / %g" % (
            name, w[BULK], C[BULK], w[EDGE], C[EDGE], mr.c_kernel(name)[BULK], mr.c_kernel(name)[EDGE]))
        for cls in (BULK, EDGE):
            assert w[cls] <= C[cls], (name, cls, w[cls])
            assert C[cls] == 2.0 ** np.ceil(np.log2(max(w[cls], 1.0))), (name, cls, w[cls], C[cls])


def test_grid_row_regenerates_from_the_50_digit_reference(grid):
    for tag in ("hetgaussian", "ordinal5", "binomial", "dirichlet3"):
        b = _block(grid, tag)
        c = b.calls[1]                  # S = 2
        i = c.n - 1
        y = float(c.y[i, 0]) if c.y.shape[1] == 1 else tuple(float(t) for t in c.y[i])
        R, Sc, n_out, near = mmp.row(b.name, y, c.m[i], c.v[i], c.S, c.seed, i, **b.kw)
        assert R == c.R[i] and Sc == c.Sc[i] and n_out == 0


def test_refused_families_stay_refused():
    for name in mr.MC_REFUSED:
        with pytest.raises(ValueError):
            mr.estimate(name, np.ones(3), np.zeros((3, 2)), np.ones((3, 2)), 4, 0)


# ------------------------------------------------------------------------------------------------ the generator's law
def test_generator_law():
    """Every statistic of the restated generator reaches p >= 1e-6 at 2e5 draws; at most 1000 statistics, so that with fixed seeds a correct
    generator fails anywhere with probability <= 1e-3."""
    lo, where = 1.0, None
    for seed in STAT_SEEDS:
        for pair in STAT_PAIRS:
            for k, p in mr.generator_statistics(seed, pair).items():
                if p < lo:
                    lo, where = p, (seed, pair, k)
                assert p >= mr.P_MIN, (seed, pair, k, p)
    print("[mclp] generator law: %d statistics, smallest p = %.3g at %r" % (mr.N_STATISTICS[0], lo, where))
    assert 0 < mr.N_STATISTICS[0] <= mr.MAX_STATISTICS


GENERATOR_REJECTED_BY = {"pair_ignored": "pair p ~ p+1", "s_unshifted": "(s, p+1) ~ (s+1, p)", "u2_from_h": "rows z0 chi2", "z1_is_z0": "z0 ~ z1",
                         "row_ignored": "row n ~ n+1", "no_two_pi": "rows z0 chi2"}


@pytest.mark.parametrize("corrupt", mr.GENERATOR_CORRUPTIONS)
def test_generator_corruptions_are_rejected(corrupt):
    p = mr.generator_statistics(STAT_SEEDS[1], 0, corrupt=corrupt)
    k = GENERATOR_REJECTED_BY[corrupt]
    failed = sorted(t for t, v in p.items() if v < mr.P_MIN)
    print("[mclp] generator corruption %-14s p(%s) = %.3g; %d statistics below 1e-6: %s" % (corrupt, k, p[k], len(failed), ", ".join(failed)))
    assert p[k] < mr.P_MIN, (corrupt, k, p[k])


# ------------------------------------------------------------------------------------------------ the combination
# corruption -> (block, S of the call, row of the call): the named grid row that must miss its C_KERNEL
COMBINE_ROW = {"no_log_S": ("bernoulli", 65, 1), "S_round_64": ("poisson", 65, 0), "idle_lanes": ("dirichlet3", 65, 0),
               "drop_partial_stride": ("categorical9", 65, 0), "no_rescale": ("student_nu5", 1000, 0), "stride_N_minus_1": ("weibull", 1000, 0)}


@pytest.mark.parametrize("corrupt", mr.COMBINE_CORRUPTIONS)
def test_combination_corruptions_are_rejected(grid, corrupt):
    tag, S, row = COMBINE_ROW[corrupt]
    c = _call(grid, tag, S)
    b = c.block
    clean = mr.ratios(mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, **b.kw), c)[row]
    r = mr.ratios(mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, corrupt=corrupt, **b.kw), c)[row]
    C = mr.c_kernel(b.name)[int(c.cls[row])]
    print("[mclp] corruption %-20s %s S = %d row %d: ratio %.3g (clean %.3g, C_KERNEL %g)" % (corrupt, tag, S, row, r, clean, C))
    assert clean <= mr.c_oracle(b.name)[int(c.cls[row])]
    assert r > C, (corrupt, r)


# ------------------------------------------------------------------------------------------------ the kernels' own update
def test_lane_update_on_the_issue_examples():
    """The per-lane update before the fix, as NumPy evaluates it: (mx, se) after the samples of ONE lane."""
    def lane(ls, fixed):
        mx, se = -np.inf, 0.0
        with np.errstate(all="ignore"):
            for x in ls:
                if fixed and x == -np.inf:
                    continue
                if x > mx:
                    se, mx = se * np.exp(mx - x) + 1.0, x
                else:
                    se += np.exp(x - mx)
        return mx, se
    mx, se = lane([-np.inf, -1.0, -2.0], False)
    assert mx == -1.0 and np.isnan(se)
    mx, se = lane([-1.0, -np.inf, -2.0], False)
    assert mx == -1.0 and abs(se - (1.0 + np.exp(-1.0))) < 1e-15
    mx, se = lane([-np.inf], False)
    assert mx == -np.inf and np.isnan(se)
    assert lane([-np.inf, -1.0, -2.0], True) == lane([-1.0, -2.0], True)
    assert lane([-np.inf], True) == (-np.inf, 0.0)
    assert np.isnan(lane([np.nan], True)[1]) and np.isnan(lane([-1.0, np.nan], True)[1])      # a NaN log p still reaches the sum


def test_emulated_kernel_update_on_the_minus_inf_rows(grid):
    """The two branches plus the butterfly, in the kernels' order, on the Exponential rows with y = 1e300.  Before the fix: NaN where a lane
    holds a -inf sample in front of a finite one (S = 1000); where every lane holds one sample (S = 64) or only -inf samples (S = 1, 65)
    the butterfly's own -inf guard still hides the lane's NaN.  With the fix: R on every one of them."""
    e = _block(grid, "exponential")
    seen = []
    for c in e.calls:
        for i in np.flatnonzero(c.y[:, 0] == 1e300):
            l = mr.estimate(e.name, c.y_arg(), c.m, c.v, c.S, c.seed, return_parts=True)[1][i]
            n_inf = int(np.isneginf(l).sum())
            old, new = mr.kernel_combine(l, c.S, fixed=False), mr.kernel_combine(l, c.S, fixed=True)
            first_inf = any(np.isneginf(l[k]) and np.isfinite(l[k + 64:c.S:64]).any() for k in range(min(64, c.S)))
            print("[mclp] Exponential y = 1e300, (m, v) = (%g, %g), S = %d: %d samples -inf; update before the fix %r, with it %r, R %r" % (
                c.m[i, 0], c.v[i, 0], c.S, n_inf, old, new, float(c.R[i])))
            seen.append((c.S, first_inf))
            if np.isneginf(c.R[i]):
                assert n_inf == c.S and new == -np.inf
            else:
                assert 0 < n_inf < c.S
                assert abs(new - c.R[i]) <= mr.c_kernel(e.name)[EDGE] * mr.EPS * c.Sc[i]
                assert np.isnan(old) == first_inf
    assert (1000, True) in seen and len(seen) == 4


def test_emulated_kernel_update_is_the_estimate_on_a_bulk_call(grid):
    """On rows without -inf samples the emulated kernel order (with and without the fix) stays within C_KERNEL of R."""
    for tag in ("poisson", "dirichlet3"):
        c = _call(grid, tag, 100)
        b = c.block
        l = mr.estimate(b.name, c.y_arg(), c.m, c.v, c.S, c.seed, return_parts=True, **b.kw)[1]
        for fixed in (False, True):
            got = np.array([mr.kernel_combine(r, c.S, fixed=fixed) for r in l])
            assert (mr.ratios(got, c) <= mr.c_kernel(b.name)[BULK]).all()
        nan_row = l[0].copy()
        nan_row[70] = np.nan
        assert np.isnan(mr.kernel_combine(nan_row, c.S, fixed=True))
        assert np.isnan(mr.kernel_combine(np.full(1, np.nan), 1, fixed=True))
        assert mr.kernel_combine(np.full(1, np.nan), 1, fixed=False) == -np.inf     # the old butterfly guard replaced the NaN lane by 0


def test_spec_is_json_and_seeds_survive(grid):
    g = np.load(mr.GRID)
    spec = json.loads(str(g["spec"]))
    assert max(seed for _, _, _, calls in spec for _, seed in calls) == 2 ** 63 + 5
