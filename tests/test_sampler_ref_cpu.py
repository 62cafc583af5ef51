"""The sampler reference on its own, no GPU: the restated samplers of tests/sampler_ref.py pass every statistic of every
designed case with the very seeds, rows and thresholds that tests/test_samplers_gpu.py uses -- so the acceptance level is a condition
checked beforehand, not a measurement -- and each seeded corruption of the restatement is rejected by at least one statistic."""
import functools

import numpy as np
import pytest

import sampler_ref as sr

CASES = sr.cases()
BY_ID = {c["id"]: c for c in CASES}


def test_restated_samplers_pass_every_designed_case():
    sr.N_STATISTICS[0] = 0
    low = {}
    for c in CASES:
        p = sr.run_case(c, sr.restated_sample)
        k = min(p, key=p.get)
        print("%-22s %3d statistics, smallest p %.3g (%s)" % (c["id"], len(p), p[k], k))
        low.update({(c["id"], s): v for s, v in p.items() if not v >= sr.P_MIN})
    n = sr.N_STATISTICS[0]
    print("%d statistics in all: a correct sampler fails one of them with probability <= %.1e" % (n, n * sr.P_MIN))
    assert n <= sr.MAX_STATISTICS
    assert not low, low


def test_cases_are_reproducible_and_cover_the_switches():
    again = {c["id"]: c for c in sr.cases()}
    assert all(np.array_equal(c["F"], again[c["id"]]["F"]) and c["seed"] == again[c["id"]]["seed"] for c in CASES)
    assert len({c["seed"] for c in CASES}) == len(CASES) and all(c["F"].shape[0] == sr.N_ROWS for c in CASES)
    lam = np.unique(np.exp(BY_ID["poisson"]["F"][:, 0]))
    assert np.any((lam < 10.0) & (lam > 9.9)) and np.any((lam >= 10.0) & (lam < 10.1)) and np.any(lam > 1e15)     # both sides of the switch
    a = np.exp(BY_ID["gamma"]["F"][:, 0])
    assert a.min() < 0.025 and np.mean(a < 0.2) > 0.02 and a.max() > 1e9                                          # boost branch, upper clip
    b = np.exp(BY_ID["gamma"]["F"][:, 1])
    assert b.min() < 1e-9 and b.max() > 1e9
    nq = 1000 * np.minimum(sr.sigmoid_clipped(BY_ID["binomial_n1000"]["F"][:, 0]), 1 - sr.sigmoid_clipped(BY_ID["binomial_n1000"]["F"][:, 0]))
    assert np.any((nq < 10.0) & (nq > 9.9)) and np.any((nq >= 10.0) & (nq < 10.1))


def test_restatement_matches_the_law_where_it_is_closed_form():
    """The generator's own arithmetic at points that can be written down: the first uniforms of (seed 0, row 0) from splitmix64 worked by
    hand in Python integers, and a row's key depending on the row."""
    M = (1 << 64) - 1

    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & M
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)
    for seed, row in ((0, 0), (11, 7), (2 ** 63 + 5, 199999)):
        g = sr.RowRng(seed, row + 1)
        key = sm(seed ^ ((row * 0xD1342543DE82EF95) & M))
        assert int(g.key[row]) == key
        idx = np.array([row])
        for ctr in (1, 2, 3):
            h = sm(key ^ ((ctr * 0x9E3779B97F4A7C15) & M))
            assert g.uniform(idx)[0] == ((h >> 11) + 0.5) / 9007199254740992.0
        assert int(g.ctr[row]) == 3 and (row == 0 or int(g.ctr[0]) == 0)     # a row that draws advances alone


# (corruption, the designed case that must reject it, the point at which the earlier two-moment check is put to it)
CORRUPTIONS = [("boost_exponent", "gamma", ("Gamma", [-0.7, 0.3], {})),
               ("squeeze_always", "gamma_shape_1_4", ("Gamma", [0.4, 0.3], {})),
               ("ptrs_fast_accept", "poisson_ptrs", ("Poisson", [3.5], {})),
               ("inversion_from_one", "poisson", ("Poisson", [1.0], {})),
               ("no_reflection", "binomial_n1000", ("Binomial", [0.85], {"pred_trials": 1000})),
               ("normal_one_counter", "gaussian_sigma_0.7", ("Gaussian", [0.4], {"sigma": 0.7})),
               ("key_ignores_row", "gaussian_sigma_0.7", ("Gaussian", [0.4], {"sigma": 0.7})),
               ("student_gamma_nu", "student_nu_5", ("Student", [0.4, -0.3], {"deg_free": 5.0})),
               ("categorical_no_renorm", "categorical_den_overflow_K4", None)]


@pytest.mark.parametrize("corrupt,cid,probe", CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_seeded_corruption_is_rejected(corrupt, cid, probe):
    """Each defect, seeded into the restatement, must be rejected (p < 1e-6) by a statistic of a designed case; printed beside it is whether
    40 000 draws' mean and variance within 5 standard errors -- all the suite asked before -- would have let it through.

    categorical_no_renorm is put to the rows where 1 + sum_k exp(f_k) overflows (two f at 750): the clipped probabilities sum to K 1e-9 there
    and the renormalisation alone decides the draw.  Everywhere else the clips move the sum by at most (K - 1) 1e-9 -- about 1e-3 differing
    labels in 2e5 rows -- and no statistic on draws can tell (on categorical_K4 the corrupted sampler changes not one label, p 0.184)."""
    assert set(c[0] for c in CORRUPTIONS) == set(sr.CORRUPTIONS)
    p = sr.run_case(BY_ID[cid], functools.partial(sr.restated_sample, corrupt=corrupt))
    k = min(p, key=p.get)
    if corrupt == "key_ignores_row":
        assert p["lag_rows"] < sr.P_MIN
    mom = "n/a (labels)" if probe is None else ("pass" if sr.moments_within_5se(probe[0], probe[1], probe[2], corrupt) else "reject")
    print("%-22s on %-20s smallest p %.3g (%s); rejected by %s; two moments at 5 s.e.: %s" %
          (corrupt, cid, p[k], k, sorted(s for s in p if p[s] < sr.P_MIN), mom))
    assert p[k] < sr.P_MIN, (corrupt, p)


def test_beta_draw_with_both_variates_underflowing_is_a_vertex():
    """The regime the Beta sampler had 0 / 0 in (e^f below 7e-3 in both components): a share of rows does have both Gamma variates at 0, and
    the restated draw there is 0 or 1."""
    c = BY_ID["beta_tiny"]
    g = sr.RowRng(c["seed"], c["F"].shape[0])
    al = np.arange(c["F"].shape[0])
    x = g.gamma(al, sr.clip9(sr.safe_exp(c["F"][:, 0])))
    yv = g.gamma(al, sr.clip9(sr.safe_exp(c["F"][:, 1])))
    both = (x + yv == 0.0)
    share = [float(both[idx].mean()) for idx in c["groups"]]
    print("share of rows with both variates 0, per group of beta_tiny:", ["%.3g" % s for s in share])
    assert share[1] > 0.2 and share[4] > 0.99 and share[6] == 0.0
    y = sr.restated_sample("Beta", c["F"], c["seed"])[:, 0]
    assert np.all(np.isfinite(y)) and set(np.unique(y[both])) <= {0.0, 1.0}


def test_a_wrong_label_on_the_clip_rows_is_rejected():
    """The two Categorical rows the clips decide (one f at +30, all f at -30) leave one class with an expectation of 20 draws or more: the
    statistic there is the binomial count of that class, which passes the law's own draws and rejects a constant other label, a uniform
    label and twenty stray labels in 66 667."""
    for K in (2, 4, 6):
        c = BY_ID["categorical_K%d" % K]
        for gi in (1, 2):
            pmf = sr.law("Categorical", c["F"][c["groups"][gi][0]], K=K)[0]
            n, top = len(c["groups"][gi]), int(np.argmax(pmf)) + 1
            assert pmf[top - 1] > 1.0 - 1e-8
            other = top % K + 1
            right = np.full(n, float(top))
            stray = right.copy()
            stray[:20] = other
            assert sr.pmf_test(right, pmf) >= sr.P_MIN
            assert sr.pmf_test(np.full(n, float(other)), pmf) < sr.P_MIN
            assert sr.pmf_test(1.0 + np.arange(n) % K, pmf) < sr.P_MIN
            assert sr.pmf_test(stray, pmf) < sr.P_MIN
