"""GPU: `hmogp_sample` against the laws it draws from.  The designed cases of tests/sampler_ref.py -- the same seeds, rows and
thresholds that tests/test_sampler_ref_cpu.py has already put the restated samplers through -- run through `engine.sample`: every
statistic must reach p >= 1e-6.  The branch-free samplers are also pinned draw by draw against the restatement (splitmix64, the row key,
the counter order and Box-Muller themselves); for the rejection samplers the share of differing rows is printed, not asserted: it is the
share of rows where an ulp of the device libm flips an acceptance.

Measured figures (smallest p per case, differing-row shares, run times): DESIGN 9p."""
import time

import numpy as np
import pytest

import sampler_ref as sr

pytestmark = pytest.mark.gpu

CASES = sr.cases()
BY_ID = {c["id"]: c for c in CASES}


def _draw(name, F, seed, **kw):
    from hetmogp_amd import engine
    return engine.sample(name, F, seed=seed, **kw)


@pytest.mark.parametrize("cid", [c["id"] for c in CASES])
def test_device_draws_follow_their_law(cid):
    t0 = time.time()
    p = sr.run_case(BY_ID[cid], _draw)
    k = min(p, key=p.get)
    print("%-22s %3d statistics, smallest p %.3g (%s), %.2f s" % (cid, len(p), p[k], k, time.time() - t0))
    assert not {s: v for s, v in p.items() if not v >= sr.P_MIN}, (cid, p)


def test_beta_draws_are_finite_down_to_the_clips():
    """f down to -25 in both components (a = b = 1e-9 after the clip): both Gamma variates underflow in almost every row.  Every draw is
    finite and in [0, 1]; in every row where the restatement has both variates at exactly 0 the device draw is a vertex, and the very
    vertex the restatement takes (one more uniform and one comparison, no libm in between)."""
    c = BY_ID["beta_tiny"]
    F, seed = c["F"], c["seed"]
    y = _draw("Beta", F, seed)[:, 0]
    assert not np.any(np.isnan(y)) and np.all((y >= 0.0) & (y <= 1.0))
    ref = sr.restated_sample("Beta", F, seed)[:, 0]
    g = sr.RowRng(seed, F.shape[0])
    al = np.arange(F.shape[0])
    x = g.gamma(al, sr.clip9(sr.safe_exp(F[:, 0])))
    both = (x + g.gamma(al, sr.clip9(sr.safe_exp(F[:, 1]))) == 0.0)
    idx = c["groups"][4]                                       # f = (-25, -25)
    assert both[idx].mean() > 0.99 and set(np.unique(y[both])) <= {0.0, 1.0}
    print("Beta: rows with both variates 0 in the restatement %d of %d, of which the device differs in %d; share of ones at f = (-25, -25) "
          "%.4f (a / (a + b) = 0.5)" % (both.sum(), both.size, int(np.sum(y[both] != ref[both])), y[idx].mean()))
    assert np.array_equal(y[both], ref[both])


@pytest.mark.parametrize("cid", sr.PIN_CASES + ("ordinal",))
def test_branch_free_draws_equal_the_restated_generator(cid):
    c = sr.ordinal_pin_case() if cid == "ordinal" else BY_ID[cid]
    got = _draw(c["name"], c["F"], c["seed"], **c["kw"])[:, 0]
    ref = sr.restated_sample(c["name"], c["F"], c["seed"], **c["kw"])[:, 0]
    if c["name"] in sr.PIN_LABELS:
        assert np.array_equal(got, ref), (cid, int(np.sum(got != ref)), "labels differ")
        return
    same = got == ref                                            # (covers a pair of equal infinities)
    with np.errstate(invalid="ignore"):
        ex = np.where(same, 0.0, np.abs(got - ref) / sr.pin_scale(c, ref))
    print("%-20s worst |device - restated| / scale %.3g; rows equal to the bit %.4f" % (cid, np.nanmax(ex), same.mean()))
    assert np.all(ex <= 1e-12), (cid, float(np.nanmax(ex)), int(np.nanargmax(ex)))


def test_rejection_samplers_differ_from_the_restatement_only_in_a_few_rows():
    """Printed, not asserted: where the device libm and NumPy's differ by an ulp, an acceptance flips and the row's later draws shift."""
    for cid in sr.REJECTION_CASES:
        c = BY_ID[cid]
        got = _draw(c["name"], c["F"], c["seed"], **c["kw"])
        ref = sr.restated_sample(c["name"], c["F"], c["seed"], **c["kw"])
        with np.errstate(invalid="ignore", divide="ignore"):
            diff = np.any(np.abs(got - ref) > 1e-9 * np.maximum(np.abs(ref), 1e-300), axis=1)
        print("%-18s share of rows that differ from the restatement (beyond 1e-9 relative): %.3e" % (cid, diff.mean()))


@pytest.mark.parametrize("cid", ["gamma", "beta_tiny", "binomial_n1000", "dirichlet_K3", "categorical_K5"])
def test_draws_are_reproducible_per_seed(cid):
    c = BY_ID[cid]
    F = c["F"][:4099]
    a, b, d = (_draw(c["name"], F, s, **c["kw"]) for s in (c["seed"], c["seed"], c["seed"] + 1))
    assert np.array_equal(a, b) and not np.array_equal(a, d)
    head = _draw(c["name"], F[:257], c["seed"], **c["kw"])       # a row's draw depends on (seed, row) alone, not on the batch
    assert np.array_equal(head, a[:257])
