"""GPU: one model that holds all three contract families -- Student, Ordinal and Dirichlet -- against the oracle,
with the checks and yardsticks of tests/model_cases.py.  The smallest shapes at which pool offsets, the per-task `ldy` stride (only
the Dirichlet task's Y is [N, 3]) and the per-family launches can go wrong together; it runs no code the family files do not."""
import pytest

import model_cases as mc

pytestmark = pytest.mark.gpu

SPECS = [("Student", {"deg_free": 3.0}), ("Ordinal", {"K": 5, "bin_edges": [-2.0, -0.9, 0.1, 1.7], "sigma": 0.8}),      # ORD5 of test_ordinal_gpu.py
         ("Dirichlet", {"K": 3})]
NS = [300, 257, 129]


def test_small_model_path_and_no_small_path():
    """M = 16: a family set outside the baseline masks, so the segment table takes the singleton quad_multi launches."""
    mc.check_small_vs_regular(mc.family_case(3100, SPECS, NS, 16, 2, 1), NS, ([60, 50, 20], [160, 137, 129]))


def test_elbo_grad_vs_oracle():
    mc.check_vs_oracle(mc.family_case(3200, SPECS, NS, 128, 2, 1), NS)
