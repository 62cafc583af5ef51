"""CPU: the heteroscedastic Student-t likelihood at the layers that need no device -- the C enum, the ctypes ids, the
descriptor and its metadata, and the NumPy restatement the GPU tests compare against."""
import os
import re

import numpy as np
import pytest

from oracle import lik_student

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hetmogp_hip.h")


def test_header_declares_student_id():
    src = open(HEADER).read()
    assert re.search(r"\bHMOGP_LIK_STUDENT\s*=\s*8\b", src)
    assert int(re.search(r"#define HMOGP_ABI_VERSION (\d+)", src).group(1)) == 8   # additive: no ABI bump


def test_python_ids_and_dims():
    from hetmogp_amd import _lib, engine
    assert _lib.LIK_STUDENT == 8 and _lib.LIK_IDS_BY_NAME["Student"] == 8
    assert engine.LIK_IDS["Student"] == 8
    assert engine.lik_dim_f("Student", deg_free=3.0) == 2
    assert engine.lik_param("Student", deg_free=3.0) == 3.0
    assert engine.lik_param("Student") == 5.0


def test_descriptor_metadata_and_positional_call():
    from hetmogp_amd import Student
    s = Student()
    assert s.get_metadata() == (1, 2, 1)
    assert s.deg_free == 5.0 and s.kwargs() == {"deg_free": 5.0}
    assert Student(None, 3.0).deg_free == 3.0          # the reference's positional order: gp_link first
    assert Student(deg_free=30).kwargs() == {"deg_free": 30.0}


def test_het_likelihood_metadata_with_student():
    from hetmogp_amd import HetLikelihood, Gaussian, Student
    md = HetLikelihood([Gaussian(), Student()]).generate_metadata()
    assert md["function_index"].tolist() == [0, 1, 1]
    assert md["d_index"].tolist() == [0, 0, 1]
    assert md["y_index"].tolist() == [0, 1] and md["pred_index"].tolist() == [0, 1]
    assert HetLikelihood([Student(), Student(None, 2.0)]).specs() == [("Student", {"deg_free": 5.0}),
                                                                      ("Student", {"deg_free": 2.0})]


@pytest.mark.parametrize("nu", [1.0, 2.5, 5.0, 30.0])
def test_reference_derivatives_match_central_differences(nu):
    rng = np.random.RandomState(int(nu * 10))
    n = 200
    y = rng.randn(n) * 3.0
    f0 = rng.randn(n) * 2.0
    f1 = rng.randn(n) * 1.5
    y[:20] += 40.0                                     # outlier regime
    h = 1e-5
    lp, d0, d1, d00, d11 = lik_student.logpdf_and_derivatives(y, f0, f1, nu)
    P = lambda a, b: lik_student.logpdf_and_derivatives(y, a, b, nu)
    fd0 = (P(f0 + h, f1)[0] - P(f0 - h, f1)[0]) / (2 * h)
    fd1 = (P(f0, f1 + h)[0] - P(f0, f1 - h)[0]) / (2 * h)
    fd00 = (P(f0 + h, f1)[1] - P(f0 - h, f1)[1]) / (2 * h)
    fd11 = (P(f0, f1 + h)[2] - P(f0, f1 - h)[2]) / (2 * h)
    for an, fd in ((d0, fd0), (d1, fd1), (d00, fd00), (d11, fd11)):
        assert np.max(np.abs(an - fd) / (1.0 + np.abs(an))) < 1e-7


def test_reference_logpdf_is_a_density_and_tends_to_het_gaussian():
    # integrates to one over y (trapezoid on a wide grid), and at nu -> inf equals the HetGaussian log density
    yy = np.linspace(-400.0, 400.0, 400001)
    lp = lik_student.logpdf_and_derivatives(yy, 0.3, np.log(0.7), 3.0)[0]
    assert abs(np.trapezoid(np.exp(lp), yy) - 1.0) < 1e-4
    y, f0, f1 = np.array([0.1, -2.0, 3.0]), np.array([0.0, 0.5, 1.0]), np.array([-0.3, 0.2, 0.0])
    het = -0.5 * np.log(2 * np.pi) - 0.5 * f1 - 0.5 * (y - f0) ** 2 * np.exp(-f1)
    assert np.max(np.abs(lik_student.logpdf_and_derivatives(y, f0, f1, 1e8)[0] - het)) < 1e-6
