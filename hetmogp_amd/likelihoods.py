"""Likelihood descriptors with the reference's class names and constructor arguments (likelihoods/*.py) and the
heterogeneous wrapper (hetmogp/het_likelihood.py).  They describe the model to the engine; the variational
expectations themselves are HIP kernels (csrc/lik_device.h).  `var_exp` / `var_exp_derivatives` are offered with the
reference's signatures and run on the device."""
import numpy as np

from .param import Param

# Rows of the deterministic log predictive density whose effective number of nodes `ess` is below their family's value here are
# reported by one RuntimeWarning per call: the fixed, prior-centred Gauss-Hermite rule does not resolve a likelihood that much narrower
# than q(f).  MEASURED, not chosen (tests/test_logpred_cpu.py::test_accuracy_envelope re-measures and prints them; table in DESIGN 9j): per
# family the largest ess, rounded up to one decimal, among the seeded bulk rows (m in [-3, 3], v in [1e-3, 4]) whose rule differs from the
# integral itself by more than 1e-2.  One constant for all families does not work: a tensor rule's ess is the product of its dimensions'
# (a 400-node rule that resolves one dimension and not the other still has ess ~ 10), so the 28.3 of Dirichlet would flag every good
# one-dimensional row.  Families in which no seeded row misses 1e-2 take the largest value among the families with as many nodes
# (marked *); Categorical, alone in its class, takes none, and the closed-form Gaussian has ess = +inf.
LPD_ESS_WARN = {
    "Gaussian": 0.0, "Bernoulli": 2.4, "Poisson": 2.0, "Exponential": 2.3, "Ordinal": 2.4, "HetGaussian": 2.4,      # Bernoulli *, Ordinal *
    "Gamma": 11.2, "Beta": 9.0, "Student": 13.8, "Weibull": 14.2, "NegBinomial": 14.2,                              # NegBinomial *
    "Dirichlet": 28.3, "Categorical": 0.0,
    # (rows (k, n) with n log-uniform in 1 .. 2000: tests/test_binom_cpu.py::test_lpd_ess_warn_is_measured re-measures these two.  A row of
    #  many trials is a narrow likelihood: 23 of the 232 Binomial rows whose dense integral settles miss 1e-2, ten of them at v <= 0.25)
    "Binomial": 2.1, "BetaBinomial": 6.0,
    # (tests/test_zip_cpu.py::test_lpd_ess_warn_is_measured re-measures it: 7 of the 505 seeded rows whose dense integral settles miss 1e-2,
    #  every one of them a row with y >= 1 -- a Poisson count's narrow likelihood in f0 -- and none of the 475 rows within 1e-4 is flagged)
    "ZIPoisson": 10.7,
}


def lpd_ess_warn(name, **kw):
    """The family's LPD_ESS_WARN.  Dirichlet's is measured at K = 3 (10^3 nodes); another K takes the same value per dimension,
    28.3^(K/3) -- an extrapolation, not a measurement."""
    c = LPD_ESS_WARN[name]
    return c ** (int(kw["K"]) / 3.0) if name == "Dirichlet" and "K" in kw else c


def warn_low_ess(ess_per_task, specs, what="log_predictive_density"):
    """One RuntimeWarning naming every task with rows below its family's LPD_ESS_WARN and their number (nothing when there is none).
    specs: [(family name, kwargs)] per task."""
    import warnings
    low = [(t, int(np.sum(np.asarray(e) < lpd_ess_warn(n, **k))), lpd_ess_warn(n, **k)) for t, (e, (n, k)) in enumerate(zip(ess_per_task, specs))]
    low = ["%d rows of task %d (effective nodes < %.1f)" % (n, t, c) for t, n, c in low if n > 0]
    if low:
        warnings.warn("%s: the fixed Gauss-Hermite rule does not resolve %s: the likelihood is much narrower than q(f) there and the "
                      "values are unreliable" % (what, ", ".join(low)), RuntimeWarning, stacklevel=3)


class _Lik(object):
    name = None
    _dims = (1, 1, 1)

    def kwargs(self):
        return {}

    # ---- the likelihood's own parameters: nothing to learn unless a constructor flag asks for it
    def learnable_params(self):
        """[(name, Param)] of the parameters this likelihood learns; SVMOGP lists them as `likelihood.<t>.<name>`."""
        return []

    def engine_values(self):
        """Current values in the layout of `hmogp_set_lik_params` (None: the engine's constants stay what they are)."""
        return None

    def set_engine_gradient(self, g):
        """Writes the Params' `.gradient` from the engine's raw gradient (layout of `engine_values`)."""

    def get_metadata(self):
        """(dim_y, dim_f, dim_p) as the reference's get_metadata()."""
        return self._dims

    def ismulti(self):
        return False

    def var_exp(self, Y, m, v, gh_points=None, Y_metadata=None):
        from .engine import var_exp
        ve, _, _ = var_exp(self.name, Y, m, v, **self.kwargs())
        return ve[:, None]

    def var_exp_derivatives(self, Y, m, v, gh_points=None, Y_metadata=None):
        from .engine import var_exp
        _, dm, dv = var_exp(self.name, Y, m, v, **self.kwargs())
        return dm, dv

    def log_predictive(self, Ytest, mu_F_star, v_F_star, num_samples, seed=0):
        """The reference's Monte-Carlo log predictive, including its 1/num_samples factor on the sum over test points
        (e.g. bernoulli.py:130-144).  Sampling happens on the device."""
        from .engine import log_predictive_rows
        lp = log_predictive_rows(self.name, Ytest, mu_F_star, v_F_star, num_samples, seed, **self.kwargs())
        return (1.0 / num_samples) * lp.sum()

    def log_predictive_density(self, Ytest, m, v, gh_T=0, return_ess=False):
        """Deterministic per-row log predictive density (N,) of DESIGN 9j: no sampling, no seed, no 1/num_samples factor; defined
        for every family.  return_ess=True: (lpd, ess)."""
        from .engine import log_predictive_density_rows
        lpd, ess = log_predictive_density_rows(self.name, Ytest, m, v, gh_T=gh_T, return_ess=True, **self.kwargs())
        warn_low_ess([ess], [(self.name, self.kwargs())])
        return (lpd, ess) if return_ess else lpd

    def predictive_cdf(self, Ytest, m, v, gh_T=0, return_sf=False):
        """Per-row predictive cdf P(Y <= y) (N,) of DESIGN 9k; return_sf=True: (cdf, sf).  Ytest: (N,) values (Ordinal labels, Weibull
        times).  NotImplementedError for a family whose cdf needs a special function that is not built."""
        from .engine import predictive_cdf_rows, predq_require
        predq_require(self.name)
        return predictive_cdf_rows(self.name, Ytest, m, v, gh_T=gh_T, return_sf=return_sf, **self.kwargs())

    def predictive_quantiles(self, m, v, probs, gh_T=0):
        """(N, len(probs)) predictive quantiles of DESIGN 9k; probs are probabilities in (0, 1)."""
        from .engine import predictive_quantile_rows, predq_require
        predq_require(self.name)
        return predictive_quantile_rows(self.name, m, v, probs, gh_T=gh_T, **self.kwargs())

    def predictive(self, m, v, gh_points=None, Y_metadata=None):
        """Predictive mean / variance of y (the reference's `predictive`; Gauss-Hermite order of a fresh instance)."""
        from .engine import predictive
        return predictive(self.name, m, v, **self.kwargs())

    def samples(self, F, num_samples=1, Y_metadata=None, seed=None):
        """One draw y ~ p(y | F[n]) per row, (N, 1); (N, K) for Dirichlet -- the reference's `samples` (e.g. gaussian.py:36-39, gamma.py:43-50,
        categorical.py:65-75: same link functions and clips, labels 1..K), generated on the device (`hmogp_sample`).
        The reference draws from NumPy's global generator; here the device generator is keyed by `seed`, which is itself
        drawn from NumPy's global generator when not given -- so `np.random.seed(k)` still makes a run reproducible, but
        the stream differs from the reference's (only the distribution is the same)."""
        from .engine import sample
        if seed is None:       # NB: one extra draw from NumPy's GLOBAL generator per call (shifts it relative to the reference)
            seed = int(np.random.randint(0, 2 ** 31 - 1))
        F = np.asarray(F, dtype=float)
        y = sample(self.name, F, seed=seed, **self.kwargs())
        if self.get_metadata()[1] == 1 and F.ndim == 2 and F.shape[1] > 1:
            return y.reshape(F.shape)      # one-function likelihoods: every entry of F is a draw, shape kept (gaussian.py:36-39)
        return y


class Gaussian(_Lik):
    name = "Gaussian"

    def __init__(self, sigma=None, gp_link=None, learn_sigma=False):
        self._sigma = 0.5 if sigma is None else sigma      # gaussian.py:21-24
        self._p_sigma = Param("sigma", [float(self._sigma)], positive=True) if learn_sigma else None

    @property
    def sigma(self):
        """The current value: a plain float also while it is being learned."""
        return self._sigma if self._p_sigma is None else float(self._p_sigma.values[0])

    @sigma.setter
    def sigma(self, value):
        if self._p_sigma is None:
            self._sigma = value
        else:
            self._p_sigma[...] = float(value)

    def kwargs(self):
        return {"sigma": self.sigma}

    def learnable_params(self):
        return [] if self._p_sigma is None else [("sigma", self._p_sigma)]

    def engine_values(self):
        return None if self._p_sigma is None else np.array([self.sigma])

    def set_engine_gradient(self, g):
        if self._p_sigma is not None:
            self._p_sigma.gradient = [g[0]]


class Bernoulli(_Lik):
    name = "Bernoulli"

    def __init__(self, gp_link=None):
        pass


class HetGaussian(_Lik):
    name = "HetGaussian"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Poisson(_Lik):
    name = "Poisson"

    def __init__(self, gp_link=None):
        pass


class Exponential(_Lik):
    name = "Exponential"

    def __init__(self, gp_link=None):
        pass


class Gamma(_Lik):
    name = "Gamma"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Beta(_Lik):
    name = "Beta"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Student(_Lik):
    """Heteroscedastic Student-t (the reference's likelihoods/student.py is a constructor only; the model is DESIGN 9):
    f0 = location (identity link), f1 = log of the squared scale (HetGaussian's convention), deg_free = nu -- fixed, or learned
    with `learn_deg_free=True`.  `gp_link` comes first so that the reference's positional call Student(gp_link) still works."""
    name = "Student"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None, deg_free=5.0, learn_deg_free=False):
        self._deg_free = float(deg_free)                   # 5: GPy's StudentT default
        self._p_nu = Param("deg_free", [self._deg_free], positive=True) if learn_deg_free else None

    @property
    def deg_free(self):
        return self._deg_free if self._p_nu is None else float(self._p_nu.values[0])

    @deg_free.setter
    def deg_free(self, value):
        if self._p_nu is None:
            self._deg_free = float(value)
        else:
            self._p_nu[...] = float(value)

    def kwargs(self):
        return {"deg_free": self.deg_free}

    def learnable_params(self):
        return [] if self._p_nu is None else [("deg_free", self._p_nu)]

    def engine_values(self):
        return None if self._p_nu is None else np.array([self.deg_free])

    def set_engine_gradient(self, g):
        if self._p_nu is not None:
            self._p_nu.gradient = [g[0]]


class Ordinal(_Lik):
    """Ordered probit (the reference's likelihoods/ordinal.py is a constructor only; the model is DESIGN 9b): one latent function,
    labels 1..K, p(y = k | f) = Phi((b_k - f) / sigma) - Phi((b_{k-1} - f) / sigma) with cut points b_1 < ... < b_{K-1}
    (`bin_edges`; K alone: b_k = k - K/2) and noise scale sigma -- fixed, or learned with `learn_edges` / `learn_sigma`:
    the cuts are then the free `edge0` = b_1 and the positive `gaps` delta_k = b_{k+1} - b_k, which no optimiser can make cross.
    `gp_link` comes first so that the reference's positional call Ordinal(gp_link) still works.  `predictive` returns the mean and
    variance of the label, (N, 1) each.
    The stand-alone helpers (`predictive`, `samples`, `log_predictive`, `var_exp`) carry the cuts through `hmogp_ordinal_table`, whose
    process-wide registry keeps every DISTINCT table (at most 4096, then InvalidArgument): calling one of them after every update of
    learned cuts, e.g. to log a score per training iteration, uses one entry per call.  The model's own evaluations do not (the
    engine keeps a private table); log every so many iterations, or at the end."""
    name = "Ordinal"

    def __init__(self, gp_link=None, K=None, bin_edges=None, sigma=1.0, learn_edges=False, learn_sigma=False):
        from .engine import ordinal_edges
        self._edges = ordinal_edges(K, bin_edges)
        self.K = len(self._edges) + 1
        self._sigma = float(sigma)
        self._p_edge0 = self._p_gaps = self._p_sigma = None
        if learn_edges:
            self._p_edge0 = Param("edge0", self._edges[:1])
            if self.K > 2:
                self._p_gaps = Param("gaps", np.diff(self._edges), positive=True)
        if learn_sigma:
            self._p_sigma = Param("sigma", [self._sigma], positive=True)

    @property
    def bin_edges(self):
        """The current cut points, a plain array."""
        if self._p_edge0 is None:
            return self._edges
        gaps = self._p_gaps.values if self._p_gaps is not None else np.zeros(0)
        return float(self._p_edge0.values[0]) + np.concatenate([[0.0], np.cumsum(gaps)])

    @bin_edges.setter
    def bin_edges(self, value):
        """Assignable as before; the number of cuts (K) is fixed at construction and the values are checked by the library."""
        e = np.array(value, dtype=np.float64).reshape(-1)
        if len(e) != self.K - 1:
            raise ValueError("Ordinal: %d cut points assigned to a likelihood with K = %d" % (len(e), self.K))
        if self._p_edge0 is None:
            self._edges = e
        else:
            self._p_edge0[...] = e[:1]
            if self._p_gaps is not None:
                self._p_gaps[...] = np.diff(e)

    @property
    def sigma(self):
        return self._sigma if self._p_sigma is None else float(self._p_sigma.values[0])

    @sigma.setter
    def sigma(self, value):
        if self._p_sigma is None:
            self._sigma = float(value)
        else:
            self._p_sigma[...] = float(value)

    def learnable_params(self):
        return [(p.name, p) for p in (self._p_edge0, self._p_gaps, self._p_sigma) if p is not None]

    def engine_values(self):
        if self._p_edge0 is None and self._p_sigma is None:
            return None
        return np.concatenate([self.bin_edges, [self.sigma]])

    def set_engine_gradient(self, g):
        """Chain rule from the gradient with respect to the raw cuts: g_{b_1} = sum_k g_k, g_{delta_j} = sum_{k > j} g_k."""
        g = np.asarray(g, dtype=float)
        K = self.K
        if self._p_edge0 is not None:
            self._p_edge0.gradient = [g[:K - 1].sum()]
        if self._p_gaps is not None:
            self._p_gaps.gradient = [g[j + 1:K - 1].sum() for j in range(K - 2)]
        if self._p_sigma is not None:
            self._p_sigma.gradient = [g[K - 1]]

    def kwargs(self):
        return {"K": self.K, "bin_edges": [float(b) for b in self.bin_edges], "sigma": self.sigma}


class Dirichlet(_Lik):
    """Compositions (the reference's likelihoods/dirichlet.py is a constructor only; the model is DESIGN 9d): a row of Y is
    y = (y_1 .. y_K) on the open simplex, K latent functions, alpha_k = clip(exp(f_k), 1e-9, 1e9) -- the K-part generalisation of
    Beta.  `K` comes first, like Categorical; 2 <= K <= 4.  Y is (N, K): every y_k must be finite and > 0 and every row must sum to
    1 within 1e-6, so zeros have to be replaced by the caller (as is usual for compositions) before the data is handed over.
    `predictive` returns the mean and variance of every part, (N, K) each; `samples` returns (N, K).  Where every alpha_k sits at
    the lower clip all K Gamma variates underflow and `samples` returns a vertex of the simplex (parts that are exactly 0 and 1, the
    limit of the distribution): such draws have to be moved off the boundary like any other zeros before they are used as data.
    The link is fixed (`gp_link` is accepted for the reference's signature and not used)."""
    name = "Dirichlet"

    def __init__(self, K, gp_link=None):
        if int(K) != K or not 2 <= int(K) <= 4:
            raise ValueError("Dirichlet: K must be an integer in 2 .. 4, got %r" % (K,))
        self.K = int(K)

    def kwargs(self):
        return {"K": self.K}

    def get_metadata(self):
        return self.K, self.K, self.K

    def ismulti(self):
        return True


class NegBinomial(_Lik):
    """Heteroscedastic Negative Binomial for over-dispersed counts (not in the reference; the model is DESIGN 9h): f0 = log of the
    mean mu, f1 = log of the dispersion ("size") r = clip(exp(f1), 1e-9, 1e9), so that Var[y | f] = mu + mu^2 / r and f1 -> +inf is
    Poisson.  Y is one column of non-negative integers (anything else is refused by the library).  There is no parameter of its
    own: the dispersion is the second latent function.  `predictive` is a closed form; `samples` draws the Gamma-Poisson mixture.
    The links are fixed (`gp_link` is accepted for the reference's signature and not used)."""
    name = "NegBinomial"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Weibull(_Lik):
    """Weibull time-to-event likelihood with right-censoring (not in the reference; the model is DESIGN 9i): f0 = log of the scale
    lambda, f1 = log of the shape k = clip(exp(f1), 1e-3, 1e3).  Y is (N, 2): the time y > 0 and the event indicator, exactly 1.0
    (the event was observed at y) or 0.0 (right-censored: the event is later than y; the row then contributes its log survival
    probability).  Anything else is refused by the library.  There is no parameter of its own: the shape is the second latent
    function.  `predictive` is the mean and variance of the event time, `samples` draws event times (N, 1), never censored, and
    `log_predictive` takes (N, 2) test rows, censored ones included.  The 20 x 20 rule is accurate while the variance of f1 stays
    small (DESIGN 9i has the table).  The links are fixed (`gp_link` is accepted for the reference's signature and not used)."""
    name = "Weibull"
    _dims = (2, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Binomial(_Lik):
    """Binomial likelihood with per-row trial counts (not in the reference; the model is DESIGN 9l): k successes out of n trials with
    p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9), Bernoulli's link and clip, so that a row (k, n) is exactly n Bernoulli rows collapsed into
    one.  Y is (N, 2): (k, n), integers with 1 <= n <= 1e9 and 0 <= k <= n; anything else is refused by the library.  `predictive` and
    `samples` receive no y: they describe a count out of `pred_trials` trials (an integer in 1 .. 1e9).  `log_predictive` and
    `log_predictive_density` take (N, 2) test rows.  There is no parameter to learn, and the predictive cdf / quantiles are not built.
    The link is fixed (`gp_link` is accepted for the reference's signature and not used)."""
    name = "Binomial"
    _dims = (2, 1, 1)

    def __init__(self, gp_link=None, pred_trials=1):
        self.pred_trials = pred_trials

    def kwargs(self):
        return dict(pred_trials=self.pred_trials)


class BetaBinomial(Binomial):
    """Beta-Binomial likelihood, Binomial's over-dispersed sibling: k successes out of n trials whose success probability is
    itself Beta(a, b), a = clip(exp(f0), 1e-9, 1e9), b = clip(exp(f1), 1e-9, 1e9) (Beta's links and clips).  Mean n a / (a + b), variance
    n mu (1 - mu) (a + b + n) / (a + b + 1): a + b -> inf is the Binomial.  Y, `pred_trials`, `predictive`, `samples` and the log
    predictive routines as Binomial's."""
    name = "BetaBinomial"
    _dims = (2, 2, 1)


class ZIPoisson(_Lik):
    """Zero-inflated Poisson for counts with more zeros than any rate explains (not in the reference; the model is DESIGN 9n): a
    structural zero with probability pi = clip(e^f1 / (1 + e^f1), 1e-9, 1 - 1e-9) (Bernoulli's link and clip), else a Poisson count of
    rate lambda = exp(f0) (Poisson's link): p(0 | f) = pi + (1 - pi) exp(-lambda), p(y | f) = (1 - pi) Poisson(y | lambda) for y >= 1.  Y is
    one column of non-negative integers (anything else is refused by the library).  There is no parameter of its own: the share of
    structural zeros is the second latent function.  `predictive` gives the mean and variance of a count, `samples` draws from the
    mixture; the predictive cdf / quantiles are not built.  The links are fixed (`gp_link` is accepted for the reference's signature
    and not used)."""
    name = "ZIPoisson"
    _dims = (1, 2, 1)

    def __init__(self, gp_link=None):
        pass


class Categorical(_Lik):
    name = "Categorical"

    def __init__(self, K, gp_link=None):
        self.K = int(K)

    def kwargs(self):
        return {"K": self.K}

    def get_metadata(self):
        return 1, self.K - 1, self.K - 1                   # categorical.py:287-291


class HetLikelihood(object):
    """het_likelihood.py:10-44,85-90."""

    def __init__(self, likelihoods_list, gp_link=None, name="heterogeneous_likelihood"):
        self.likelihoods_list = list(likelihoods_list)
        self.name = name

    def generate_metadata(self):
        t_index = np.arange(len(self.likelihoods_list))
        y_index, f_index, d_index, p_index = [], [], [], []
        for t, lik in enumerate(self.likelihoods_list):
            dim_y, dim_f, dim_p = lik.get_metadata()
            y_index += [t] * dim_y
            f_index += [t] * dim_f
            d_index += list(range(dim_f))
            p_index += [t] * dim_p
        return {"task_index": t_index, "y_index": np.int_(y_index), "function_index": np.int_(f_index),
                "d_index": np.int_(d_index), "pred_index": np.int_(p_index)}

    def num_output_functions(self, Y_metadata):
        return Y_metadata["function_index"].flatten().shape[0]

    def ismulti(self, task):
        return self.likelihoods_list[task].ismulti()

    def specs(self):
        return [(l.name, l.kwargs()) for l in self.likelihoods_list]

    def samples(self, F, Y_metadata):
        """het_likelihood.py:72-83: one draw per task from its likelihood, generated on the device."""
        return [l.samples(F[t], num_samples=1) for t, l in enumerate(self.likelihoods_list)]

    def var_exp(self, Y, mu_F, v_F, Y_metadata):
        return [l.var_exp(Y[t], mu_F[t], v_F[t]) for t, l in enumerate(self.likelihoods_list)]

    def predictive(self, mu_F_pred, v_F_pred, Y_metadata):
        """het_likelihood.py:133-148."""
        out = [l.predictive(mu_F_pred[t], v_F_pred[t]) for t, l in enumerate(self.likelihoods_list)]
        return [o[0] for o in out], [o[1] for o in out]

    def negative_log_predictive(self, Ytest, mu_F_star, v_F_star, Y_metadata, num_samples, seed=0):
        """het_likelihood.py:150-164."""
        logpred = 0.0
        for t, l in enumerate(self.likelihoods_list):
            logpred += l.log_predictive(Ytest[t], mu_F_star[t], v_F_star[t], num_samples, seed=seed + t)
        return -logpred

    def log_predictive_density(self, Ytest, mu_F, v_F, Y_metadata=None, gh_T=0):
        """Per-task list of (N_t,) deterministic per-row log predictive densities; one RuntimeWarning per call when some
        row's effective number of nodes is below LPD_ESS_WARN."""
        from .engine import log_predictive_density_rows
        out = [log_predictive_density_rows(l.name, Ytest[t], mu_F[t], v_F[t], gh_T=gh_T, return_ess=True, **l.kwargs())
               for t, l in enumerate(self.likelihoods_list)]
        warn_low_ess([o[1] for o in out], self.specs())
        return [o[0] for o in out]

    def _predq_tasks(self, tasks):
        from .engine import predq_require
        tasks = list(range(len(self.likelihoods_list))) if tasks is None else [int(t) for t in tasks]
        for t in tasks:                                      # (every refusal before the first launch)
            predq_require(self.likelihoods_list[t].name)
        return tasks

    def predictive_cdf(self, Ytest, mu_F, v_F, Y_metadata=None, return_sf=False, tasks=None, gh_T=0):
        """One (N_t,) cdf -- or (cdf, sf) pair -- per requested task; the lists are indexed by task.  tasks=None: all tasks;
        NotImplementedError when one of them has no predictive cdf."""
        return [self.likelihoods_list[t].predictive_cdf(Ytest[t], mu_F[t], v_F[t], gh_T=gh_T, return_sf=return_sf)
                for t in self._predq_tasks(tasks)]

    def predictive_quantiles(self, mu_F, v_F, probs, Y_metadata=None, tasks=None, gh_T=0):
        """One (N_t, len(probs)) array of quantiles per requested task; probs are probabilities in (0, 1)."""
        return [self.likelihoods_list[t].predictive_quantiles(mu_F[t], v_F[t], probs, gh_T=gh_T) for t in self._predq_tasks(tasks)]

    def var_exp_derivatives(self, Y, mu_F, v_F, Y_metadata):
        out = [l.var_exp_derivatives(Y[t], mu_F[t], v_F[t]) for t, l in enumerate(self.likelihoods_list)]
        return [o[0] for o in out], [o[1] for o in out]
