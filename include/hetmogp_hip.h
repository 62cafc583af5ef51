/*
 * hetmogp_hip.h -- C ABI of the MI355X-native SVI engine for heterogeneous multi-output GPs.
 *
 * Drop-in boundary for ONE hot path of pmorenoz/HetMOGP: the ELBO-and-gradient evaluation that the
 * reference performs in SVMOGP.parameters_changed()  (hetmogp/svmogp.py:85-166), i.e.
 *   SVMOGPInf.inference()            hetmogp/svmogp_inf.py:23-109
 *     util.latent_funs_cov           hetmogp/util.py:181-200      (K_uu, jitchol, K_uu^-1)
 *     SVMOGPInf.calculate_q_f        hetmogp/svmogp_inf.py:186-225 (q(f_d) mean / variance)
 *     HetLikelihood.var_exp(_derivatives)  hetmogp/het_likelihood.py:101-131 -> likelihoods/<name>.py
 *     SVMOGPInf.calculate_KL         hetmogp/svmogp_inf.py:227-250
 *     SVMOGPInf.calculate_gradients  hetmogp/svmogp_inf.py:111-183
 *   + the parameter-gradient assembly hetmogp/svmogp.py:101-166, util.py:228-231,248-255.
 *
 * The reference has no FFI (it is pure Python over GPy); the binding a maintainer would add is the
 * ctypes stub shown in INTEGRATION.md.  Why the boundary sits at the OUTER level (parameters in,
 * parameter gradients out) and not at SVMOGPInf.inference(): the inner protocol returns dL_dKmn as
 * Q*Df dense M x N matrices (24.6 GB at N=200k, M=1024) for Python to reduce.
 *
 * Conventions: every array is C-contiguous float64 (int32 / int64 where stated) in HOST memory owned by
 * the caller; the engine copies in / out and keeps data and workspaces resident in HBM between calls.
 * One handle = one host thread = one HIP device.  Every function returns 0 on success or a negative
 * HMOGP_E_* code; hmogp_last_error() gives the message.  The library has no CPU fallback: without a
 * HIP device hmogp_create fails with HMOGP_E_NO_DEVICE.
 */
#ifndef HETMOGP_HIP_H
#define HETMOGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HMOGP_ABI_VERSION 8

/* likelihood ids (class names of /root/reference/likelihoods/<name>.py) */
enum {
  HMOGP_LIK_GAUSSIAN = 0,    /* gaussian.py     param = sigma (default 0.5)          dim_f = 1   */
  HMOGP_LIK_BERNOULLI = 1,   /* bernoulli.py                                          dim_f = 1   */
  HMOGP_LIK_HETGAUSSIAN = 2, /* hetgaussian.py                                        dim_f = 2   */
  HMOGP_LIK_CATEGORICAL = 3, /* categorical.py  param = K (labels 1..K)               dim_f = K-1 */
  HMOGP_LIK_POISSON = 4,     /* poisson.py                                            dim_f = 1   */
  HMOGP_LIK_EXPONENTIAL = 5, /* exponential.py                                        dim_f = 1   */
  HMOGP_LIK_GAMMA = 6,       /* gamma.py                                              dim_f = 2   */
  HMOGP_LIK_BETA = 7,        /* beta.py                                               dim_f = 2   */
  HMOGP_LIK_STUDENT = 8,     /* student.py      param = deg_free nu (finite, > 0)     dim_f = 2   */
  HMOGP_LIK_ORDINAL = 9,     /* ordinal.py      param = id from hmogp_ordinal_table   dim_f = 1   */
  HMOGP_LIK_DIRICHLET = 10,  /* dirichlet.py    param = K (2 .. HMOGP_DIRICHLET_MAXK)  dim_f = K, Y is [N, K] */
  HMOGP_LIK_NEGBINOMIAL = 11, /* (not in the reference)  no param (0.0 is passed and ignored)  dim_f = 2 */
  HMOGP_LIK_WEIBULL = 12,     /* (not in the reference)  no param (0.0 is passed and ignored)  dim_f = 2, Y is [N, 2] */
  HMOGP_LIK_BINOMIAL = 13,    /* (not in the reference)  param = trial count n* of predictive / sample (0.0: 1)  dim_f = 1, Y is [N, 2] */
  HMOGP_LIK_BETABINOMIAL = 14, /* (not in the reference)  param as Binomial's                                   dim_f = 2, Y is [N, 2] */
  HMOGP_LIK_ZIPOISSON = 15    /* (not in the reference)  no param (0.0 is passed and ignored)  dim_f = 2 */
};

/* Zero-inflated Poisson: counts with more zeros than a rate explains.  f0 = log of the rate lambda (Poisson's link),
 * f1 = logit of the structural-zero probability pi = clip(e^f1 / (1 + e^f1), 1e-9, 1 - 1e-9) (Bernoulli's link and clip):
 *   p(0 | f) = pi + (1 - pi) exp(-lambda),     p(y | f) = (1 - pi) Poisson(y | lambda) for y >= 1.
 * A row with y >= 1 is the sum of Poisson's 20-node rule over f0 and Bernoulli's (label 0) over f1; a row with y = 0 is the 20 x 20 rule.
 * Y is one column of finite, non-negative, integer-valued doubles; anything else is HMOGP_E_INVALID ("ZIPoisson" in the message) in
 * hmogp_set_task_data (the task keeps its previous data) and in every building block that takes y (hmogp_var_exp[_ex],
 * hmogp_log_predictive, hmogp_log_predictive_gh), there before the device is asked for.  The family has no parameter of its own:
 * hmogp_lik_param_count answers 0 and hmogp_var_exp_dparam refuses it.  The predictive cdf and quantiles are refused (they need the
 * regularised incomplete gamma function, like Poisson's).  New enum value only: ABI version 8 stays. */

/* Binomial and Beta-Binomial: k successes out of n trials, n the row's own.  Y is [N, 2] row-major: (k, n), both finite,
 * integer-valued doubles with 1 <= n <= 1e9 and 0 <= k <= n.  With lc = lgamma(n+1) - lgamma(k+1) - lgamma(n-k+1):
 *   Binomial      one function, Bernoulli's link and clip p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9):
 *                   log p(k | n, f) = lc + k log p + (n - k) log(1 - p)            (a row (k, n) is n Bernoulli rows collapsed into one)
 *   BetaBinomial  two functions, Beta's links and clips a = clip(exp(f0), 1e-9, 1e9), b = clip(exp(f1), 1e-9, 1e9), s = a + b:
 *                   log p(k | n, f) = lc + G(k, a) + G(n - k, b) - G(n, s),        G(y, r) = lgamma(y + r) - lgamma(r)
 *                 the over-dispersed sibling: mean n a / s, variance n (a / s) (b / s) (s + n) / (s + 1).
 * Anything else in Y is HMOGP_E_INVALID (the family's name in the message) in hmogp_set_task_data (the task keeps its previous data) and
 * in every building block that takes y (hmogp_var_exp[_ex], hmogp_log_predictive, hmogp_log_predictive_gh, whose y is [N, 2] as well).
 * lik_param is the trial count n* of hmogp_predictive and hmogp_sample, which receive no y: an integer-valued double in 1 .. 1e9, 0.0
 * meaning 1; anything else is HMOGP_E_INVALID in hmogp_create and in every building block.  It is ignored wherever y carries n.
 * hmogp_sample writes counts [N, 1]; hmogp_predictive the mean and variance of a count out of n* trials.  Neither family has a parameter
 * of its own: hmogp_lik_param_count answers 0 and hmogp_var_exp_dparam refuses them.  The predictive cdf and quantiles are refused (they
 * need the regularised incomplete beta function).  New enum values only: ABI version 8 stays. */

/* Weibull with right-censoring: times to an event that may be only partly observed.  f0 = log of the scale lambda,
 * f1 = log of the shape k = clip(exp(f1), 1e-3, 1e3).  Y is [N, 2] row-major: (y, delta), y finite and > 0, delta exactly 1.0 (the
 * event was observed at y) or 0.0 (right-censored: the event is later than y).  With z = min(k (log y - f0), 680), e = exp(z):
 *   log p(y, delta | f) = delta (log k - log y + z) - e       (delta = 0: the log survival function -e).
 * Anything else in Y is HMOGP_E_INVALID ("Weibull" in the message) in hmogp_set_task_data (the task keeps its previous data) and in
 * every building block that takes y (hmogp_var_exp[_ex], hmogp_log_predictive, whose y is [N, 2] as well).  hmogp_sample writes
 * event times [N, 1] (never censored); hmogp_predictive the mean and variance of the event time.  The family has no parameter of its
 * own: hmogp_lik_param_count answers 0 and hmogp_var_exp_dparam refuses it.  New enum value only: ABI version 8 stays. */

/* Negative Binomial: counts with their own dispersion, f0 = log of the mean mu, f1 = log of the size
 * r = clip(exp(f1), 1e-9, 1e9), Var[y | f] = mu + mu^2 / r (f1 -> +inf is Poisson):
 *   log p(y | f) = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + y z - (r + y) softplus(z),   z = f0 - log r.
 * Y is one column of finite, non-negative, integer-valued doubles; anything else is HMOGP_E_INVALID ("NegBinomial" in the message) in
 * hmogp_set_task_data and in every building block that takes y (hmogp_var_exp[_ex], hmogp_log_predictive).  The family has no
 * parameter of its own: hmogp_lik_param_count answers 0 and hmogp_var_exp_dparam refuses it.  New enum value only: ABI version 8 stays. */

/* Ordinal (ordered probit): most classes K of one table, and most distinct tables one process can register */
#define HMOGP_ORDINAL_MAXK 32
#define HMOGP_ORDINAL_MAXTABLES 4096

/* Dirichlet (the reference's likelihoods/dirichlet.py is a constructor only): a row's observation is a composition
 * y = (y_1 .. y_K) on the open simplex, K latent functions, alpha_k = clip(exp(f_k), 1e-9, 1e9), A = sum_k alpha_k:
 *   log p(y | f) = lgamma(A) - sum_k lgamma(alpha_k) + sum_k (alpha_k - 1) log y_k.
 * It is the one family whose Y has more than one column: wherever another family passes y [N], a Dirichlet task passes
 * Y [N, K] row-major (hmogp_set_task_data, hmogp_var_exp[_ex], hmogp_log_predictive), and hmogp_sample writes [N, K].  A y_k that
 * is not finite, is <= 0, or a row with |sum_k y_k - 1| > 1e-6 is HMOGP_E_INVALID (zeros must be replaced by the caller), and so
 * is a lik_param that is not an integer in 2 .. HMOGP_DIRICHLET_MAXK, in hmogp_create and in every building block.  The bound on
 * K is the 10^K nodes of the tensor rule and the per-wave table of the quadrature kernels. */
#define HMOGP_DIRICHLET_MAXK 4

/* error codes; the Python facade maps them onto the reference's exception types */
enum {
  HMOGP_OK = 0,
  HMOGP_E_INVALID = -1,     /* bad argument                                                        */
  HMOGP_E_NO_DEVICE = -2,   /* no HIP device / HIP runtime error                                    */
  HMOGP_E_NOT_PD = -3,      /* LinAlgError("not positive definite, even with jitter.") / non-positive
                               diagonal -- GPy jitchol, reached from util.py:198                    */
  HMOGP_E_SQI_UNSTABLE = -4,/* ValueError("Sqi: Cholesky representation unstable") svmogp_inf.py:126 */
  HMOGP_E_STATE = -5,       /* call order violated (finish without begin, data not set, ...)        */
  HMOGP_E_COMM = -6         /* RCCL not loadable / a collective failed (hmogp_comm_*); ABI version 4  */
};

/* output flags (hmogp_outputs.flags) */
#define HMOGP_FLAG_V_NEGATIVE 1u /* some v_fd < 0: the reference prints 'v negative!' (svmogp_inf.py:221) */
#define HMOGP_FLAG_ILL_CONDITIONED 2u /* ABI v6: hmogp_outputs.cond_est of some latent is beyond what this engine's mode keeps within
   the north-star's element-wise 1e-5 of the reference: > 5e2 without HMOGP_CFG_STRICT_QF (cond(K_uu) ~ 1e4 and more: take the
   strict mode), > 1e6 with it (cond beyond the ~2e7 that GPy's jitter rung 0 leaves: the reference's own numbers move by more than 1e-5 with the last bit of its
   covariance there).  The reference has no such diagnostic (GPy's jitchol only reports a failed factorisation).              */

/* Reference quirks (hmogp_config.quirks).  A set bit reproduces the reference's behaviour, a cleared
 * bit gives the mathematically exact quantity.  HMOGP_QUIRKS_REFERENCE (all set) is what parity is measured against;
 * HMOGP_QUIRKS_EXACT (0) makes every returned gradient the true gradient of the returned ELBO (finite-difference
 * tested), which is what a quasi-Newton optimiser needs.                                                          */
#define HMOGP_QUIRK_GAMMA_BETA_PI 1u   /* Q1: Gamma / Beta var_exp and derivatives are 1/pi x the 2-D quadrature
                                          (gamma.py:110,139-141; beta.py:113,142-144); exact: the quadrature itself */
#define HMOGP_QUIRK_CATEGORICAL_DM 2u  /* Q2: Categorical d var_exp / dm = onehot(y)[d] - 1, independent of f
                                          (categorical.py:102-113); exact: E[onehot(y)[d] - softmax_d(f)]            */
#define HMOGP_QUIRK_STALE_W 4u         /* Q3: chain factors W0 / kappa0 (construction-time copies, svmogp.py:98,141,143,
                                          156) are honoured; exact: hmogp_params.W0 / kappa0 are ignored (= W / kappa) */
#define HMOGP_QUIRK_W_DIAG 8u          /* Q4: dW from the K_ff diagonal = W * sum(gv)   (util.py:230); exact:
                                          2 * W * variance_q * sum(gv)                                               */
#define HMOGP_QUIRK_KAPPA_DIAG 16u     /* Q5: dkappa = sum(gv)  (util.py:231); exact: variance_q * sum(gv)            */
#define HMOGP_QUIRKS_REFERENCE 31u
#define HMOGP_QUIRKS_EXACT 0u

/* gradient-group mask (hmogp_params.group_mask): which parameter groups receive a gradient.  Mirrors the
 * VEM gating of svmogp.py:104-110,131-137,145-151,160-166 and Z.is_fixed (:153,158).                    */
#define HMOGP_GROUP_QU 1u     /* m_u, L_u            (zeroed in stochastic M-steps)                 */
#define HMOGP_GROUP_HYPER 2u  /* variance, lengthscale, W, kappa (zeroed in stochastic E-steps)      */
#define HMOGP_GROUP_Z 4u      /* inducing inputs     (zeroed in stochastic E-steps or when fixed)    */
#define HMOGP_GROUP_ALL 7u

typedef struct hmogp_engine* hmogp_handle;

/* Static description of the model: SVMOGP.__init__ (svmogp.py:17-79) + HetLikelihood.generate_metadata
 * (het_likelihood.py:24-44).                                                                          */
typedef struct {
  int32_t abi_version;      /* HMOGP_ABI_VERSION                                                     */
  int32_t T;                /* number of likelihoods / tasks  = len(Y)                               */
  int32_t Q;                /* number of latent GPs u_q       = len(kern_list)                       */
  int32_t M;                /* inducing points per latent GP  = Z.shape[0]                           */
  int32_t P;                /* input dimension (Xdim)                                                */
  int32_t Df;               /* number of latent parameter functions f_d = sum_t dim_f(t)             */
  const int32_t* lik_id;    /* [T]  HMOGP_LIK_*                                                      */
  const double* lik_param;  /* [T]  sigma (Gaussian) | K (Categorical) | ignored                     */
  const int32_t* f_index;   /* [Df] task owning function d      (Y_metadata['function_index'])        */
  const int32_t* d_index;   /* [Df] column of d inside its task (Y_metadata['d_index'])               */
  int32_t device;           /* HIP device ordinal                                                    */
  int64_t chunk_rows;       /* rows streamed per pass, across tasks (0 = default: up to 2^20, less when
                               2 * Q * rows * M * 8 bytes of N x M workspace would exceed ~64 GB)     */
  uint32_t flags;           /* HMOGP_CFG_*                                                           */
  uint32_t quirks;          /* HMOGP_QUIRK_* mask; HMOGP_QUIRKS_REFERENCE reproduces the reference             */
} hmogp_config;
/* Engine limits (hmogp_create fails with HMOGP_E_INVALID beyond them): 1 <= P <= 4 input dimensions (the distance
 * kernels are instantiated per P); Q <= 8 latent GPs; dim_f <= 8 functions per likelihood (Categorical K <= 9);
 * exact-zero windows: M <= 8192.  T, M, Df and the row counts are bounded by device memory only.                 */

/* hmogp_config.flags */
#define HMOGP_CFG_STRICT_QF 8u /* ABI v6, opt-in: STRICT q(f).  The reference forms q(f_d) and the row side of its gradients through
   A = K_fu K_uu^-1 obtained by triangular solves against Luu (dpotrs, svmogp_inf.py:214-218; A^T alpha, A^T diag(beta) A and
   A (S K_uu^-1 - I) at :144-161); the default path uses the algebraically equal explicit C_q = K_uu^-1 S K_uu^-1 - K_uu^-1, which
   differs from that by ~cond(K_uu) * 2^-53.  Once GPy's jitter ladder is taken (cond ~ 1e7) the default path's g_W / g_kappa / g_Z
   are 1e-4 .. 1e-3 away from the reference's; with this flag the engine follows the reference's forms (two blocked triangular
   solves against Luu, the Gram of A, ...) and stays within 1e-5 element-wise there (tests/test_gpu_ladder.py).  Regular kernels
   only (no fused small-model path), excludes HMOGP_CFG_EXACT_ZERO_WINDOWS.  bench.py's `value` never uses it.
   (ABI v8) Cost at the headline size: 1.6x the default step for an evaluation that asks for the q(u) gradients only (136 vs 84 ms),
   1.8x for a full-gradient evaluation (213 vs 119.5 ms; 2.5x in ABI v7) while the condition estimate of K_uu is <= 1e6 -- GPy's whole
   jitter-ladder regime --, 2.2x beyond (263 ms).  Up to 1e6 an evaluation takes the ONE-SOLVE form: only the forward substitution
   X = K_fu Luu^-T touches the n x M side, the backward half of dpotrs sits in M x M factors (A m = X (Luu^-1 m), A L_q =
   X (Luu^-1 L_q), rowsum(A .* K_fu) = rowsum(X .* X), A^T diag(b) A = Luu^-T (X^T diag(b) X) Luu^-1, A (S K_uu^-1 - I) =
   X (Luu^-1 (S K_uu^-1 - I))); beyond it the literal two-solve form (the two are equally far from the reference's
   operations up to there, and the one-solve form drifts out of the reference's own sensitivity beyond).                       */
#define HMOGP_CFG_NO_SMALL_PATH 4u /* ABI v5: keep the regular kernels and three streams also for small models (M <= 64 would
                                    * otherwise take the fused small-model kernels, M <= 128 with <= 65536 rows one stream): A/B
                                    * comparisons of the two paths inside one process (tests)                                */
#define HMOGP_CFG_CACHE_KUU 2u /* opt-in: reuse K_uu, its Cholesky factor and inverse while (Z, variance, lengthscale,
   forced rungs) are bit-identical to the previous evaluation's (VEM / SVI E-steps only move q(u)).  Off by default and
   never used by bench.py, whose steps re-evaluate identical parameters.                                          */
#define HMOGP_CFG_EXACT_ZERO_WINDOWS 1u /* opt-in: skip the parts of K_uf = k(X,Z) that are EXACTLY 0.0 in float64
   (exp underflow beyond ~38.6 lengthscales).  For spatially sorted inputs K_uf is banded and the row pass only touches
   the band; every skipped term is a product with an exact zero, so ELBO and gradients are unchanged (tested equal to
   the dense path); unsorted inputs fall back to dense ranges on the device.  Default off: the dense path is what
   bench.py reports as `value`.                                                                                  */

/* All model parameters of one evaluation: the arrays paramz hands to parameters_changed().             */
typedef struct {
  const double* Z;            /* [M, Q*P]  block q = inducing inputs of u_q (svmogp.py:52)            */
  const double* m_u;          /* [M, Q]    q_u_means                  } both NULL: use the device-resident q(u)  */
  const double* L_flat;       /* [M(M+1)/2, Q] q_u_chols, GPy row-major tril packing } (hmogp_qu_load / _adadelta) */
  const double* variance;     /* [Q]  RBF variance of k_q                                             */
  const double* lengthscale;  /* [Q]  RBF lengthscale of k_q                                          */
  const double* W;            /* [Q, Df] live coregionalisation weights  B_list[q].W                  */
  const double* kappa;        /* [Q, Df] live kappa                      B_list[q].kappa              */
  const double* W0;           /* [Q, Df] or NULL (= W): construction-time W_list used for the chain
                                 factors at svmogp.py:98,141,143,156             */
  const double* kappa0;       /* [Q, Df] or NULL (= kappa)                                            */
  const double* batch_scale;  /* [T] or NULL (= 1): N_all[t] / N_batch[t]  (svmogp.py:89-90)          */
  const int64_t* row_begin;   /* [T] or NULL (= 0):   first row of task t used in this evaluation     */
  const int64_t* row_end;     /* [T] or NULL (= N_t): one past the last row (contiguous minibatch
                                 slices of util.py:52-72; also the row shard of this rank)            */
  const int32_t* forced_rung; /* [Q] or NULL: -2 = run GPy's jitter ladder, -1 = no jitter,
                                 k>=0 = jitter mean(diag)*1e-6*10^k (compare CPU/GPU at equal rung)   */
  uint32_t group_mask;        /* HMOGP_GROUP_*                                                        */
  uint32_t eval_flags;        /* HMOGP_EVAL_* of THIS evaluation (0 = none; (ABI v8) unknown bits are refused
                                 with HMOGP_E_INVALID: zero the struct before filling it)   (ABI version 6) */
} hmogp_params;
#define HMOGP_EVAL_STRICT_QF 1u /* run this evaluation in the strict q(f) mode (see HMOGP_CFG_STRICT_QF) whatever the engine was
   created with: lets a caller re-evaluate, and go on evaluating, in that mode once hmogp_outputs.flags reported
   HMOGP_FLAG_ILL_CONDITIONED -- the facade's strict_qf="auto".  Its extra workspaces are allocated at the first such call. */
#define HMOGP_EVAL_NO_G_L 2u /* (ABI v7) the gradient of q(u)'s Cholesky factor is not wanted from this evaluation: dL/dS L and its packing
                             * are skipped (outputs.g_L_u, if given, is zero-filled).  A natural-gradient E-step consumes dL/dS and dL/dm
                             * only (hmogp_natgrad_step / hmogp_qu_natgrad*).  hmogp_qu_adadelta phase 1 refuses to follow such an
                             * evaluation (HMOGP_E_STATE).  Ignored by the fused small-model path (M <= 64), which forms it anyway. */

typedef struct {
  double* elbo;          /* [1]   log_marginal (svmogp_inf.py:88)                                     */
  double* g_m_u;         /* [M, Q]                                                                    */
  double* g_L_u;         /* [M(M+1)/2, Q]                                                             */
  double* g_variance;    /* [Q]                                                                       */
  double* g_lengthscale; /* [Q]                                                                       */
  double* g_W;           /* [Q, Df]                                                                   */
  double* g_kappa;       /* [Q, Df]                                                                   */
  double* g_Z;           /* [M, Q*P]                                                                  */
  double* dL_dS;         /* [Q, M, M] or NULL: dL/dS_q (svmogp_inf.py:169), for natural gradients     */
  int32_t* rung;         /* [Q] jitter rung taken per latent (-1 = none)                              */
  uint32_t* flags;       /* [1] HMOGP_FLAG_*                                                          */
  double* kl;            /* [Q] or NULL: KL(q(u_q) || p(u_q)) per latent (calculate_KL, svmogp_inf.py:227-250);
                            elbo = (scaled data term) - sum_q kl[q]                      (ABI version 3) */
  double* cond_est;      /* [Q] or NULL: variance_q * max_i (K_uu^-1)_ii of the (jittered) prior covariance of latent q: a lower
                            bound of its condition number, 30-150x below it for RBF kernels          (ABI version 6) */
} hmogp_outputs;

/* ---- life cycle ------------------------------------------------------------------------------------ */
int hmogp_create(const hmogp_config* cfg, hmogp_handle* out);
void hmogp_destroy(hmogp_handle h);
const char* hmogp_last_error(hmogp_handle h); /* h may be NULL: error of the last failed hmogp_create    */
int hmogp_abi_version(void);

/* Upload (replace) the full data of task t: X [N, P], Y [N] (Xmulti_all[t], Ymulti_all[t]).  A Dirichlet task's Y is [N, K]
 * row-major; it is checked (see HMOGP_DIRICHLET_MAXK) before the task's state changes.                                  */
int hmogp_set_task_data(hmogp_handle h, int32_t t, const double* X, const double* Y, int64_t N);

/* ---- the hot path ----------------------------------------------------------------------------------- */
/* One full evaluation = parameters_changed(): ELBO + all parameter gradients (single device).           */
int hmogp_elbo_grad(hmogp_handle h, const hmogp_params* p, hmogp_outputs* out);
/* Small models (M <= 64, see HMOGP_CFG_NO_SMALL_PATH): the evaluation is a fixed launch sequence on one stream; the second
 * hmogp_elbo_grad with the same gradient gates / row ranges / forced rungs is captured into a hipGraph and every later one is a
 * replay (one hipGraphLaunch instead of ~35 API calls; the parameter VALUES travel through a page-locked image the graph's
 * upload node reads).  hmogp_graph_stats reports how many graphs were captured and how many evaluations were replays
 * (diagnostics / tests; environment HMOGP_SMALL_GRAPH=0 disables the mechanism).  ABI v5.                                  */
int hmogp_graph_stats(hmogp_handle h, int64_t* captures, int64_t* replays);

/* The same, split at the one exchange point of the path for row-sharded multi-GPU runs:
 *   begin  : upload parameters, replicated M x M pre-algebra, row pass over [row_begin,row_end) of every
 *            task -> additive statistic bundle left in device memory (synchronous at return);
 *   (caller sum-all-reduces the bundle in place across ranks, e.g. torch.distributed over RCCL)
 *   finish : replicated M x M post-processing of the bundle -> outputs.                                 */
int hmogp_step_begin(hmogp_handle h, const hmogp_params* p);
int hmogp_stats_buffer(hmogp_handle h, void** device_ptr, int64_t* count); /* float64 words            */
int hmogp_step_finish(hmogp_handle h, hmogp_outputs* out);
/* Host-staged access to the bundle (tests).  Between begin and finish H_q holds its LOWER triangle only (the row
 * pass fills nothing else; finish mirrors it), so sums of bundles of different row shards stay valid bundles.     */
int hmogp_stats_read(hmogp_handle h, double* host /* [count] */);
int hmogp_stats_write(hmogp_handle h, const double* host /* [count] */);
/* Wire format of the bundle = what actually travels in the exchange step: H_q is symmetric, so only its lower
 * triangle is sent -- [head 2+Df | per q: tril(H_q) row-major packed, M(M+1)/2 | r (M) | dZ (M*P) | sa | sl | swk (Df)]
 * = 12.7 MB instead of 25.2 MB at M = 1024, Q = 3.  Usage between begin and finish:
 *   hmogp_wire_pack(h);  all-reduce(sum, float64) the `count` words at `device_ptr` in place;  hmogp_wire_unpack(h);
 * pack / unpack are synchronous at return.  hmogp_wire_read / _write: host-staged variant (CPU backends, tests).   */
int hmogp_wire_buffer(hmogp_handle h, void** device_ptr, int64_t* count);
int hmogp_wire_pack(hmogp_handle h);
int hmogp_wire_unpack(hmogp_handle h);
int hmogp_wire_read(hmogp_handle h, double* host /* [count] */);
int hmogp_wire_write(hmogp_handle h, const double* host /* [count] */);

/* ---- the exchange step inside the library (ABI version 4) --------------------------------------------------------
 * The reference is single-process (no distributed code at all); the contract is SURVEY.md 8(e): rows are
 * sharded over one process per GPU and the additive bundle is sum-all-reduced ONCE per step.  With a communicator
 * attached the library does that itself: wire pack -> ncclAllReduce(sum, float64, in place) -> wire unpack, all enqueued
 * on the engine's own HIP stream between the row pass and the replicated post-processing -- no host synchronisation, no
 * second library's stream.  librccl is resolved at run time (dlopen by soname: in a process that already holds one,
 * e.g. PyTorch's, that copy is used), so single-GPU users do not need it.
 *   hmogp_comm_available   1 if librccl could be loaded, else 0 (no handle needed; never fails)
 *   hmogp_comm_unique_id   ncclGetUniqueId: ONE rank calls it and distributes the HMOGP_COMM_ID_BYTES bytes out of band
 *                          (torch.distributed broadcast, MPI, a file ...)
 *   hmogp_comm_init        ncclCommInitRank on the engine's device; collective: every rank calls it with the same id
 *   hmogp_comm_destroy     ncclCommDestroy (also done by hmogp_destroy)
 *   hmogp_comm_info        nranks / rank of the attached communicator (0 / -1 without one)
 * hmogp_elbo_grad_sharded (ABI v5) IS the row-sharded step: begin on this rank's rows -> exchange -> finish, one call, one
 * final host synchronisation; COLLECTIVE -- every rank of the communicator must call it.  hmogp_elbo_grad itself never
 * communicates, also with a communicator attached (ABI v4 keyed the collective on the communicator's presence: a debug
 * call on one rank would then block its peers).  hmogp_step_exchange is the middle part for callers that keep the
 * three-call form.  Failure semantics: a rank whose row pass fails before it could contribute ABORTS the communicator
 * (ncclCommAbort) so that the peers' collective ends with HMOGP_E_COMM instead of blocking; while a collective is in
 * flight the final wait polls ncclCommGetAsyncError and a deadline (environment HMOGP_COMM_TIMEOUT_S, default 600,
 * 0 = none) and aborts the communicator on either.  After an abort hmogp_comm_info reports 0 ranks.  The exchange is
 * category [8] of hmogp_last_timings.  A communicator of ONE rank runs the same three launches (used by the tests).   */
#define HMOGP_COMM_ID_BYTES 128
int hmogp_comm_available(void);
int hmogp_comm_unique_id(void* id /* [HMOGP_COMM_ID_BYTES] */);
int hmogp_comm_init(hmogp_handle h, int32_t nranks, int32_t rank, const void* id /* [HMOGP_COMM_ID_BYTES] */);
int hmogp_comm_destroy(hmogp_handle h);
int hmogp_comm_info(hmogp_handle h, int32_t* nranks, int32_t* rank);
int hmogp_step_exchange(hmogp_handle h);
int hmogp_elbo_grad_sharded(hmogp_handle h, const hmogp_params* p, hmogp_outputs* out);

/* ---- posterior / prediction (consumers: svmogp.py:238-251, 280-306) --------------------------------- */
/* woodbury_vector[q] = Kuu^-1 m_q  [Q, M];  woodbury_inv[q] = Kuu^-1 - Kuu^-1 S_q Kuu^-1  [Q, M, M]
 * of the parameters of the last evaluation.                                                             */
int hmogp_posterior_u(hmogp_handle h, double* woodbury_vector, double* woodbury_inv);
/* q(f_d) at new inputs for all functions: m [Nnew, Df], v [Nnew, Df] (= predictive_new's (mu, |var|)
 * before the abs; svmogp_inf.py:186-225 with X := Xnew), using the parameters of the last evaluation.   */
int hmogp_predict_f(hmogp_handle h, const double* Xnew, int64_t Nnew, double* m, double* v);

/* ---- natural-gradient update of q(u) (named in the north-star; the reference has no such step) ---------- */
/* From the gradients of the LAST finished evaluation (its group_mask must include HMOGP_GROUP_QU):
 *   S_q^-1 <- S_q^-1 - 2 gamma dL/dS_q ;  S_q^-1 m_q <- S_q^-1 m_q + gamma (dL/dm_q - 2 dL/dS_q m_q)
 * returns the new m_u [M, Q] and L_flat [M(M+1)/2, Q] (Cholesky of the new S_q, GPy packing).  HMOGP_E_NOT_PD if
 * the step leaves the positive-definite cone (nothing is modified: retry with a smaller gamma).  A successful step
 * invalidates posterior_u / predict_f until the next evaluation.                                                       */
int hmogp_natgrad_step(hmogp_handle h, double gamma, double* m_u_new, double* L_flat_new);
/* The same step applied IN PLACE to the device-resident q(u) of hmogp_qu_load (ABI v5): nothing but two info words crosses
 * PCIe; the next evaluation (m_u = L_flat = NULL) sees the updated q(u).  HMOGP_E_NOT_PD leaves the resident q(u) and the
 * gradients of the last evaluation untouched (the step only wrote scratch), so the caller can retry at once with a smaller
 * gamma.  After a successful step posterior_u / predict_f / another step need a new evaluation (HMOGP_E_STATE otherwise).  */
int hmogp_qu_natgrad(hmogp_handle h, double gamma);
/* (ABI v7) The same in-place step WITHOUT the host synchronisation.  Everything is enqueued, the commit into the resident q(u) is
 * decided on the device (a step that leaves the positive-definite cone writes nothing), and the call returns at once: the caller
 * can enqueue the next evaluation straight away -- its parameter upload, row staging and K_uf construction then run beside this
 * step's factorisation chain instead of behind a host round trip (0.3 ms per SVI iteration at M = 1024, Q = 3).
 * hmogp_qu_natgrad_status waits for the pending step (if any) and sets *taken = 1 if it was committed, 0 if it was refused (q(u)
 * unchanged; the gradients it was computed from are gone once a new evaluation has run: take a smaller step from the new ones).
 * At most one step may be pending (HMOGP_E_STATE); the synchronous entry points resolve a pending step first.              */
int hmogp_qu_natgrad_async(hmogp_handle h, double gamma);
int hmogp_qu_natgrad_status(hmogp_handle h, int32_t* taken);

/* ---- device-resident q(u) and its Adadelta state: the SVI loop without moving 2 x 12.6 MB per iteration ------ */
/* The reference's stochastic driver (util.py:321-329) runs climin.Adadelta over the flat optimiser vector, 98 % of which
 * is q(u) (m_u, L_u: 1.58 M numbers at M = 1024, Q = 3); its gradient is svmogp.py:188-199 (stochastic_grad).  These
 * entry points keep q(u), its gradient and the three Adadelta accumulators in HBM; the caller runs the same recurrence
 * on the few remaining parameters (Z, variance, W ...) on the host.  The device recurrence performs the same IEEE
 * operations in the same order as the host one, so the iterates are bit-identical.
 *   hmogp_qu_load      upload q(u) (zeroes the accumulators); evaluations with params.m_u = params.L_flat = NULL use it,
 *                      outputs.g_m_u / g_L_u may then be NULL (nothing is copied back)
 *   hmogp_qu_adadelta  phase 0: q(u) -= step2 of the previous iteration; step1 = momentum * step; q(u) -= step1
 *                               (before the gradient evaluation)
 *                      phase 1: gms = d gms + (1-d) g^2; step2 = sqrt(sms+o)/sqrt(gms+o) g rate (kept pending);
 *                               step = step1 + step2; sms = d sms + (1-d) step^2       with g = -dELBO/dq(u) of the last
 *                               evaluation, or 0 if its group_mask excluded HMOGP_GROUP_QU (the M-steps of svmogp.py:196)
 *   hmogp_qu_read      download q(u) as of the LAST EVALUATION (the second half-step of the last update still pending):
 *                      what the reference's model object holds between iterations -- climin updates its own vector, the
 *                      model is only written by stochastic_grad (svmogp.py:188)                                       */
int hmogp_qu_load(hmogp_handle h, const double* m_u, const double* L_flat);
int hmogp_qu_read(hmogp_handle h, double* m_u, double* L_flat);
int hmogp_qu_adadelta(hmogp_handle h, int32_t phase, double step_rate, double momentum, double decay,
                      double one_minus_decay, double offset);

/* ---- timing --------------------------------------------------------------------------------------- */
/* Milliseconds the kernels of the last evaluation spent, measured with HIP events on the engine's stream:
 * out[0] whole evaluation, [1] K_uf construction (rbf_cross_cov; + window kernels in the opt-in mode), [2] forward
 * N x M x M contraction incl. its fused row-statistics epilogue (ONE kernel per launch, all latents of a task chunk),
 * [3] combine of the row-statistic partials, [4] quadrature, [5] weighted Gram contraction (ONE kernel per launch),
 * [6] column statistics + slab reductions, [7] replicated M x M algebra, [8] the in-library exchange step (pack + RCCL
 * all-reduce + unpack; 0 without a communicator), [9] the triangular solves of the strict q(f) mode (trsm_panel_kernel /
 * trsm_diag_kernel + their update GEMMs; [2] then holds the mode's products T = A L_q and P~ = A (S K_uu^-1 - I) only),
 * [10] the strict mode's row-statistic kernels (0 in the default mode).  launches[i] = kernel launches behind out[i].  Both
 * arrays hold HMOGP_NTIMINGS entries (8 before ABI version 4, 9 before ABI version 8).                                */
#define HMOGP_NTIMINGS 11
int hmogp_last_timings(hmogp_handle h, double* out_ms /* [HMOGP_NTIMINGS] */, int64_t* launches /* [HMOGP_NTIMINGS] or NULL */);

/* ---- inner protocol, debug / parity mode (small N only) ------------------------------------------------ */
/* The raw gradient dictionary SVMOGPInf.inference returns (svmogp_inf.py:107, built at :130-171) for the LAST finished
 * evaluation, which must have used group_mask = HMOGP_GROUP_ALL and streamed all its rows in one pool (N_total <=
 * chunk_rows): dL_dKmm [Q, M, M] (:166-171); dL_dKmn = for q, for d: [M, N_t(d)] row-major, concatenated (:157-161);
 * dL_dKdiag = for q, for d: [N_t(d)], concatenated (:164).  N_t(d) = rows of the task owning function d in that
 * evaluation.  Any pointer may be NULL.  This is 8*Q*Df*M*N bytes -- the reason the product boundary is the outer
 * protocol; it exists so that the device's dL_dKmm / dL_dKmn can be compared with the reference's with nothing in
 * between.                                                                                                       */
int hmogp_debug_raw_grads(hmogp_handle h, double* dL_dKmm, double* dL_dKmn, double* dL_dKdiag);

/* ---- building blocks, exposed for parity tests ("inner protocol" at small sizes) ---------------------- */
/* K = variance * exp(-0.5 * |x - z|^2 / lengthscale^2), GPy RBF.K(X, Z) semantics (util.py:161,197).      */
int hmogp_rbf_cross_cov(int32_t device, const double* X, int64_t N, const double* Z, int32_t M, int32_t P,
                        double variance, double lengthscale, double* K /* [N, M] */);
/* The same with the rounding order selectable: exact = 1 is hmogp_rbf_cross_cov (GPy's r = sqrt(clip(r2))/l, used
 * for K_uu); exact = 0 is the variant the row pass uses for K_uf (clip(r2) * (1/l^2): no sqrt / divide per element,
 * <= 2 ulp of the exponent away).                                                                                 */
int hmogp_rbf_cross_cov_ex(int32_t device, const double* X, int64_t N, const double* Z, int32_t M, int32_t P,
                           double variance, double lengthscale, int32_t exact, double* K /* [N, M] */);
/* The exact-zero windows of K = k(X, Z) exactly as HMOGP_CFG_EXACT_ZERO_WINDOWS computes them for one row range and one latent
 * (a stateless view of the engine's own window kernels; still ABI v8).  X [N, P] row-major, Z [M, ldz] with the latent's inputs in
 * its first P columns (ldz >= P: pass hmogp_params.Z + q P with ldz = Q P), 1 <= M <= 8192, 1 <= P <= 4.
 *   rowwin [ceil(N / 128)][2]  per 128-row tile the column range [lo, hi) outside which every K[n][m] of the tile is exactly 0.0;
 *                              lo, hi multiples of 16, hi <= (M + 15) & ~15 (which may exceed M); [0, 0) = the tile has no non-zero
 *   colwin [ceil(M / 128)][2]  per 128-column block the row range [lo, hi) that holds the tiles touching it; [0, 0) = none
 * Inputs that are not banded (a tile inside a block's row range that does not touch the block) give the full ranges [0, (M+15)&~15)
 * and [0, N) everywhere.                                                                                                          */
int hmogp_kuf_windows(int32_t device, const double* X, int64_t N, int32_t P, const double* Z, int32_t ldz, int32_t M,
                      double lengthscale, int32_t* rowwin, int32_t* colwin);
/* Batched lower Cholesky with GPy's jitter ladder + inverse: A [Q,M,M] -> L, Ainv; rung[q] as above.     */
int hmogp_jitchol_inv(int32_t device, const double* A, int32_t Q, int32_t M, const int32_t* forced_rung,
                      double* L, double* Ainv, int32_t* rung);
/* (L L^T)^-1 from lower factors (GPy dpotri): L [Q,M,M] -> Sinv [Q,M,M].                                 */
int hmogp_potri(int32_t device, const double* L, int32_t Q, int32_t M, double* Sinv);
/* out [n, M] = dpotrs(L, B^T)^T = B (L L^T)^-1 for the n rows of B [n, M], L [M, M] lower (GPy util.linalg.dpotrs as
 * svmogp_inf.py:214 calls it): two blocked triangular solves, true substitution inside 32-column diagonal blocks -- the
 * building block of HMOGP_CFG_STRICT_QF.  ABI v6.                                                                      */
int hmogp_potrs_rows(int32_t device, const double* L, int32_t M, const double* B, int64_t n, double* out);
/* C = alpha * op(A) op(B) + beta * C on the FP64-MFMA GEMM; transA/transB in {0,1}; row-major.           */
int hmogp_gemm_f64(int32_t device, int32_t transA, int32_t transB, int32_t M, int32_t N, int32_t K,
                   double alpha, const double* A, int32_t lda, const double* B, int32_t ldb, double beta,
                   double* C, int32_t ldc);
/* Variational expectations of one likelihood: y [N] (Dirichlet: [N, K]), m,v [N, dim_f] -> ve [N], dm, dv [N, dim_f].
 * Here and in hmogp_predictive / hmogp_log_predictive / hmogp_sample / hmogp_create a Student deg_free that is not
 * finite and > 0 is HMOGP_E_INVALID.                                                                      */
int hmogp_var_exp(int32_t device, int32_t lik_id, double lik_param, int64_t N, const double* y,
                  const double* m, const double* v, double* ve, double* dm, double* dv);

/* Ordinal (ordered probit; the reference's likelihoods/ordinal.py is a constructor only, the model is DESIGN 9b): one latent
 * function f, labels 1..K, K - 1 cut points b_1 < ... < b_{K-1} (b_0 = -inf, b_K = +inf), fixed noise scale sigma:
 *   p(y = k | f) = Phi((b_k - f) / sigma) - Phi((b_{k-1} - f) / sigma).
 * Every entry point carries ONE double per task, so the K numbers of an Ordinal task are registered once: this call checks
 * them (2 <= K <= HMOGP_ORDINAL_MAXK; edges [K - 1] finite and strictly increasing; sigma finite and > 0), stores an
 * immutable copy in a process-wide table (thread-safe; an identical table gets the id it already has; at most
 * HMOGP_ORDINAL_MAXTABLES distinct tables, then HMOGP_E_INVALID) and writes to *lik_param_out the value to pass as
 * `lik_param` of an HMOGP_LIK_ORDINAL task to hmogp_create / hmogp_var_exp[_ex] / hmogp_predictive / hmogp_log_predictive /
 * hmogp_sample.  Any other lik_param is HMOGP_E_INVALID there, and so is a label y that is not an integer in 1..K
 * (hmogp_set_task_data, hmogp_var_exp[_ex], hmogp_log_predictive).  Needs no device.  hmogp_predictive returns the closed-form
 * moments of the label (mean = sum_k k P_k, var = sum_k k^2 P_k - mean^2; gh_T is ignored).                          */
int hmogp_ordinal_table(int32_t K, const double* edges, double sigma, double* lik_param_out);

/* The same under a quirk mask (HMOGP_QUIRK_GAMMA_BETA_PI, HMOGP_QUIRK_CATEGORICAL_DM).                            */
int hmogp_var_exp_ex(int32_t device, int32_t lik_id, double lik_param, uint32_t quirks, int64_t N, const double* y,
                     const double* m, const double* v, double* ve, double* dm, double* dv);

/* ---- Likelihood parameters: Gaussian sigma, Student deg_free, Ordinal cut points and sigma can be LEARNED.  All of it is
 * new symbols: the ABI version, the three structs and the eval_flags mask are unchanged, and an engine that never calls them behaves
 * as before.
 *
 * Per-row derivatives of the variational expectation with respect to the likelihood's own parameters (same rules as hmogp_var_exp:
 * closed form, GH20, 20 x 20).  y, m, v as for hmogp_var_exp, validated the same way; out is [N, C]:
 *   Gaussian C = 1: d ve / d sigma;   Student C = 1: d ve / d deg_free (the constant's derivative included);
 *   Ordinal  C = 3: d ve / d lo, d ve / d hi, d ve / d sigma for the row's OWN two cut points (0 for an infinite one).
 * Any other family: HMOGP_E_INVALID.                                                                             */
int hmogp_var_exp_dparam(int32_t device, int32_t lik_id, double lik_param, int64_t N, const double* y, const double* m,
                         const double* v, double* out);
/* Number of parameters of task t: 1 (Gaussian: sigma), 1 (Student: deg_free), K (Ordinal: b_1 .. b_{K-1}, then sigma), 0 otherwise. */
int hmogp_lik_param_count(hmogp_handle h, int32_t t, int32_t* n);
/* New values for task t's parameters (n = hmogp_lik_param_count), validated like the constructors (sigma, deg_free finite and > 0;
 * cut points finite and strictly increasing); on HMOGP_E_INVALID the task is unchanged.  An Ordinal task keeps a private table from
 * here on -- the registry of hmogp_ordinal_table is not touched, any number of updates is fine -- and its rows' cut points are
 * rebuilt on the device from the resident labels.  Captured small-model graphs are dropped.                       */
int hmogp_set_lik_params(hmogp_handle h, int32_t t, const double* values, int32_t n);
/* Persistent switch, default off.  While it is on, every evaluation whose group_mask contains HMOGP_GROUP_HYPER also computes
 * batch_scale[t] * sum_rows d ve / d theta for every task with parameters (one row kernel per family behind the quadrature,
 * block partials summed in a fixed order: two evaluations give the same bits).  hmogp_step_begin and hmogp_elbo_grad_sharded
 * return HMOGP_E_INVALID while it is on: the bundle and the wire format do not carry this gradient.                 */
int hmogp_lik_grad_enable(hmogp_handle h, int32_t on);
/* d ELBO / d theta of the last evaluation, layout of hmogp_set_lik_params (Ordinal: with respect to the raw cut points and sigma).
 * Zeros when the switch is off or the evaluation's group_mask had no HMOGP_GROUP_HYPER.                            */
int hmogp_lik_grad_read(hmogp_handle h, int32_t t, double* g, int32_t n);

/* Predictive mean / variance of y under q(f) = N(m, diag v): the reference's `<likelihood>.predictive(m, v)`
 * (e.g. bernoulli.py:113-128, gamma.py:196-238, categorical.py:224-269), consumed by HetLikelihood.predictive
 * (het_likelihood.py:133-148).  m, v [N, dim_f] -> mean, var [N, dim_p] (dim_p = K-1 for Categorical, K for Dirichlet, else 1).
 * gh_T: Gauss-Hermite order, 20 (fresh reference instance), 10 (instance whose var_exp ran first: GPy caches the
 * first rule), 0 = the reference's default for a fresh instance.                                              */
int hmogp_predictive(int32_t device, int32_t lik_id, double lik_param, int32_t gh_T, int64_t N, const double* m,
                     const double* v, double* mean, double* var);

/* Monte-Carlo log predictive density per test row (the inner part of `<likelihood>.log_predictive`, e.g.
 * bernoulli.py:130-144): log_pred[n] = -log(S) + logsumexp_s log p(y_n | f_s), f_s ~ N(m_n, diag v_n), S = num_samples,
 * counter-based generator seeded by `seed` (reproducible; a different stream than NumPy's).  The reference then returns
 * (1/S) * sum_n log_pred[n] and HetLikelihood.negative_log_predictive (het_likelihood.py:150-164) negates the sum over
 * tasks -- done by the caller.  Defined for Gaussian, Bernoulli, HetGaussian, Poisson, Exponential, Categorical,
 * Student, Ordinal, Dirichlet (y [N, K]).                                                                                 */
int hmogp_log_predictive(int32_t device, int32_t lik_id, double lik_param, int64_t N, int32_t num_samples, uint64_t seed,
                         const double* y, const double* m, const double* v, double* log_pred);

/* Deterministic log predictive density per test row, for all thirteen families -- Gamma and Beta included, which
 * hmogp_log_predictive refuses.  For q(f) = N(m_n, diag v_n) over the family's dim_f functions:
 *   lpd[n] = log sum_nodes (prod_d w_{i_d}) p(y_n | f_node),   f_node,d = m_d + sqrt(2 v_d) x_{i_d},
 * the Gauss-Hermite tensor rule with gh_T nodes per dimension and weights normalised to sum 1 (gh_T = 0: the default, 20, but 10
 * for Categorical and Dirichlet, which accept 0 or 10 only; every other family 0, 10 or 20; anything else HMOGP_E_INVALID).
 * log p(y | f) is what hmogp_log_predictive evaluates per sample; Gamma and Beta: their densities with the families' links and
 * clips, no division by pi.  Gaussian is the closed form log N(y; m, sigma^2 + v) with the task's sigma (quirk Q6 belongs to the
 * Monte-Carlo routine only); HetGaussian integrates f0 analytically: gh_T nodes over f1 of log N(y; m0, v0 + safe_exp(f1)).
 * ess[n] (optional, NULL to skip) = (sum e)^2 / sum e^2 over the nodes' e = (prod w) p: the effective number of nodes.  A value
 * next to 1 means the likelihood is much narrower than q(f) and the fixed rule cannot resolve it: lpd is then unreliable.
 * Gaussian: +inf.  A row whose every node has p = 0: lpd = -inf, ess = NaN.  No seed, no sampling noise.
 * y, its layout per family and its checks are those of hmogp_var_exp / hmogp_log_predictive (Dirichlet [N, K], Weibull [N, 2]);
 * Gaussian with lik_param <= 0 means sigma = 0.5.  New symbols only: ABI version 8 stays.                                    */
int hmogp_log_predictive_gh(int32_t device, int32_t lik_id, double lik_param, int32_t gh_T, int64_t N, const double* y,
                            const double* m, const double* v, double* lpd /* [N] */, double* ess /* [N] or NULL */);
/* The same score for new rows (Xnew [Nnew, P], Ynew in the layout hmogp_set_task_data takes for task t, with its checks) of task t
 * of an engine: q(f) at Xnew is formed on the device as hmogp_predict_f forms it (same chunks, same strict / default mode), the
 * task's columns and |v| feed the rule directly with the task's CURRENT likelihood parameters (hmogp_set_lik_params), and only
 * lpd / ess [Nnew] come back.  HMOGP_E_STATE before the first evaluation; HMOGP_E_INVALID for a t out of range, a bad gh_T, or a
 * NULL pointer (ess excepted) with Nnew > 0.                                                                                  */
int hmogp_predict_log_density(hmogp_handle h, int32_t t, const double* Xnew, const double* Ynew, int64_t Nnew, int32_t gh_T,
                              double* lpd /* [Nnew] */, double* ess /* [Nnew] or NULL */);

/* Predictive cdf, survival function and quantiles per test row, over the nodes and normalised weights of
 * hmogp_log_predictive_gh: cdf[n] = sum_nodes w C(y_n | f_node), sf[n] = sum_nodes w S(y_n | f_node) with the family's conditional cdf C
 * and survival function S, each evaluated directly (never as 1 - the other: a tail of 1e-200 keeps its relative precision), links and
 * clips as in hmogp_log_predictive.  Built for the six families whose pair is closed-form in exp, expm1, log and erfc:
 *   Gaussian     closed form, z = (y - m) / sqrt(sigma^2 + v) (lik_param <= 0: sigma = 0.5): cdf = erfc(-z / sqrt 2) / 2, sf = erfc(z / sqrt 2) / 2
 *   HetGaussian  f0 integrated analytically, gh_T nodes over f1: z_j = (y - m0) / sqrt(v0 + safe_exp(f1_j))
 *   Bernoulli    p1 = sum w clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9), p0 = sum w (1 - that): (0, 1) for y < 0, (p0, p1) for 0 <= y < 1, (1, 0) for y >= 1
 *   Exponential  b = clip(safe_exp(-f), 1e-9, 1e9): (0, 1) for y <= 0, else S = exp(-y / b), C = -expm1(-y / b)
 *   Ordinal      closed form; y is the label c in 1 .. K (anything else: HMOGP_E_INVALID): P(Y <= c) = Phi((b_c - m) / sqrt(sigma^2 + v)), b_K = +inf
 *   Weibull      y is a TIME, [N] with no indicator column: (0, 1) for y <= 0, else k = shape(f1), z = min(k (log y - f0), 680), e = exp(z),
 *                S = exp(-e), C = -expm1(-e); the gh_T x gh_T tensor rule
 * Every other family is HMOGP_E_INVALID with the reason in the error string: Poisson, ZIPoisson and Gamma need a regularised incomplete gamma
 * function, Beta, Student and NegBinomial a regularised incomplete beta function, Categorical has no order, Dirichlet is multivariate.
 * gh_T: 0 (= 20), 10 or 20.  y [N], m, v [N, dim_f]; cdf, sf [N], either may be NULL.
 * Quantiles: q[n, i] for the nP <= HMOGP_QUANT_MAXP probabilities p[i]; a p outside (0, 1) gives NaN in its column.  Bernoulli and
 * Ordinal: the smallest point of the support whose cdf is >= p, as a double.  The others: the y with cdf(y) = p -- solved on the cdf for
 * p <= 1/2, on sf(y) = 1 - p otherwise; in y (Gaussian, HetGaussian) or in log y (Exponential, Weibull) -- by a bracketed Newton
 * iteration whose loops are bounded at compile time: a row makes at most 128 evaluations of the rule, and is NaN when that budget is
 * exhausted.  New symbols only: ABI version 8 stays.                                                                             */
#define HMOGP_QUANT_MAXP 8
int hmogp_predictive_cdf(int32_t device, int32_t lik_id, double lik_param, int32_t gh_T, int64_t N, const double* y, const double* m,
                         const double* v, double* cdf /* [N] or NULL */, double* sf /* [N] or NULL */);
int hmogp_predictive_quantile(int32_t device, int32_t lik_id, double lik_param, int32_t gh_T, int64_t N, int32_t nP,
                              const double* p /* [nP] */, const double* m, const double* v, double* q /* [N, nP] */);
/* The same for new rows of task t of an engine: q(f) at Xnew [Nnew, P] is formed on the device as hmogp_predict_f forms it (same
 * chunks, same strict / default mode, small or regular model); the task's columns and |v| feed the kernels directly, with the task's
 * CURRENT likelihood parameters and its private Ordinal table (hmogp_set_lik_params).  ynew is [Nnew] as above.  HMOGP_E_STATE
 * before the first evaluation; HMOGP_E_INVALID for an unsupported family, a bad gh_T, nP outside 1 .. HMOGP_QUANT_MAXP, a NULL pointer
 * (cdf / sf excepted) with Nnew > 0, a t out of range, or a bad Ordinal label -- every refusal before anything is launched.     */
int hmogp_predict_cdf(hmogp_handle h, int32_t t, const double* Xnew, const double* ynew, int64_t Nnew, int32_t gh_T,
                      double* cdf /* [Nnew] or NULL */, double* sf /* [Nnew] or NULL */);
int hmogp_predict_quantile(hmogp_handle h, int32_t t, const double* Xnew, int64_t Nnew, int32_t nP, const double* p /* [nP] */,
                           int32_t gh_T, double* q /* [Nnew, nP] */);

/* The JOINT posterior at new inputs: the Gaussian over f = (f_{d_1}(x_1..x_N), ..., f_{d_nD}(x_1..x_N)), function-major,
 * n = nD * Nnew, for nD distinct function indices d_index[j] in 0 .. Df-1, from the parameters of the last evaluation and in its
 * mode (default: through the explicit C_q; strict: through solves against Luu), small or regular model:
 *   mean[j, i]            = hmogp_predict_f's m[i, d_j]
 *   cov[(j, i), (j', i')] = sum_q (W_q[d_j] W_q[d_j'] + kappa_q[d_j] [j == j']) k_q(x_i, x_i') + W_q[d_j] W_q[d_j'] G_q[i, i'],
 *   G_q = A_q C_q A_q^T,  A_q = k_q(Xnew, Z_q),  C_q = Kuu^-1 S_q Kuu^-1 - Kuu^-1
 * cov [n, n] is written exactly symmetric (lower tiles computed, mirrored bit for bit); its diagonal is hmogp_predict_f's v before
 * any abs.  k_q(x_i, x_i') takes GPy's rounding order, so its diagonal is exactly the variance.
 * hmogp_sample_f_joint: F[s] = mean + L z_s for s < S, L the lower Cholesky factor of cov + jitter I on the ladder of
 * hmogp_jitchol_inv (first try without jitter: *rung_out = -1 and *jitter_out = 0; else rung k = 0 .. 4 and jitter = mean(diag cov)
 * 1e-6 10^k; HMOGP_E_NOT_PD beyond), z_s[i] = z0 of the counter-based normal generator at (seed, row i, sample s, pair 0) -- so
 * draw s does not depend on S.  F is [S, n]; mean [n], L [n, n] (dense, zeros above the diagonal), jitter_out, rung_out may be NULL.
 * HMOGP_E_STATE before the first evaluation; HMOGP_E_INVALID for nD < 1, an index out of range or repeated, n >
 * HMOGP_JOINT_MAXDIM, S < 1, or a NULL required pointer with Nnew > 0 -- every refusal before anything is launched.  Nnew = 0
 * returns at once.  New symbols only: ABI version 8 stays.                                                                       */
#define HMOGP_JOINT_MAXDIM 8192
int hmogp_predict_f_joint(hmogp_handle h, const double* Xnew, int64_t Nnew, int32_t nD, const int32_t* d_index /* [nD] */,
                          double* mean /* [nD, Nnew] */, double* cov /* [nD Nnew, nD Nnew] */);
int hmogp_sample_f_joint(hmogp_handle h, const double* Xnew, int64_t Nnew, int32_t nD, const int32_t* d_index /* [nD] */, int32_t S,
                         uint64_t seed, double* F /* [S, nD, Nnew] */, double* mean /* [nD, Nnew] or NULL */,
                         double* L /* [n, n] or NULL */, double* jitter_out /* or NULL */, int32_t* rung_out /* or NULL */);

/* Inducing inputs chosen from the data by greedy conditional variance = pivoted incomplete Cholesky of K_ff (Burt,
 * Rasmussen & van der Wilk 2020).  Stateless: no engine handle.  X [N, P] are the pooled rows, 1 <= P <= 4; the kernel of the
 * selection is k = sum_q variance[q] exp(-r_q^2 / 2) over the Q <= 8 RBF kernels (one Z serves all latents): r_q^2 in GPy's rounding
 * order with no contraction (what K_uu is built with), the sum over q from left to right, k0 = sum_q variance[q] summed the same way.
 *   d_i = k0 for all rows; then for j = 0 .. Mmax-1:
 *   1. p_j = forced[j] for j < n_forced, else the row with the largest d_i, ties to the SMALLEST index (so the first free pick is row 0);
 *   2. stop with *Mout = j if d_{p_j} <= max(tol, HMOGP_ZSEL_FLOOR) k0 -- forced picks too (below the floor d is rounding noise, and
 *      dividing by its root would fill a column with garbage);
 *   3. c_i = (k(x_i, x_{p_j}) - sum_{l<j} L_il L_{p_j l}) / sqrt(d_{p_j}), the sum ONE chain over l = 0, 1, .., j-1 per row (a row's
 *      result does not depend on the other rows or the grid);  L_ij = c_i,  d_i = max(d_i - c_i^2, 0),  d_{p_j} = 0 explicitly.
 * Out: *Mout; pivots[0 .. Mout); Z [Mout, P] = the pivots' rows; dpiv[j] = d_{p_j} at the time of the pick (its square root is the
 * Cholesky diagonal of K_uu in pick order); trace[0 .. Mout] = sum_i d_i before pick j, trace[Mout] the value after the last pick
 * (= tr(K_ff - Q_ff)); optionally L [N, Mmax] (columns at Mout and beyond are zero) and the final d [N].  The arrays are sized by Mmax
 * (pivots, dpiv [Mmax]; Z [Mmax, P]; trace [Mmax + 1]); entries beyond Mout come back as -1 (pivots) or 0.
 * HMOGP_E_INVALID, with a message that names the argument and before the device is touched, for N < 1, P outside 1..4, Q outside 1..8,
 * Mmax < 1, a non-finite entry of X, a variance or lengthscale that is not finite and > 0, tol negative or NaN, n_forced outside
 * 0..Mmax, a forced index out of range or repeated, or a NULL pointer (forced with n_forced = 0, L and d excepted).  Then
 * HMOGP_E_NO_DEVICE without a device, and HMOGP_E_INVALID (the message gives the bytes needed) if the factor's 8 N Mmax bytes plus the
 * row arrays exceed the device's free memory -- asked before any allocation.  New symbol only: ABI version 8 stays.                  */
#define HMOGP_ZSEL_FLOOR 9.094947017729282e-13 /* 2^-40 */
int hmogp_select_inducing(int32_t device, int64_t N, int32_t P, const double* X /* [N, P] */, int32_t Q, const double* variance /* [Q] */,
                          const double* lengthscale /* [Q] */, int32_t Mmax, double tol, int32_t n_forced,
                          const int64_t* forced /* [n_forced] or NULL */, int64_t* pivots /* [Mmax] */, double* Z /* [Mmax, P] */,
                          double* dpiv /* [Mmax] */, double* trace /* [Mmax + 1] */, double* L /* [N, Mmax] or NULL */,
                          double* d /* [N] or NULL */, int32_t* Mout);

/* Gradients of q(f) with respect to the new inputs (GPy's `predictive_gradients` at the level of the latent functions).
 * hmogp_predict_f forms, for row x, latent q and function d,
 *   k_qm(x) = variance_q exp(-r_qm^2 / 2 l_q^2),  p_q = sum_m a_qm k_qm,  c_q = sum_mm' k_qm C_q,mm' k_qm',
 *   m_d = sum_q W_qd p_q,  v_d = sum_q (W_qd^2 + kappa_qd) variance_q + W_qd^2 c_q
 * with a_q = Kuu^-1 m_q (hmogp_posterior_u's woodbury_vector) and C_q = Kuu^-1 S_q Kuu^-1 - Kuu^-1 (the NEGATIVE of its woodbury_inv).
 * The prior term of v_d is constant in x (the kernel is stationary), so with t_q = one row of A_q C_q, A_q = k_q(X, Z_q):
 *   gp_qj = (1 / l_q^2) sum_m a_qm k_qm (z_qmj - x_j),   gc_qj = (2 / l_q^2) sum_m t_qm k_qm (z_qmj - x_j),
 *   dm[i, d, j] = d m_d / d x_j = sum_q W_qd gp_qj,      dv[i, d, j] = d v_d / d x_j = sum_q W_qd^2 gc_qj.
 * v is the SIGNED value hmogp_predict_f returns: the gradient is that of v before any abs a caller takes.  (z - x) is one subtraction
 * per term; k_qm is the image the mean is formed with (written by the K_uf kernel in the named rounding variant and read back); a row's
 * result depends on that row's own inputs alone -- not on N, the row's position, or any chunking: the same row gives the same bits.
 * hmogp_qf_input_grad is the building block: any a [Q, M] and any C [Q, M, M] (t_q = k_q^T C_q: C_q,m'm weights k_qm'), `exact` the
 * rounding variant of hmogp_rbf_cross_cov_ex, Z laid out as in hmogp_params ([M, Q P]: latent q's inputs in columns q P .. q P + P).
 * HMOGP_E_INVALID, with a message that names the argument and before the device is touched, for N < 0, P outside 1..4, M, Q or Df below 1,
 * Q above 8, a required pointer NULL with N > 0, a variance or lengthscale that is not finite and > 0; then HMOGP_E_NO_DEVICE without a
 * device.  N = 0 returns success at once.
 * hmogp_predict_f_grad is the engine path, from the parameters of the last evaluation and in ITS mode (default: T = A C_q with the explicit
 * C_q; strict: T = ((A Kuu^-1) L_q L_q^T - A) Kuu^-1 through row solves against Luu, C_q never read), small or regular model, in the chunks
 * of hmogp_predict_f.  m and v (each may be NULL) are hmogp_predict_f's own values, bit for bit.  HMOGP_E_INVALID for a NULL handle,
 * Nnew < 0, or Xnew, dm or dv NULL with Nnew > 0; HMOGP_E_STATE before the first evaluation; Nnew = 0 returns success at once.
 * New symbols only: ABI version 8 stays.                                                                                              */
int hmogp_qf_input_grad(int32_t device, int64_t N, int32_t P, const double* X /* [N, P] */, int32_t M, int32_t Q,
                        const double* Z /* [M, Q*P], as hmogp_params */, const double* variance /* [Q] */,
                        const double* lengthscale /* [Q] */, int32_t exact /* the rbf rounding variant, as hmogp_rbf_cross_cov_ex */,
                        const double* a /* [Q, M] */, const double* C /* [Q, M, M] */, int32_t Df, const double* W /* [Q, Df] */,
                        double* dm /* [N, Df, P] */, double* dv /* [N, Df, P] */);
int hmogp_predict_f_grad(hmogp_handle h, const double* Xnew, int64_t Nnew, double* m /* [Nnew, Df] or NULL */,
                         double* v /* [Nnew, Df] or NULL */, double* dm /* [Nnew, Df, P] */, double* dv /* [Nnew, Df, P] */);

/* Posterior sample paths as FUNCTIONS: pathwise (Matheron) conditioning (Wilson, Borovitskiy, Terenin, Mostowsky & Deisenroth,
 * ICML 2020).  A path set = (nD distinct functions d_index[j], S samples, Lf random Fourier frequencies per latent, a 64-bit seed) is drawn
 * ONCE from the parameters of the last evaluation -- q(u_q) = N(m_q, L_q L_q^T), K_q = k_q(Z_q, Z_q) -- and can then be
 * evaluated at any inputs, any number of times: the same function on every call, O(N (Lf + M)) per sample, no bound on N.
 *   draws (z0 of the counter-based normal generator at (seed, n, s, pair); the pair is the stream tag):
 *     zeta_{q,l,p}    n = l,             s = 4 q + p,   pair 1      frequencies, shared by all samples: omega_{q,l,p} = zeta / (pi l_q)
 *     theta_{q,s}[k]  n = k < 2 Lf,      s = s Q + q,   pair 2      prior weights
 *     eps_{q,s}[m]    n = m < M,         s = s Q + q,   pair 3      q(u) normals
 *     theta'_{d,q,s}  n = d 2 Lf + k,    s = s Q + q,   pair 4      weights of the kappa part of FUNCTION d (its index, not its position)
 *   features: t_l(x) = sum_p omega_{q,l,p} x_p (in p order), c_q = sqrt(variance_q / Lf), phi_{q,l} = c_q cos(pi t_l), phi_{q,Lf+l} = c_q sin(pi t_l)
 *   (sincospi: exact argument reduction); E[phi_q(x)^T phi_q(x')] = k_q(x, x').  The STORED omega is the contract.
 *   paths:  u_{q,s} = m_q + L_q eps_{q,s},   v_{q,s} = K_q^-1 (u_{q,s} - Phi_q(Z_q) theta_{q,s})   (row solves against the set's own factor, below),
 *     f_d^s(x) = sum_q [ phi_q(x)^T (W_q[d] theta_{q,s} + sqrt(kappa_q[d]) theta'_{d,q,s}) + W_q[d] k_q(x, Z_q)^T v_{q,s} ]
 * Given the frequencies the S paths are i.i.d. Gaussian with hmogp_predict_f's mean exactly and hmogp_predict_f_joint's covariance with k_q
 * replaced by phi_q^T phi_q; at the inducing inputs the update cancels the feature error identically.  A function's paths depend neither on
 * S nor on which other functions were asked for; a row's value does not depend on Nnew or on the chunks; the set has one set of bits
 * whatever mode the evaluation ran in.  For that the set does NOT read the factor the evaluation left behind (the small-model kernel's
 * and the blocked factorisation's differ in their last bits): it forms K_q from its own copy of Z in GPy's rounding order and factorises
 * it with the blocked kernels of hmogp_jitchol_inv on the jitter rung the evaluation took -- compare v against that, not against a Luu
 * obtained elsewhere.  A set is a SNAPSHOT (its own copies of Z, omega, c_q, the weights, l_q, variance_q): later
 * evaluations, q(u) updates and hmogp_set_lik_params do not change it; hmogp_destroy frees every live set.
 * hmogp_paths_create: *id = the slot of the new set.  hmogp_paths_eval: F [S, nD, Nnew], the layout of hmogp_sample_f_joint.
 * hmogp_paths_state (each pointer may be NULL): omega [Q, Lf, P]; theta [Q, 2 Lf, S, nD] = W theta + sqrt(kappa) theta'; v [Q, M, S, nD] = W v;
 * u [Q, S, M].  hmogp_paths_free releases the slot.
 * HMOGP_E_INVALID for a NULL handle; then HMOGP_E_STATE before the first evaluation; HMOGP_E_INVALID for nD < 1, an index out of range or
 * repeated, S < 1, Lf < 1, Lf > HMOGP_PATHS_MAXFEAT, nD S > HMOGP_PATHS_MAXCOLS, no free slot (HMOGP_PATHS_MAXSETS live sets), a NULL id, an
 * unknown or freed id, Nnew < 0, Xnew or F NULL with Nnew > 0 -- every refusal before any device call; then HMOGP_E_INVALID, with the bytes
 * needed in the message, if the set's state and the draw's workspace exceed the device's free memory (asked before anything is
 * allocated).  Nnew = 0 returns success at once.  New symbols only: ABI version 8 stays.                                             */
#define HMOGP_PATHS_MAXFEAT 8192     /* Lf */
#define HMOGP_PATHS_MAXCOLS 4096     /* nD * S */
#define HMOGP_PATHS_MAXSETS 16       /* live path sets per engine */
int hmogp_paths_create(hmogp_handle h, int32_t nD, const int32_t* d_index /* [nD] */, int32_t S, int32_t Lf, uint64_t seed, int32_t* id);
int hmogp_paths_eval(hmogp_handle h, int32_t id, const double* Xnew /* [Nnew, P] */, int64_t Nnew, double* F /* [S, nD, Nnew] */);
int hmogp_paths_state(hmogp_handle h, int32_t id, double* omega /* [Q, Lf, P] */, double* theta /* [Q, 2Lf, S, nD] */,
                      double* v /* [Q, M, S, nD] */, double* u /* [Q, S, M] */);   /* each may be NULL */
int hmogp_paths_free(hmogp_handle h, int32_t id);
/* Gradients of the paths with respect to the new inputs: G [S, nD, Nnew, P], G[s, j, i, p] = d f_{d_j}^s / d x_p at row i of Xnew,
 * the exact derivative of the function hmogp_paths_eval evaluates (both parts of a path are linear in the set's state):
 *   d/dx_p phi_q(x)^T Theta~_q = phi_q(x)^T Theta~(p)_q,  Theta~(p)_q[l] = (pi omega_{q,l,p}) Theta~_q[Lf + l],  Theta~(p)_q[Lf + l] = -(pi omega_{q,l,p}) Theta~_q[l]
 *   d/dx_p k_q(x, z_m) = k_q(x, z_m) ((z_{q,m,p} - x_p) (1 / (l_q l_q)))          ((z - x): one subtraction per term)
 * summed over q from left to right.  F (optional): [S, nD, Nnew], the bits of hmogp_paths_eval.  Theta~(p) (P times the bytes of theta) is
 * built at the set's first gradient call and kept with the set; a set that is never differentiated pays nothing.  A row's bits depend on
 * neither Nnew nor the chunks nor S nor the other functions nor whether F is given, and are the same after a default-mode and a
 * strict-mode evaluation.  Given the frequencies the mean of G over the samples is d m_d / d x of hmogp_predict_f_grad.
 * HMOGP_E_INVALID for a NULL handle; HMOGP_E_STATE before the first evaluation; HMOGP_E_INVALID for an unknown or freed id, Nnew < 0, Xnew or G
 * NULL with Nnew > 0 -- every refusal before any device call; then HMOGP_E_INVALID, with the bytes in the message, if Theta~(p) and the
 * growth of the chunk workspace exceed the device's free memory.  Nnew = 0 returns success at once.  New symbol only: ABI version 8 stays. */
int hmogp_paths_eval_grad(hmogp_handle h, int32_t id, const double* Xnew /* [Nnew, P] */, int64_t Nnew,
                          double* F /* [S, nD, Nnew] or NULL */, double* G /* [S, nD, Nnew, P] */);

/* Data generation on the device: one draw Y[n] ~ p(y | F[n, :]) per row with the link functions and clips of the
 * reference's `<likelihood>.samples` (het_likelihood.py:72-83 -> e.g. gamma.py:43-50, categorical.py:65-75; labels of
 * Categorical are 1..K).  Counter-based generator keyed by (seed, row): reproducible, but a different stream than
 * NumPy's -- only the distribution is comparable with the reference.  Y is [N]; Dirichlet writes [N, K] (K Gamma(alpha_k, 1)
 * variates, normalised).                                                                                        */
int hmogp_sample(int32_t device, int32_t lik_id, double lik_param, int64_t N, uint64_t seed, const double* F /* [N, dim_f] */,
                 double* Y /* [N] */);

/* Micro-benchmark of the two row-pass contractions on synthetic operands resident in HBM (tools/bench_gemm.py):
 * role 1: forward  P~[n,M] = K^[n,M] C[M,M];  role 2: weighted Gram  H[M,M] (lower tiles) = K^T diag(beta) K^ incl. the
 * slab reduction; roles 3 / 4: role 1 with the fused row-statistics epilogue, with / without the P~ store; role 5: K_uf
 * construction alone (rbf_kernel<1, false>, 3 latents batched: 3 * 8 * n * M bytes written per launch); role 6
 * (diagnostic): role 2 over ALL tiles instead of the lower ones, same kernel, no slab reduction (2 n M^2 flops).
 * Returns the average milliseconds per launch over `iters` launches (HIP events).                              */
int hmogp_bench_contraction(int32_t device, int32_t role, int64_t n, int32_t M, int32_t iters, double* avg_ms);

/* Page-locked host memory (hipHostMalloc / hipHostFree).  Optional: parameter and gradient arrays that live in such
 * memory are transferred by DMA without the driver's staging copy (the 12.6 MB L_flat / g_L_u at M = 1024, Q = 3 cost
 * about 1 ms per evaluation from pageable memory).  Returns NULL without a HIP device or on failure.  No reference
 * equivalent.                                                                                                       */
void* hmogp_host_alloc(uint64_t bytes);
void hmogp_host_free(void* p);

#ifdef __cplusplus
}
#endif
#endif /* HETMOGP_HIP_H */
