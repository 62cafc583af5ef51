// lik_launch.h -- the likelihood families as the host sees them: the compile-time facts host code and kernels share, the Ordinal table,
// and the launchers of the per-family building blocks (lik_blocks.hip, logpred.hip, predq.hip).  The row pass's own launchers: rowpass.h.
#pragma once
#include "common.h"
#include "../../include/hetmogp_hip.h"

// lanes per row of a likelihood's predictive rule
__host__ __device__ constexpr int lik_pred_lanes(int lik) {
  return (lik == HMOGP_LIK_BETA || lik == HMOGP_LIK_GAMMA || lik == HMOGP_LIK_CATEGORICAL || lik == HMOGP_LIK_DIRICHLET) ? 64 : 1;
}

// lanes per row of a likelihood
__host__ __device__ constexpr int lik_lanes(int lik) {
  return (lik == HMOGP_LIK_BETA || lik == HMOGP_LIK_CATEGORICAL || lik == HMOGP_LIK_STUDENT || lik == HMOGP_LIK_DIRICHLET ||
          lik == HMOGP_LIK_NEGBINOMIAL || lik == HMOGP_LIK_WEIBULL || lik == HMOGP_LIK_BETABINOMIAL || lik == HMOGP_LIK_ZIPOISSON)
             ? 64
             : 1;
}

// Binomial, Beta-Binomial: the row carries its own trial count
__host__ __device__ constexpr bool lik_has_trials(int lik) { return lik == HMOGP_LIK_BINOMIAL || lik == HMOGP_LIK_BETABINOMIAL; }
// the count families whose yaux is gammaln(y + 1) (poisson.py:33)
__host__ __device__ constexpr bool lik_yaux_gammaln(int lik) {
  return lik == HMOGP_LIK_POISSON || lik == HMOGP_LIK_NEGBINOMIAL || lik == HMOGP_LIK_ZIPOISSON;
}
// the tensor rules over every function of the row, which exist with 10 nodes per dimension only
__host__ __device__ constexpr bool lik_tensor10(int lik) { return lik == HMOGP_LIK_CATEGORICAL || lik == HMOGP_LIK_DIRICHLET; }

// One registered Ordinal likelihood (hmogp_ordinal_table): K classes, K - 1 cut points, noise scale.  Small enough to
// travel to the predictive / sampling kernels by value.
struct OrdinalTable {
  int K = 0;
  double sigma = 0.0;
  double edge[HMOGP_ORDINAL_MAXK - 1];
};
// the table behind an Ordinal task's lik_param (lik_host.hip; throws HMOGP_E_INVALID for an id that was never handed out)
const OrdinalTable& ordinal_table(double lik_param);

// Ordinal: `param` is the table id in all four building blocks below, and `y` of launch_var_exp / launch_log_predictive is [2][N]:
// the rows' lower cut points, then their upper ones (ordinal_row_cuts).  Dirichlet: `param` is K, `y` is [K][N]: log y_k (dirichlet_log_rows),
// launch_predictive writes [N][K] moments and launch_sample [N][K] compositions
void launch_var_exp(int lik, int J, double param, long long N, const double* y, const double* m, const double* v, double* ve,
                    double* dm, double* dv, hipStream_t s, unsigned quirks = 0x1fu);
// predictive mean / variance of y: m, v [N][J] -> mean, var [N][Jp]; T = Gauss-Hermite order (10 or 20)
void launch_predictive(int lik, int J, int Jp, double param, int T, long long N, const double* m, const double* v,
                       double* mean, double* var, hipStream_t s);
// out[n] = -log S + logsumexp_s log p(y_n | f_s), f_s ~ N(m_n, diag v_n): Monte-Carlo log predictive density per row
void launch_log_predictive(int lik, int J, double param, long long N, int S, unsigned long long seed, const double* y,
                           const double* m, const double* v, double* out, hipStream_t s);
// Y[n] ~ p(y | F[n]): the reference's `<likelihood>.samples`, one draw per row, counter-based generator
void launch_sample(int lik, int J, double param, long long N, unsigned long long seed, const double* F, double* Y,
                   hipStream_t s);
void launch_gammaln1p(const double* y, double* out, long long N, hipStream_t s);
// Deterministic log predictive density per row (logpred.hip): lpd[n] = log of the Gauss-Hermite tensor rule of p(y_n | f)
// under q(f) = N(m_n, diag v_n), ess[n] = the rule's effective number of nodes (nullptr: not wanted).  `y` is the image the other
// building blocks read ([N]; Ordinal [2][ldy] cut points; Weibull [2][ldy]; Dirichlet [K][ldy]); m, v: row n starts at m[n * ldf], so
// that a task's columns of the engine's [N][Df] q(f) arrays are read in place.  `param`: sigma (Gaussian, Ordinal -- not the table
// id), nu (Student), K (Categorical, Dirichlet).  T: 10 or 20 nodes per dimension (Categorical, Dirichlet: 10).
struct LpdArgs {
  int lik = 0, J = 1, T = 20;
  double param = 0.0;
  long long N = 0;
  const double* y = nullptr;
  long long ldy = 0;
  const double *m = nullptr, *v = nullptr;
  int ldf = 1;
  bool absv = false;               // take |v| (the engine's q(f) variance, as the facade does)
  double *lpd = nullptr, *ess = nullptr;
};
void launch_log_predictive_gh(const LpdArgs& a, hipStream_t s);
// Predictive cdf / survival function / quantiles per row (predq.hip) over the same nodes and weights, for Gaussian,
// HetGaussian, Bernoulli, Exponential, Ordinal and Weibull; m, v, ldf, absv as in LpdArgs.  `y` (cdf only): [N]; Ordinal [2][ldy] cut
// points (the upper one is read); Weibull [N] log of the time, -inf for a time <= 0.  `param`: sigma (Gaussian, Ordinal -- not the
// table id).  `table`: the Ordinal table (quantiles only).  cdf / sf: [N], either may be null.  q: [N][nP], p: nP <= HMOGP_QUANT_MAXP
// probabilities (one outside (0, 1): NaN in its column).  T: 10 or 20.
struct PqArgs {
  int lik = 0, T = 20;
  double param = 0.0;
  const OrdinalTable* table = nullptr;
  long long N = 0;
  const double* y = nullptr;
  long long ldy = 0;
  const double *m = nullptr, *v = nullptr;
  int ldf = 1;
  bool absv = false;
  double *cdf = nullptr, *sf = nullptr;
  int nP = 0;
  double p[HMOGP_QUANT_MAXP] = {};
  double* q = nullptr;
};
const char* predq_refusal(int lik);   // nullptr for the six families, else the reason the family is refused
void launch_predictive_cdf(const PqArgs& a, hipStream_t s);
void launch_predictive_quantile(const PqArgs& a, hipStream_t s);
