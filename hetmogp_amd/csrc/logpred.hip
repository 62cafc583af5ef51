// logpred.hip -- deterministic per-row log predictive density: for a test row with q(f) = N(m, diag v),
//   lpd = log sum_nodes (prod_d w_{i_d}) p(y | f_node),   f_node,d = m_d + sqrt(2 v_d) x_{i_d},
// the Gauss-Hermite tensor rule with the normalised weights GH10_WN / GH20_WN once per dimension, and beside it the effective number of
// nodes ess = (sum e)^2 / sum e^2, e = (prod w) p.  log p(y|f) is what the Monte-Carlo kernel evaluates (lik_logpdf_sample,
// lik_dirichlet_logpdf; Gamma and Beta: lik_gamma_logpdf / lik_beta_logpdf).  Gaussian is the closed form log N(y; m, sigma^2 + v)
// (ess = +inf), HetGaussian integrates f0 analytically: T nodes over f1 of log N(y; m0, v0 + safe_exp(f1)).
// Two kernels, the split quad_kernel makes: rules of at most 20 nodes run one lane per row, the tensor rules one wave per row (four
// rows per block), nodes strided over the lanes.  Declarations: lik_launch.h.
#include "lik_launch.h"
#include "lik_device.h"
#include "lik_dispatch.h"

namespace {

// one node into a lane's running (max, sum e / exp(max), sum e^2 / exp(2 max)); a node with log p = -inf contributes nothing
__device__ __forceinline__ void lpd_add(double& mx, double& s1, double& s2, double w, double l) {
  if (l == -INFINITY) return;
  if (l > mx) {
    const double r = exp(mx - l);
    s1 = s1 * r + w;
    s2 = s2 * (r * r) + w * w;
    mx = l;
  } else {
    const double e = w * exp(l - mx);
    s1 += e;
    s2 += e * e;
  }
}
// every node -inf: lpd = -inf, ess = NaN
__device__ __forceinline__ void lpd_store(double mx, double s1, double s2, long long n, double* __restrict__ lpd,
                                          double* __restrict__ ess) {
  const bool none = mx == -INFINITY;
  lpd[n] = none ? -INFINITY : mx + log(s1);
  if (ess) ess[n] = none ? nan("") : (s1 * s1) / s2;
}

// ---- rules of at most 20 nodes: one lane per row, the node loop in registers ---------------------------------------------------
// y: [N], Ordinal [2][ldy] (lower, upper cut point), Binomial [3][ldy] (k, n, lc); m, v: row n at m[n * ldf] (the task's column of a wider q(f) array)
template <int LIK>
__global__ __launch_bounds__(256) void lpd_lane_kernel(double param, int T, long long N, const double* __restrict__ y, long long ldy,
                                                       const double* __restrict__ m, const double* __restrict__ v, int ldf, int absv,
                                                       double* __restrict__ lpd, double* __restrict__ ess) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double yy = y[n];
  const double m0 = m[n * ldf];
  double v0 = v[n * ldf];
  if (absv) v0 = fabs(v0);
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    const double s2 = param * param + v0, d = yy - m0;
    lpd[n] = -0.5 * log(2.0 * M_PI) - 0.5 * log(s2) - 0.5 * (d * d / s2);
    if (ess) ess[n] = INFINITY;
    return;
  }
  double mx = -INFINITY, s1 = 0.0, s2 = 0.0;
  if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    const double m1 = m[n * ldf + 1];
    double v1 = v[n * ldf + 1];
    if (absv) v1 = fabs(v1);
    const double s = sqrt(2.0 * v1), d2 = safe_square(yy - m0);
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const double var = v0 + safe_exp(gh_x(T, i) * s + m1);
      lpd_add(mx, s1, s2, gh_wn(T, i), -0.5 * log(2.0 * M_PI) - 0.5 * log(var) - 0.5 * (d2 / var));
    }
  } else {
    const double yaux = lik_yaux_gammaln(LIK) ? lgamma(yy + 1.0)
                                                 : (LIK == HMOGP_LIK_ORDINAL ? y[ldy + n] : (lik_has_trials(LIK) ? y[2 * ldy + n] : 0.0));
    if constexpr (lik_has_trials(LIK)) param = y[ldy + n];   // Binomial: y is [3][ldy] = (k, n, lc); the row's own n
    const double s = sqrt(2.0 * v0);
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const double f = gh_x(T, i) * s + m0;
      lpd_add(mx, s1, s2, gh_wn(T, i), lik_logpdf_sample<LIK>(yy, yaux, &f, param));
    }
  }
  lpd_store(mx, s1, s2, n, lpd, ess);
}

// ---- tensor rules: one wave per row, four rows per block ----------------------------------------------------------------------
// JD = the family's functions (a template parameter: the node's f lives in registers under static indices only).  The node values of
// dimension k go into the wave's own LDS slice at [20 k, 20 k + T), filled from global memory (a run-time k costs nothing there).
// y: [N]; Weibull [2][ldy] (log y, delta); Dirichlet [K][ldy] (log y_k); Beta-Binomial [3][ldy] (k, n, lc).
template <int LIK, int JD>
__global__ __launch_bounds__(256) void lpd_wave_kernel(double param, int T, long long N, const double* __restrict__ y, long long ldy,
                                                       const double* __restrict__ m, const double* __restrict__ v, int ldf, int absv,
                                                       double* __restrict__ lpd, double* __restrict__ ess) {
  static_assert(20 * JD <= HMOGP_ETAB, "node table");
  __shared__ double etab[4][HMOGP_ETAB];
  const int lane = threadIdx.x & 63, w4 = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * 4 + w4;
  if (n >= N) return;
  double* tab = etab[w4];
  for (int e = lane; e < JD * T; e += 64) {
    const int k = e / T, i = e - k * T;
    double vk = v[n * ldf + k];
    if (absv) vk = fabs(vk);
    tab[20 * k + i] = gh_x(T, i) * sqrt(2.0 * vk) + m[n * ldf + k];
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only
  const double yy = y[n];
  const double yaux = lik_yaux_gammaln(LIK) ? lgamma(yy + 1.0)
                                                   : (LIK == HMOGP_LIK_WEIBULL ? y[ldy + n] : (lik_has_trials(LIK) ? y[2 * ldy + n] : 0.0));
  if constexpr (lik_has_trials(LIK)) param = y[ldy + n];   // Beta-Binomial: y is [3][ldy] = (k, n, lc); the row's own n
  double ly[LIK == HMOGP_LIK_DIRICHLET ? JD : 1];
  if (LIK == HMOGP_LIK_DIRICHLET) {
#pragma unroll
    for (int k = 0; k < JD; ++k) ly[k] = y[k * ldy + n];
  } else {
    ly[0] = 0.0;
  }
  int total = 1;
#pragma unroll
  for (int k = 0; k < JD; ++k) total *= T;
  double mx = -INFINITY, s1 = 0.0, s2 = 0.0;
  for (int node = lane; node < total; node += 64) {
    double f[HMOGP_MAXJ], w = 1.0;
    int rem = node;
#pragma unroll
    for (int k = HMOGP_MAXJ - 1; k >= 0; --k) {
      if (k < JD) {
        const int i = rem % T;
        rem /= T;
        f[k] = tab[20 * k + i];
        w *= gh_wn(T, i);
      } else {
        f[k] = 0.0;
      }
    }
    double l;
    if constexpr (LIK == HMOGP_LIK_DIRICHLET) l = lik_dirichlet_logpdf<JD>(ly, f);
    else if constexpr (LIK == HMOGP_LIK_GAMMA) l = lik_gamma_logpdf(yy, f);
    else if constexpr (LIK == HMOGP_LIK_BETA) l = lik_beta_logpdf(yy, f);
    else l = lik_logpdf_sample<LIK>(yy, yaux, f, param);
    lpd_add(mx, s1, s2, w, l);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // combine the (max, sum, sum of squares) triples across the wave
    const double omx = __shfl_xor(mx, o, 64), o1 = __shfl_xor(s1, o, 64), o2 = __shfl_xor(s2, o, 64);
    const double nm = fmax(mx, omx);
    const double a = mx == -INFINITY ? 0.0 : exp(mx - nm), b = omx == -INFINITY ? 0.0 : exp(omx - nm);
    s1 = s1 * a + o1 * b;
    s2 = s2 * (a * a) + o2 * (b * b);
    mx = nm;
  }
  if (lane == 0) lpd_store(mx, s1, s2, n, lpd, ess);
}

}  // namespace

void launch_log_predictive_gh(const LpdArgs& a, hipStream_t s) {
  if (a.N <= 0) return;
  const dim3 glane((unsigned)((a.N + 255) / 256)), gwave((unsigned)((a.N + 3) / 4));
  if (lik_tensor10(a.lik) ? a.T != 10 : (a.T != 10 && a.T != 20))
    throw HipError{hipErrorInvalidValue, "log predictive density: nodes per dimension must be 10 or 20 (Categorical, Dirichlet: 10)", __FILE__, __LINE__};
  visit_family(a.lik, a.J, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK, D = decltype(fam)::D;
    // rules of at most 20 nodes: one lane per row; the tensor rules of the two-function families and of Categorical / Dirichlet: one wave
    constexpr bool lane = L == HMOGP_LIK_GAUSSIAN || L == HMOGP_LIK_BERNOULLI || L == HMOGP_LIK_POISSON || L == HMOGP_LIK_EXPONENTIAL ||
                          L == HMOGP_LIK_ORDINAL || L == HMOGP_LIK_BINOMIAL || L == HMOGP_LIK_HETGAUSSIAN;
    constexpr bool wave2 = L == HMOGP_LIK_GAMMA || L == HMOGP_LIK_BETA || L == HMOGP_LIK_STUDENT || L == HMOGP_LIK_NEGBINOMIAL ||
                           L == HMOGP_LIK_WEIBULL || L == HMOGP_LIK_BETABINOMIAL || L == HMOGP_LIK_ZIPOISSON;
    static_assert(lane || wave2 || lik_tensor10(L), "launch_log_predictive_gh: a family with neither a lane nor a wave rule");
    if constexpr (lane)
      hipLaunchKernelGGL((lpd_lane_kernel<L>), glane, dim3(256), 0, s, a.param, a.T, a.N, a.y, a.ldy, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.lpd, a.ess);
    else
      hipLaunchKernelGGL((lpd_wave_kernel<L, wave2 ? 2 : D>), gwave, dim3(256), 0, s, a.param, a.T, a.N, a.y, a.ldy, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.lpd, a.ess);
  });
}
