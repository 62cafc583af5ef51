// lik_blocks.hip -- the per-family building blocks outside the engine's row pass (gfx950): stand-alone variational expectations,
// predictive moments, the Monte-Carlo log predictive density, data generation, with the Ordinal and Dirichlet kernels of their own,
// and gammaln(y + 1).  One family visitor (lik_dispatch.h) picks the instantiation in every launcher.  Declarations: lik_launch.h.
#include "lik_launch.h"
#include "lik_device.h"
#include "lik_dispatch.h"

namespace {

__global__ void gammaln1p_kernel(const double* __restrict__ y, double* __restrict__ out, long long N) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < N) out[i] = lgamma(y[i] + 1.0);
}

// ---- stand-alone variational expectations (hmogp_var_exp; also the predictive building block) -------------------
template <int LIK, int CATD = 0>
__global__ __launch_bounds__(256) void var_exp_kernel(int J, double param, long long N, const double* __restrict__ y,
                                                      const double* __restrict__ m, const double* __restrict__ v,
                                                      double* __restrict__ ve, double* __restrict__ dm,
                                                      double* __restrict__ dv, unsigned quirks) {
  constexpr int G = lik_lanes(LIK);
  __shared__ double etab[4][HMOGP_ETAB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long n = ((long long)blockIdx.x * 256 + t) / G;
  if (n >= N) return;
  double mu[HMOGP_MAXJ], vv[HMOGP_MAXJ];
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) {
    mu[j] = (j < J) ? m[n * J + j] : 0.0;
    vv[j] = (j < J) ? v[n * J + j] : 0.0;
  }
  LikOut o;
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) o.gm[j] = o.gv[j] = 0.0;
  const double yy = y[n];
  const double yaux = lik_yaux_gammaln(LIK)
                          ? lgamma(yy + 1.0)
                          : ((LIK == HMOGP_LIK_ORDINAL || LIK == HMOGP_LIK_WEIBULL) ? y[N + n] : (lik_has_trials(LIK) ? y[2 * N + n] : 0.0));  // Ordinal, Weibull: y is [2][N]
  if constexpr (lik_has_trials(LIK)) param = y[N + n];   // Binomial, Beta-Binomial: y is [3][N] = (k, n, lc); the row's own n, not n*
  if constexpr (LIK == HMOGP_LIK_DIRICHLET) {  // y is [K][N]: log y_k (CATD = K)
    double ly[CATD > 0 ? CATD : 1];
#pragma unroll
    for (int k = 0; k < CATD; ++k) ly[k] = y[k * N + n];
    lik_dirichlet_wave<CATD>(ly, mu, vv, lane, etab[w], o);
  } else {
    lik_eval<LIK, CATD>(yy, yaux, mu, vv, param, lane, etab[w], quirks, o);
  }
  if (G == 1 || lane == 0) {
    ve[n] = o.ve;
#pragma unroll
    for (int j = 0; j < HMOGP_MAXJ; ++j)
      if (j < J) {
        dm[n * J + j] = o.gm[j];
        dv[n * J + j] = o.gv[j];
      }
  }
}

// ---- predictive moments of y (hmogp_predictive) ------------------------------------------------------------------
template <int LIK>
__global__ __launch_bounds__(256) void predictive_kernel(int J, int Jp, double param, int T, long long N,
                                                         const double* __restrict__ m, const double* __restrict__ v,
                                                         double* __restrict__ mean, double* __restrict__ var) {
  constexpr int G = lik_pred_lanes(LIK);
  __shared__ double etab[4][HMOGP_ETAB];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long n = ((long long)blockIdx.x * 256 + t) / G;
  if (n >= N) return;
  double mu[HMOGP_MAXJ], vv[HMOGP_MAXJ], om[HMOGP_MAXJ], ov[HMOGP_MAXJ];
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) {
    mu[j] = (j < J) ? m[n * J + j] : 0.0;
    vv[j] = (j < J) ? v[n * J + j] : 0.0;
    om[j] = ov[j] = 0.0;
  }
  lik_predictive<LIK>(mu, vv, param, T, lane, etab[w], om, ov);
  if (G == 1 || lane == 0)
    for (int j = 0; j < Jp; ++j) {
      mean[n * Jp + j] = om[j];
      var[n * Jp + j] = ov[j];
    }
}

// ---- Monte-Carlo log predictive density: one wave per test row, samples strided over the lanes ------------------------
//   out[n] = -log(S) + logsumexp_s log p(y_n | f_s),  f_s ~ N(m_n, diag v_n)       (e.g. bernoulli.py:130-144)
template <int LIK>
__global__ __launch_bounds__(256) void log_predictive_kernel(int J, double param, long long N, int S, unsigned long long seed,
                                                             const double* __restrict__ y, const double* __restrict__ m,
                                                             const double* __restrict__ v, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double mu[HMOGP_MAXJ], sd[HMOGP_MAXJ];
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) {
    mu[j] = (j < J) ? m[n * J + j] : 0.0;
    sd[j] = (j < J) ? sqrt(v[n * J + j]) : 0.0;
  }
  const double yy = y[n], yaux = lik_yaux_gammaln(LIK)
                                     ? lgamma(yy + 1.0)
                                     : ((LIK == HMOGP_LIK_ORDINAL || LIK == HMOGP_LIK_WEIBULL) ? y[N + n] : (lik_has_trials(LIK) ? y[2 * N + n] : 0.0));
  if constexpr (lik_has_trials(LIK)) param = y[N + n];   // y is [3][N] = (k, n, lc)
  double mx = -INFINITY, se = 0.0;  // running max / sum of exp(l - max)
  for (int s = lane; s < S; s += 64) {
    double f[HMOGP_MAXJ];
#pragma unroll
    for (int j = 0; j < HMOGP_MAXJ; j += 2) {
      double z0 = 0.0, z1 = 0.0;
      if (j < J) normal_pair(seed, n, s, j >> 1, z0, z1);
      f[j] = mu[j] + sd[j] * z0;
      if (j + 1 < HMOGP_MAXJ) f[j + 1] = mu[j + 1] + sd[j + 1] * z1;
    }
    const double l = lik_logpdf_sample<LIK>(yy, yaux, f, param);
    if (l > mx) {
      se = se * exp(mx - l) + 1.0;
      mx = l;
    } else if (l != -INFINITY) {  // a sample with p = 0 contributes nothing (-inf - -inf would be NaN); a NaN l still reaches se
      se += exp(l - mx);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // combine (max, sumexp) pairs across the wave
    const double omx = __shfl_xor(mx, o, 64), ose = __shfl_xor(se, o, 64);
    const double nm = fmax(mx, omx);
    // the side that holds the new maximum keeps its sum as it is (-inf == -inf too: an empty lane keeps its 0, a NaN lane its NaN)
    se = (mx == nm ? se : se * exp(mx - nm)) + (omx == nm ? ose : ose * exp(omx - nm));
    mx = nm;
  }
  if (lane == 0) out[n] = -log((double)S) + mx + log(se);
}

// ---- data generation: one lane per row -------------------------------------------------------------------------------
template <int LIK>
__global__ __launch_bounds__(256) void sample_kernel(int J, double param, long long N, unsigned long long seed,
                                                     const double* __restrict__ F, double* __restrict__ Y) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double f[HMOGP_MAXJ];
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) f[j] = (j < J) ? F[n * J + j] : 0.0;
  RowRng g(seed, n);
  Y[n] = lik_sample<LIK>(g, f, param);
}

// ---- Ordinal: closed-form predictive moments and data generation, one lane per row, the table by value ---------
__global__ __launch_bounds__(256) void ordinal_predictive_kernel(OrdinalTable tb, long long N, const double* __restrict__ m,
                                                                 const double* __restrict__ v, double* __restrict__ mean,
                                                                 double* __restrict__ var) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double om, ov;
  lik_ordinal_predictive(tb, m[n], v[n], om, ov);
  mean[n] = om;
  var[n] = ov;
}

__global__ __launch_bounds__(256) void ordinal_sample_kernel(OrdinalTable tb, long long N, unsigned long long seed,
                                                             const double* __restrict__ F, double* __restrict__ Y) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  RowRng g(seed, n);
  Y[n] = lik_ordinal_sample(g, tb, F[n]);
}

// ---- Dirichlet: kernels of their own per K (the row carries K values where the generic kernels carry one) ---------
template <int K>
__global__ __launch_bounds__(256) void dirichlet_predictive_kernel(int T, long long N, const double* __restrict__ m,
                                                                   const double* __restrict__ v, double* __restrict__ mean,
                                                                   double* __restrict__ var) {
  __shared__ double etab[4][HMOGP_ETAB];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * 4 + w;
  if (n >= N) return;
  double mu[K], vv[K], om[K], ov[K];
#pragma unroll
  for (int k = 0; k < K; ++k) mu[k] = m[n * K + k], vv[k] = v[n * K + k];
  lik_dirichlet_predictive<K>(mu, vv, T, lane, etab[w], om, ov);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) mean[n * K + k] = om[k], var[n * K + k] = ov[k];
  }
}

// y: [K][N] log y_k; samples strided over the lanes as in log_predictive_kernel (same generator, same combination)
template <int K>
__global__ __launch_bounds__(256) void dirichlet_log_predictive_kernel(long long N, int S, unsigned long long seed,
                                                                       const double* __restrict__ y, const double* __restrict__ m,
                                                                       const double* __restrict__ v, double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double mu[4], sd[4], ly[K];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    mu[j] = (j < K) ? m[n * K + j] : 0.0;
    sd[j] = (j < K) ? sqrt(v[n * K + j]) : 0.0;
  }
#pragma unroll
  for (int k = 0; k < K; ++k) ly[k] = y[k * N + n];
  double mx = -INFINITY, se = 0.0;
  for (int s = lane; s < S; s += 64) {
    double f[4];
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
      double z0 = 0.0, z1 = 0.0;
      if (j < K) normal_pair(seed, n, s, j >> 1, z0, z1);
      f[j] = mu[j] + sd[j] * z0;
      f[j + 1] = mu[j + 1] + sd[j + 1] * z1;
    }
    const double l = lik_dirichlet_logpdf<K>(ly, f);
    if (l > mx) {
      se = se * exp(mx - l) + 1.0;
      mx = l;
    } else if (l != -INFINITY) {  // as in log_predictive_kernel
      se += exp(l - mx);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double omx = __shfl_xor(mx, o, 64), ose = __shfl_xor(se, o, 64);
    const double nm = fmax(mx, omx);
    // the side that holds the new maximum keeps its sum as it is (-inf == -inf too: an empty lane keeps its 0, a NaN lane its NaN)
    se = (mx == nm ? se : se * exp(mx - nm)) + (omx == nm ? ose : ose * exp(omx - nm));
    mx = nm;
  }
  if (lane == 0) out[n] = -log((double)S) + mx + log(se);
}

template <int K>
__global__ __launch_bounds__(256) void dirichlet_sample_kernel(long long N, unsigned long long seed, const double* __restrict__ F,
                                                               double* __restrict__ Y) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  double f[K], yv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) f[k] = F[n * K + k];
  RowRng g(seed, n);
  lik_dirichlet_sample<K>(g, f, yv);
#pragma unroll
  for (int k = 0; k < K; ++k) Y[n * K + k] = yv[k];
}

}  // namespace

// =============================================================================================== launchers
// (Dirichlet: J = K was checked by check_lik_param; visit_family refuses anything else as a caller's bug)
void launch_sample(int lik, int J, double param, long long N, unsigned long long seed, const double* F, double* Y,
                   hipStream_t s) {
  if (N <= 0) return;
  dim3 grid((unsigned)((N + 255) / 256));
  visit_family(lik, J, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK, D = decltype(fam)::D;
    if constexpr (L == HMOGP_LIK_ORDINAL)
      hipLaunchKernelGGL(ordinal_sample_kernel, grid, dim3(256), 0, s, ordinal_table(param), N, seed, F, Y);
    else if constexpr (L == HMOGP_LIK_DIRICHLET)
      hipLaunchKernelGGL((dirichlet_sample_kernel<D>), grid, dim3(256), 0, s, N, seed, F, Y);
    else
      hipLaunchKernelGGL((sample_kernel<L>), grid, dim3(256), 0, s, J, param, N, seed, F, Y);
  });
}

void launch_var_exp(int lik, int J, double param, long long N, const double* y, const double* m, const double* v, double* ve,
                    double* dm, double* dv, hipStream_t s, unsigned quirks) {
  if (N <= 0) return;
  dim3 grid((unsigned)((N * lik_lanes(lik) + 255) / 256));
  visit_family(lik, J, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK, D = decltype(fam)::D;
    if constexpr (L == HMOGP_LIK_ORDINAL) param = ordinal_table(param).sigma;
    hipLaunchKernelGGL((var_exp_kernel<L, D>), grid, dim3(256), 0, s, J, param, N, y, m, v, ve, dm, dv, quirks);
  });
}

void launch_predictive(int lik, int J, int Jp, double param, int T, long long N, const double* m, const double* v,
                       double* mean, double* var, hipStream_t s) {
  if (N <= 0) return;
  dim3 grid((unsigned)((N * lik_pred_lanes(lik) + 255) / 256));
  visit_family(lik, J, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK, D = decltype(fam)::D;
    if constexpr (L == HMOGP_LIK_ORDINAL)
      hipLaunchKernelGGL(ordinal_predictive_kernel, grid, dim3(256), 0, s, ordinal_table(param), N, m, v, mean, var);
    else if constexpr (L == HMOGP_LIK_DIRICHLET)   // (64 lanes per row: the grid above is one block per 4 rows)
      hipLaunchKernelGGL((dirichlet_predictive_kernel<D>), grid, dim3(256), 0, s, T, N, m, v, mean, var);
    else
      hipLaunchKernelGGL((predictive_kernel<L>), grid, dim3(256), 0, s, J, Jp, param, T, N, m, v, mean, var);
  });
}

void launch_log_predictive(int lik, int J, double param, long long N, int S, unsigned long long seed, const double* y,
                           const double* m, const double* v, double* out, hipStream_t s) {
  if (N <= 0) return;
  dim3 grid((unsigned)((N + 3) / 4));
  visit_family(lik, J, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK, D = decltype(fam)::D;
    if constexpr (L == HMOGP_LIK_GAMMA || L == HMOGP_LIK_BETA) {
      throw HipError{hipErrorInvalidValue, "the reference defines no log_predictive for this likelihood", __FILE__, __LINE__};
    } else if constexpr (L == HMOGP_LIK_DIRICHLET) {
      hipLaunchKernelGGL((dirichlet_log_predictive_kernel<D>), grid, dim3(256), 0, s, N, S, seed, y, m, v, out);
    } else {
      if constexpr (L == HMOGP_LIK_ORDINAL) param = ordinal_table(param).sigma;
      hipLaunchKernelGGL((log_predictive_kernel<L>), grid, dim3(256), 0, s, J, param, N, S, seed, y, m, v, out);
    }
  });
}

void launch_gammaln1p(const double* y, double* out, long long N, hipStream_t s) {
  if (N <= 0) return;
  hipLaunchKernelGGL(gammaln1p_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, y, out, N);
}
