// lik_device.h -- device-side variational expectations E_q(f)[log p(y|f)] and their derivatives with respect to
// the mean / variance of q(f), for the eight likelihoods of /root/reference/likelihoods/*.py (SURVEY.md 8a, rows
// L1-L8), the heteroscedastic Student-t the reference only stubs (student.py; contract: DESIGN 9) and the Ordinal (ordered
// probit) likelihood it only stubs as well (ordinal.py; contract: DESIGN 9b; no clip), and the Dirichlet likelihood, its third stub
// (dirichlet.py; contract: DESIGN 9d; K log y_k per row), and the heteroscedastic Negative Binomial and the right-censored Weibull, which
// the reference does not have (contracts: DESIGN 9h, 9i).  Results reproduce the reference's formulas including its clips and quirks:
//   Q1  Gamma / Beta: Gauss-Hermite weights divided by sqrt(pi) twice (gamma.py:110,139-141; beta.py:113,142-144)
//   Q2  Categorical: d/dm is the constant onehot(y)[d] - 1 (categorical.py:102-113)
// At the end of the file: the derivatives with respect to the likelihoods' OWN parameters (Gaussian sigma, Student nu, Ordinal cut
// points and sigma), appended so that nothing above them changes; and, appended last, the Binomial and Beta-Binomial families
// with per-row trial counts (one lane per row and one wave per row), and after them the zero-inflated Poisson (one
// wave per row: 40 nodes where y >= 1, 400 where y = 0).
// Lane mapping: closed forms, 1-D quadratures and Gamma (separable in its two functions) use ONE lane per row;
// Beta (100 nodes), Student, Negative Binomial and Weibull (400 nodes), Categorical (10^(K-1) nodes) and Dirichlet (10^K nodes) use ONE WAVE per row,
// nodes strided over the 64 lanes and reduced with wavefront shuffles.
#pragma once
#include "common.h"
#include "gh_tables.h"
#include "../../include/hetmogp_hip.h"

#include "rowpass.h"     // HMOGP_MAXJ / HMOGP_MAXQ
#include "lik_launch.h"  // lik_lanes, lik_pred_lanes and the other compile-time family facts; OrdinalTable

#define LIM_VAL 709.782712893384      // log(DBL_MAX): GPy safe_exp clip
#define SQRT_DBL_MAX 1.3407807929942596e154  // GPy safe_square clip
#define INV_SQRT_PI 0.5641895835477563

struct LikOut {
  double ve;
  double gm[HMOGP_MAXJ];
  double gv[HMOGP_MAXJ];
};

// Binomial / Beta-Binomial: defined in the last section of this file, declared here for the dispatchers in between
__device__ __forceinline__ void lik_binomial_quad(double k, double n, double lc, double m, double v, LikOut& o);
__device__ __forceinline__ void lik_betabinomial_wave(double k, double n, double lc, const double* m, const double* v, int lane,
                                                      double* tab, LikOut& o);
__device__ __forceinline__ double lik_binomial_logpdf(double k, double n, double lc, const double* f);
__device__ __forceinline__ double lik_betabinomial_logpdf(double k, double n, double lc, const double* f);
__device__ __forceinline__ void lik_binomial_predictive(double m, double v, double param, int T, double& mean, double& var);
__device__ __forceinline__ void lik_betabinomial_predictive(const double* m, const double* v, double param, int T, double& mean,
                                                            double& var);

// Zero-inflated Poisson: defined after them, at the end of this file
__device__ __forceinline__ void lik_zipoisson_wave(double y, double lgy1, const double* m, const double* v, int lane, double* tab, LikOut& o);
__device__ __forceinline__ double lik_zipoisson_logpdf(double y, double lgy1, const double* f);
__device__ __forceinline__ void lik_zipoisson_predictive(const double* m, const double* v, int T, double& mean, double& var);

__device__ __forceinline__ double safe_exp(double f) { return exp(fmin(f, LIM_VAL)); }
__device__ __forceinline__ double safe_square(double f) {
  const double g = fmin(f, SQRT_DBL_MAX);
  return g * g;
}
__device__ __forceinline__ double clip(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// digamma for x > 0: upward recurrence to x >= 10, then the asymptotic series in Bernoulli numbers.
__device__ __forceinline__ double digamma_pos(double x) {
  double r = 0.0;
  while (x < 10.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double z = 1.0 / (x * x);
  const double y =
      z * (8.33333333333333333333e-2 +
           z * (-8.33333333333333333333e-3 +
                z * (3.96825396825396825397e-3 +
                     z * (-4.16666666666666666667e-3 +
                          z * (7.57575757575757575758e-3 + z * (-2.10927960927960927961e-2 + z * 8.33333333333333333333e-2))))));
  return log(x) - 0.5 / x - y + r;
}

// trigamma = Hurwitz zeta(2, x) for x > 0 (scipy.special.zeta(2, a) in gamma.py:98, beta.py:99-101).
__device__ __forceinline__ double trigamma_pos(double x) {
  double r = 0.0;
  while (x < 12.0) {
    r += 1.0 / (x * x);
    x += 1.0;
  }
  const double ix = 1.0 / x, z = ix * ix;
  const double s = 1.0 / 6.0 -
                   z * (1.0 / 30.0 -
                        z * (1.0 / 42.0 - z * (1.0 / 30.0 - z * (5.0 / 66.0 - z * (691.0 / 2730.0 - z * (7.0 / 6.0))))));
  return r + ix + 0.5 * z + ix * z * s;
}

// ------------------------------------------------------------------------------------------- closed forms
// gaussian.py:41-62
__device__ __forceinline__ void lik_gaussian(double y, double m, double v, double sigma, LikOut& o) {
  const double s2 = sigma * sigma;
  o.ve = -0.5 * log(2.0 * M_PI) - 0.5 * log(s2) - 0.5 * (y * y + m * m + v - 2.0 * m * y) / s2;
  o.gm[0] = -(m - y) / s2;
  o.gv[0] = -0.5 * (1.0 / s2);
}

// hetgaussian.py:46-73
__device__ __forceinline__ void lik_hetgaussian(double y, const double* m, const double* v, LikOut& o) {
  const double prec = clip(safe_exp(-m[1] + 0.5 * v[1]), -1e9, 1e9);
  const double sq = clip(safe_square(y) + safe_square(m[0]) + v[0] - 2.0 * m[0] * y, -1e9, 1e9);
  o.ve = -(0.5 * log(2.0 * M_PI)) - 0.5 * m[1] - 0.5 * prec * sq;
  o.gm[0] = prec * (y - m[0]);
  o.gm[1] = 0.5 * (prec * sq - 1.0);
  o.gv[0] = -0.5 * prec;
  o.gv[1] = -0.25 * prec * sq;
}

// ------------------------------------------------------------------------------------------- 1-D, T = 20
// bernoulli.py:31-36,66-111 ; poisson.py:31-34,56-95 ; exponential.py:28-32,58-99
template <int LIK>
__device__ __forceinline__ void lik_quad1d(double y, double yaux, double m, double v, LikOut& o) {
  const double s = sqrt(2.0 * v);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 4
  for (int i = 0; i < 20; ++i) {
    const double f = GH20_X[i] * s + m, w = GH20_WN[i];
    double lp, d1, d2;
    if (LIK == HMOGP_LIK_BERNOULLI) {
      const double ef = safe_exp(f);
      const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
      lp = y * log(p) + (1.0 - y) * log(1.0 - p);
      d1 = ((y - p) / (1.0 - p)) * (1.0 / (1.0 + ef));
      d2 = -p / (1.0 + ef);
    } else if (LIK == HMOGP_LIK_POISSON) {
      const double ef = safe_exp(f);
      lp = -ef + y * f - yaux;  // yaux = gammaln(y + 1)
      d1 = -ef + y;
      d2 = -ef;
    } else {  // exponential
      const double b = clip(safe_exp(-f), 1e-9, 1e9);
      lp = -log(b) - y / b;
      d1 = 1.0 - y / b;
      d2 = -y / b;
    }
    a0 += lp * w;
    a1 += d1 * w;
    a2 += d2 * w;
  }
  o.ve = a0;
  o.gm[0] = a1;
  o.gv[0] = 0.5 * a2;
}

// ------------------------------------------------------------------------------------------- Gamma, 10 x 10
// gamma.py:34-41,80-194.  a = exp(f1) depends only on node i, b = exp(f2) only on node j, and every term of
// logp / dlogp / d2logp is a product of a function of i and a function of j, so the 100-node tensor rule
// collapses to 10 + 10 evaluations.  Effective per-dimension weight w_i/pi (quirk Q1).
__device__ __forceinline__ void lik_gamma(double y, const double* m, const double* v, LikOut& o) {
  const double s1 = sqrt(2.0 * v[0]), s2 = sqrt(2.0 * v[1]);
  double S0 = 0.0, A1 = 0.0, Alg = 0.0, Apsi = 0.0, Azeta = 0.0, B1 = 0.0, Blog = 0.0;
  for (int i = 0; i < 10; ++i) {
    const double w = GH10_WN[i] * INV_SQRT_PI;
    const double a = clip(safe_exp(GH10_X[i] * s1 + m[0]), 1e-9, 1e9);
    const double b = clip(safe_exp(GH10_X[i] * s2 + m[1]), 1e-9, 1e9);
    S0 += w;
    A1 += w * a;
    Alg += w * lgamma(a);
    Apsi += w * digamma_pos(a) * a;
    Azeta += w * a * a * trigamma_pos(a);
    B1 += w * b;
    Blog += w * log(b);
  }
  const double ly = log(y);
  o.ve = -S0 * Alg + A1 * Blog + ly * S0 * (A1 - S0) - y * S0 * B1;
  const double common = A1 * Blog + ly * S0 * A1;
  o.gm[0] = -S0 * Apsi + common;
  o.gm[1] = S0 * A1 - y * S0 * B1;
  o.gv[0] = 0.5 * (-S0 * (Apsi + Azeta) + common);
  o.gv[1] = 0.5 * (-y * S0 * B1);
}

// ------------------------------------------------------------------------------------------- Ordinal (ordered probit), T = 20
// DESIGN 9b (the reference's ordinal.py is a constructor only).  One node of the rule: with a = (lo - f) / sigma < b = (hi - f) / sigma
// the row's own two cut points seen from f (one of them may be infinite), P = Phi(b) - Phi(a) and phi the normal density,
//   lp = log P,   g = (phi(a) - phi(b)) / P,   h = (a phi(a) - b phi(b)) / P       (terms with an infinite a or b are 0)
// without a clip and without ever forming a P that underflows:
//   * mirror (a, b) -> (-b, -a) when the bin lies on the upper side, so that |b| <= |a| and a < 0; g changes sign, lp and h do not;
//   * the bin straddles f (b > 0) and the two tails Q = Phi(a) + Phi(-b) hold less than half: lp = log1p(-Q), P = 1 - Q >= 1/2;
//   * otherwise, with E(x) = erfcx(-x / sqrt 2) and d = (a^2 - b^2) / 2 >= 0:  P = exp(-b^2 / 2) D / 2,  D = E(b) - exp(-d) E(a), so
//       lp = -b^2 / 2 + log(D / 2),   g = sqrt(2 / pi) expm1(-d) / D,   h = sqrt(2 / pi) (a exp(-d) - b) / D,
//     D being formed as (E(b) - E(a)) - expm1(-d) E(a), a sum of two positive numbers.
// An end bin costs one erfcx (E(-inf) = 0), a middle bin two.  What is left is the cancellation of a NARROW bin in E(b) - E(a),
// measured in DESIGN 9b.
#define ORD_INV_SQRT_2PI 0.3989422804014327
#define ORD_SQRT_2_OVER_PI 0.7978845608028654
__device__ __forceinline__ void ordinal_node(double a, double b, double& lp, double& g, double& h) {
  double sgn = 1.0;
  if (a + b > 0.0) {
    const double t = a;
    a = -b, b = -t, sgn = -1.0;
  }
  if (b > 0.0) {
    const double Q = 0.5 * (erfc(-a * M_SQRT1_2) + erfc(b * M_SQRT1_2));
    if (Q < 0.5) {
      const double rP = 1.0 / (1.0 - Q);
      const double pa = ORD_INV_SQRT_2PI * exp(-0.5 * a * a), pb = ORD_INV_SQRT_2PI * exp(-0.5 * b * b);
      lp = log1p(-Q);
      g = sgn * (pa - pb) * rP;
      h = ((isinf(a) ? 0.0 : a * pa) - (isinf(b) ? 0.0 : b * pb)) * rP;
      return;
    }
  }
  const double Ea = erfcx(-a * M_SQRT1_2), Eb = erfcx(-b * M_SQRT1_2);  // a = -inf: E = 0
  const double em = expm1(0.5 * (b - a) * (a + b));                      //           expm1(-inf) = -1
  const double D = (Eb - Ea) - em * Ea;
  const double rD = ORD_SQRT_2_OVER_PI / D;
  lp = -0.5 * b * b + log(0.5 * D);
  g = sgn * em * rD;
  h = ((isinf(a) ? 0.0 : a * (1.0 + em)) - b) * rD;
}

// 20-node rule, one lane per row: ve = sum w log p, dm = sum w dlog p/df, dv = 1/2 sum w d2log p/df2 with
// dlog p/df = g / sigma, d2log p/df2 = h / sigma^2 - (dlog p/df)^2.
__device__ __forceinline__ void lik_ordinal(double lo, double hi, double m, double v, double sigma, LikOut& o) {
  const double s = sqrt(2.0 * v), s2 = sigma * sigma;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 1
  for (int i = 0; i < 20; ++i) {
    const double f = GH20_X[i] * s + m, w = GH20_WN[i];
    double lp, g, h;
    ordinal_node((lo - f) / sigma, (hi - f) / sigma, lp, g, h);
    const double d1 = g / sigma;
    a0 += lp * w;
    a1 += d1 * w;
    a2 += (h / s2 - d1 * d1) * w;
  }
  o.ve = a0;
  o.gm[0] = a1;
  o.gv[0] = 0.5 * a2;
}

// closed-form moments of the label under q(f) = N(m, v): with z_k = (b_k - m) / sqrt(sigma^2 + v), P(y > k) = Phi(-z_k), so
// mean = 1 + sum_k Phi(-z_k) and E[y^2] = 1 + sum_k (2 k + 1) Phi(-z_k), k = 1 .. K - 1: sums of positive terms.
__device__ __forceinline__ void lik_ordinal_predictive(const OrdinalTable& tb, double m, double v, double& mean, double& var) {
  const double rs = M_SQRT1_2 / sqrt(tb.sigma * tb.sigma + v);
  double e1 = 1.0, e2 = 1.0;
  for (int k = 0; k < tb.K - 1; ++k) {
    const double q = 0.5 * erfc((tb.edge[k] - m) * rs);
    e1 += q;
    e2 += (double)(2 * k + 3) * q;
  }
  mean = e1;
  var = e2 - e1 * e1;
}

// Per-wave LDS scratch of the tensor-rule likelihoods (doubles): Categorical [0,80) exp(f_k(node i)), [80,160) f_k(node i),
// [160,170) normalised GH weights; Beta [0,80) a_i, psi(a_i), zeta(2,a_i), lgamma(a_i) and the same four for b_j;
// Student [0,60) r_i = y - f0(node i), f1(node j), s_j = exp(-f1(node j)); Dirichlet [0,40) a_k(node i), [40,50) weights,
// [56,64) m_k, v_k (predictive, T = 20: [0,80) a_k(node i), [80,88) m_k, v_k); Negative Binomial [0,20) min(f0(node i), LIM_VAL), then
// per node j of f1: [20,40) log r_j, [40,60) r_j, [60,80) G_j - lgamma(y+1), [80,100) r_j D1_j, [100,120) r_j^2 D2_j;
// Weibull [0,20) log y - f0(node i), [20,40) k_j, [40,60) log k_j; Beta-Binomial [0,80) a_i, G(k, a_i), a_i D1(k, a_i), a_i^2 D2(k, a_i),
// [80,160) the same four for b_j with n - k; zero-inflated Poisson (rows with y = 0 only) [0,20) lambda_i, [20,40) -expm1(-lambda_i), then per
// node j of f1: [40,60) log pi_j, [60,80) log(1 - pi_j), [80,100) pi_j, [100,120) pi_j (1 - pi_j).
#define HMOGP_ETAB 176

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// 1/d for a positive normal double: hardware seed + two Newton steps (error ~1e-16 relative; NOT correctly rounded)
__device__ __forceinline__ double fast_rcp_pos(double d) {
  double r = __builtin_amdgcn_rcp(d);
  r = fma(fma(-d, r, 1.0), r, r);
  r = fma(fma(-d, r, 1.0), r, r);
  return r;
}
// log(x) for a positive normal double: x = m 2^e with m in [sqrt(1/2), sqrt(2)), log m = 2 atanh(s), s = (m-1)/(m+1),
// |s| <= 0.1716: odd series to s^21.  Absolute error ~2e-16 (1 + |log x| eps); about half the instructions of the
// library log (no special cases: the caller guarantees 1 <= x < 1e300).
__device__ __forceinline__ double fast_log_pos(double x) {
  int e = __builtin_amdgcn_frexp_exp(x);
  double m = __builtin_amdgcn_frexp_mant(x);  // [0.5, 1)
  const bool lowm = m < 0.70710678118654752;
  m = lowm ? m + m : m;
  e = lowm ? e - 1 : e;
  const double s = (m - 1.0) * fast_rcp_pos(m + 1.0), z = s * s;
  double p = 1.0 / 21.0;
  p = fma(p, z, 1.0 / 19.0);
  p = fma(p, z, 1.0 / 17.0);
  p = fma(p, z, 1.0 / 15.0);
  p = fma(p, z, 1.0 / 13.0);
  p = fma(p, z, 1.0 / 11.0);
  p = fma(p, z, 1.0 / 9.0);
  p = fma(p, z, 1.0 / 7.0);
  p = fma(p, z, 1.0 / 5.0);
  p = fma(p, z, 1.0 / 3.0);
  p = fma(p * z, s + s, s + s);               // 2 s (1 + z p)
  const double de = (double)e;
  return fma(de, 6.93147180369123816490e-01, fma(de, 1.90821492927058770002e-10, p));
}

// ------------------------------------------------------------------------------------------- Beta, 10 x 10
// beta.py:29-36,76-197.  betaln / psi / zeta of (a+b) couple the two dimensions: 100 nodes over the 64 lanes.  Everything
// that depends on ONE dimension only -- a_i, psi(a_i), zeta(2, a_i), lgamma(a_i) and the same for b_j -- is evaluated once
// per row by 20 lanes into the wave's LDS table: 3 special functions per node (of a+b) instead of 9.
__device__ __forceinline__ void lik_beta_wave(double y, const double* m, const double* v, int lane, double* tab, LikOut& o) {
  if (lane < 20) {
    const int dim = lane / 10, i = lane - 10 * dim;
    const double x = clip(safe_exp(GH10_X[i] * sqrt(2.0 * v[dim]) + m[dim]), 1e-9, 1e9);
    double* t = tab + dim * 40 + i;
    t[0] = x, t[10] = digamma_pos(x), t[20] = trigamma_pos(x), t[30] = lgamma(x);
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  const double ly = log(y), l1y = log(1.0 - y);
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int n = lane; n < 100; n += 64) {
    const int i = n / 10, j = n - 10 * i;
    const double w = (GH10_WN[i] * INV_SQRT_PI) * (GH10_WN[j] * INV_SQRT_PI);
    const double a = tab[i], pa = tab[10 + i], za = tab[20 + i], lga = tab[30 + i];
    const double b = tab[40 + j], pb = tab[50 + j], zb = tab[60 + j], lgb = tab[70 + j];
    const double pab = digamma_pos(a + b), zab = trigamma_pos(a + b);
    const double lbeta = lga + lgb - lgamma(a + b);
    ve += w * ((a - 1.0) * ly + (b - 1.0) * l1y - lbeta);
    g0 += w * ((pab - pa + ly) * a);
    g1 += w * ((pab - pb + l1y) * b);
    h0 += w * ((pab + a * zab - pa - a * za + ly) * a);
    h1 += w * ((pab + b * zab - pb - b * zb + l1y) * b);
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

// ------------------------------------------------------------------------------------------- Dirichlet, 10^K
// DESIGN 9d (the reference's dirichlet.py is a constructor only).  A row's observation is a composition y on the open simplex; the
// kernels get ly[k] = log y_k.  K functions, a_k = clip(safe_exp(f_k), 1e-9, 1e9) (Beta's link and clip), A = sum_k a_k:
//   log p = lgamma(A) - sum_k lgamma(a_k) + sum_k (a_k - 1) ly_k
//   d/df_k = a_k (psi(A) - psi(a_k) + ly_k)        d2/df_k^2 = d/df_k + a_k^2 (psi'(A) - psi'(a_k))       (the clip is ignored)
// Under the 10-node-per-dimension tensor rule, weights w/sqrt(pi) once per dimension, W = prod_k w_{i_k}:
//   ve   = sum_nodes W lgamma(A)  - sum_k sum_i w_i lgamma(a_k(i))      + sum_k (sum_i w_i a_k(i) - 1) ly_k
//   dm_k = sum_nodes W a_k psi(A) - sum_i w_i a_k(i) psi(a_k(i))        + (sum_i w_i a_k(i)) ly_k
//   dv_k = 1/2 [ dm_k + sum_nodes W a_k^2 psi'(A) - sum_i w_i a_k(i)^2 psi'(a_k(i)) ]
// Only the three functions of A couple the dimensions.  The 10 K lanes that fill the wave's table [0, 10 K) a_k(i), [40, 50) weights
// ([56, 64) m_k, v_k) each add their own one-dimensional term into their running sums, so the reductions at the end deliver both parts at once.
// A is summed k = 0, 1, .. in this order everywhere (tests/dirichlet_ref.py does the same).
// The lane that fills table entry (k, i) needs m_k, v_k with a run-time k.  Indexing the register arrays m / v with it parks them (and
// the LikOut beside them) in scratch, and so does a chain of selects, which the compiler folds back into one indexed load; the wave's
// own LDS slice takes a run-time index for free, so lane 0 stages the 2 K numbers there: mv[k] = m_k, mv[4 + k] = v_k.
template <int K>
__device__ __forceinline__ void dirichlet_stage_mv(const double* m, const double* v, int lane, double* mv) {
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) mv[k] = m[k], mv[4 + k] = v[k];
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
}
__device__ __forceinline__ double dirichlet_alpha(const double* mv, int k, double x) {
  return clip(safe_exp(x * sqrt(2.0 * mv[4 + k]) + mv[k]), 1e-9, 1e9);
}

template <int K>
__device__ __forceinline__ void lik_dirichlet_wave(const double (&ly)[K], const double* m, const double* v, int lane, double* tab,
                                                   LikOut& o) {
  static_assert(K >= 2 && K <= HMOGP_DIRICHLET_MAXK && 10 * HMOGP_DIRICHLET_MAXK + 10 <= HMOGP_ETAB, "Dirichlet table");
  constexpr int NN = K == 2 ? 100 : (K == 3 ? 1000 : 10000);
  double* wtab = tab + 40;
  dirichlet_stage_mv<K>(m, v, lane, tab + 56);
  double ve = 0.0, g[K], h[K], s1[K];
#pragma unroll
  for (int k = 0; k < K; ++k) g[k] = h[k] = s1[k] = 0.0;
  if (lane < 10 * K) {
    const int k = lane / 10, i = lane - 10 * k;
    const double a = dirichlet_alpha(tab + 56, k, GH10_X[i]), w = GH10_WN[i];
    tab[lane] = a;
    const double wa = w * a, t2 = wa * digamma_pos(a), t3 = wa * a * trigamma_pos(a);
    ve = -(w * lgamma(a));
#pragma unroll
    for (int j = 0; j < K; ++j)
      if (k == j) s1[j] = wa, g[j] = -t2, h[j] = -t3;
  }
  if (lane < 10) wtab[lane] = GH10_WN[lane];
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  for (int n = lane; n < NN; n += 64) {
    double a[K], W = 1.0;
    int rem = n;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
      const int i = rem % 10;
      rem /= 10;
      a[k] = tab[k * 10 + i];
      W *= wtab[i];
    }
    double A = a[0];
#pragma unroll
    for (int k = 1; k < K; ++k) A += a[k];
    const double wp = W * digamma_pos(A), wz = W * trigamma_pos(A);
    ve = fma(W, lgamma(A), ve);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      g[k] = fma(wp, a[k], g[k]);
      h[k] = fma(wz * a[k], a[k], h[k]);
    }
  }
  double vs = wave_sum(ve);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double S1 = wave_sum(s1[k]);
    vs += (S1 - 1.0) * ly[k];
    const double gm = wave_sum(g[k]) + S1 * ly[k];
    o.gm[k] = gm;
    o.gv[k] = 0.5 * (gm + wave_sum(h[k]));
  }
  o.ve = vs;
}

// ------------------------------------------------------------------------------------------- Student-t, 20 x 20
// Heteroscedastic Student-t (the reference's student.py is a constructor only): f0 = location (identity link),
// f1 = log of the squared scale (sigma^2 = exp(f1), HetGaussian's convention), nu = deg_free fixed (the task's lik_param).
// With r = y - f0, s = exp(min(-f1, LIM_VAL)), u = r^2 s / nu:
//   log p = C(nu) - f1/2 - (nu+1)/2 log1p(u)
//   d/df0 = (nu+1) r s / (nu (1+u))          d2/df0^2 = (nu+1) s (u-1) / (nu (1+u)^2)
//   d/df1 = -1/2 + (nu+1)/2 u/(1+u)          d2/df1^2 = -(nu+1)/2 u/(1+u)^2
// C(nu) = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2.  From nu = 64 on the lgamma difference (two numbers of size
// nu/2 log(nu/2) that cancel to ~log(nu)/2) is its asymptotic series in x = nu/2 instead, truncation error < 1e-16:
//   lgamma(x + 1/2) - lgamma(x) = log(x)/2 - 1/(8x) + 1/(192x^3) - 1/(640x^5) + 17/(14336x^7) - ...
// so that C -> -log(2 pi)/2, HetGaussian's constant, without rounding noise of order nu eps.
__device__ __forceinline__ double student_logc(double nu) {
  if (nu < 64.0) return lgamma(0.5 * (nu + 1.0)) - lgamma(0.5 * nu) - 0.5 * log(nu * M_PI);
  const double ix = 2.0 / nu, z = ix * ix;
  return -0.5 * log(2.0 * M_PI) + ix * (-1.0 / 8.0 + z * (1.0 / 192.0 + z * (-1.0 / 640.0 + z * (17.0 / 14336.0))));
}

// 20 x 20 Gauss-Hermite tensor rule, weights w/sqrt(pi) once per dimension: ve = sum w_i w_j log p, dm_d = sum w w d/df_d,
// dv_d = 1/2 sum w w d2/df_d^2.  The node tables of each dimension (20 + 40 doubles) are formed once per row by 40 lanes in the
// wave's LDS slice; each of the 400 nodes then costs one log1p and one reciprocal.
__device__ __forceinline__ void lik_student_wave(double y, const double* m, const double* v, double nu, int lane, double* tab,
                                                 LikOut& o) {
  if (lane < 40) {
    const int dim = lane / 20, i = lane - 20 * dim;
    const double f = GH20_X[i] * sqrt(2.0 * v[dim]) + m[dim];
    if (dim == 0) {
      tab[i] = y - f;
    } else {
      tab[20 + i] = f;
      tab[40 + i] = safe_exp(-f);
    }
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  const double c = student_logc(nu), rnu = 1.0 / nu, hn = 0.5 * (nu + 1.0), kn = (nu + 1.0) * rnu;
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int n = lane; n < 400; n += 64) {
    const int i = n / 20, j = n - 20 * i;
    const double w = GH20_WN[i] * GH20_WN[j];
    const double r = tab[i], f1 = tab[20 + j], s = tab[40 + j];
    const double u = r * r * s * rnu, a = 1.0 / (1.0 + u), ua = u * a;
    ve += w * (c - 0.5 * f1 - hn * log1p(u));
    g0 += w * (kn * r * s * a);
    h0 += w * (kn * s * (u - 1.0) * a * a);
    g1 += w * (hn * ua - 0.5);
    h1 += w * (-hn * ua * a);
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

// ------------------------------------------------------------------------------------------- Negative Binomial, 20 x 20
// Heteroscedastic Negative Binomial (no counterpart in the reference): counts y = 0, 1, 2, ..; f0 = log of the mean,
// f1 = log of the dispersion ("size") r = clip(safe_exp(f1), 1e-9, 1e9) (Gamma's link and clip), Var[y | f] = mu + mu^2 / r.
// With lr = log r, z = min(f0, LIM_VAL) - lr, sp = softplus(z), p = sigmoid(z), q = 1 - p (mu and p never formed from exp(f0)):
//   log p  = G - lgamma(y+1) + y z - (r + y) sp             G  = lgamma(y+r) - lgamma(r)
//   d/df0  = y q - r p                                      D1 = psi(y+r)    - psi(r)
//   d2/df0 = -(r + y) p q                                   D2 = psi'(y+r)   - psi'(r)
//   d/df1  = r (D1 - sp) - d/df0
//   d2/df1 = r (D1 - sp) + r^2 D2 + 2 r p - (r + y) p q     (the clip is ignored in the derivatives, as for Gamma / Beta)
// G, D1, D2 are never the difference of two large numbers (at r = 1e9, y = 50 the plain difference of lgamma loses 4e-6 of 1e3):
//   y <= 32             the exact products / sums over k < y:  G = log prod (r + k),  D1 = sum 1/(r + k),  D2 = -sum 1/(r + k)^2
//                       (at most 32 factors <= 1e9 + 31: the product stays below 1e289 and carries <= 32 roundings)
//   y > 32, r >= 16     Stirling's series of the two arguments subtracted term by term, the leading terms in closed form:
//                         G  = y log(r+y) - y + (r - 1/2) log1p(y/r) + [c(r+y) - c(r)]       c(x) = 1/(12x) - 1/(360x^3) + ..
//                         D1 = log1p(y/r) + y / (2 r (r+y)) + [d(r) - d(r+y)]                d(x) = 1/(12x^2) - 1/(120x^4) + ..
//                         D2 = -y / (r (r+y)) - y (2r+y) / (2 r^2 (r+y)^2) - [e(r) - e(r+y)] e(x) = 1/(6x^3) - 1/(30x^5) + ..
//                       (every term of D1 is positive, of D2 negative; truncation at x = 16: c 1.1e-16, d 2.4e-20, e 2.4e-20)
//   y > 32, r < 16      the plain differences: lgamma(r), psi(r), psi'(r) are small beside their partners or dominate them.
__device__ __forceinline__ double nb_stirling_c(double x) {  // lgamma(x) - [(x - 1/2) log x - x + log(2 pi)/2], x >= 16
  const double ix = 1.0 / x, z = ix * ix;
  return ix * (1.0 / 12.0 + z * (-1.0 / 360.0 + z * (1.0 / 1260.0 + z * (-1.0 / 1680.0 + z * (1.0 / 1188.0)))));
}
__device__ __forceinline__ double nb_stirling_d(double x) {  // log x - 1/(2x) - psi(x), x >= 16
  const double ix = 1.0 / x, z = ix * ix;
  return z * (1.0 / 12.0 +
              z * (-1.0 / 120.0 + z * (1.0 / 252.0 + z * (-1.0 / 240.0 + z * (1.0 / 132.0 + z * (-691.0 / 32760.0 + z * (1.0 / 12.0)))))));
}
__device__ __forceinline__ double nb_stirling_e(double x) {  // psi'(x) - 1/x - 1/(2x^2), x >= 16
  const double ix = 1.0 / x, z = ix * ix;
  return ix * z *
         (1.0 / 6.0 + z * (-1.0 / 30.0 + z * (1.0 / 42.0 + z * (-1.0 / 30.0 + z * (5.0 / 66.0 + z * (-691.0 / 2730.0 + z * (7.0 / 6.0)))))));
}
// y: a non-negative integer-valued double (checked on the host), r in [1e-9, 1e9]; the Beta-Binomial also calls it with
// r = a + b up to 2e9 and y up to 1e9: the y <= 32 product then reaches (2e9 + 31)^32 = 4e297, still finite, and the series are unaffected
__device__ __forceinline__ void nb_gamma_diffs(double y, double r, double& G, double& D1, double& D2) {
  if (y <= 32.0) {
    const int ny = (int)y;
    double prod = 1.0, s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < ny; ++k) {
      const double t = r + (double)k, it = 1.0 / t;
      prod *= t;
      s1 += it;
      s2 = fma(it, it, s2);
    }
    G = log(prod), D1 = s1, D2 = -s2;
  } else if (r >= 16.0) {
    const double ry = r + y, l1 = log1p(y / r), rry = r * ry;
    G = y * log(ry) - y + (r - 0.5) * l1 + (nb_stirling_c(ry) - nb_stirling_c(r));
    D1 = l1 + y / (2.0 * rry) + (nb_stirling_d(r) - nb_stirling_d(ry));
    D2 = -y / rry - y * (2.0 * r + y) / (2.0 * rry * rry) - (nb_stirling_e(r) - nb_stirling_e(ry));
  } else {
    G = lgamma(y + r) - lgamma(r);
    D1 = digamma_pos(y + r) - digamma_pos(r);
    D2 = trigamma_pos(y + r) - trigamma_pos(r);
  }
}
__device__ __forceinline__ double nb_lgamma_diff(double y, double r) {
  double G, D1, D2;
  nb_gamma_diffs(y, r, G, D1, D2);
  return G;
}

// The full log p at one f (Monte-Carlo log predictive); lgy1 = lgamma(y + 1)
__device__ __forceinline__ double lik_negbinomial_logpdf(double y, double lgy1, const double* f) {
  const double r = clip(safe_exp(f[1]), 1e-9, 1e9);
  const double z = fmin(f[0], LIM_VAL) - log(r);
  const double sp = fmax(z, 0.0) + log1p(exp(-fabs(z)));
  return nb_lgamma_diff(y, r) - lgy1 + y * z - (r + y) * sp;
}

// 20 x 20 Gauss-Hermite tensor rule, weights w/sqrt(pi) once per dimension (Student's convention).  Lanes 0-19 write min(f0(node i), LIM_VAL)
// into the wave's LDS slice, lanes 20-39 what depends on f1(node j) alone: lr_j, r_j, G_j - lgamma(y+1), r_j D1_j, r_j^2 D2_j (y is
// the same in the whole wave: the y <= 32 loop does not diverge).  Each of the 400 nodes then costs one exp, one log1p and one reciprocal.
__device__ __forceinline__ void lik_negbinomial_wave(double y, double lgy1, const double* m, const double* v, int lane, double* tab,
                                                     LikOut& o) {
  static_assert(120 <= HMOGP_ETAB, "Negative Binomial table");
  if (lane < 40) {
    const int dim = lane / 20, i = lane - 20 * dim;
    const double f = GH20_X[i] * sqrt(2.0 * v[dim]) + m[dim];
    if (dim == 0) {
      tab[i] = fmin(f, LIM_VAL);
    } else {
      const double r = clip(safe_exp(f), 1e-9, 1e9);
      double G, D1, D2;
      nb_gamma_diffs(y, r, G, D1, D2);
      tab[20 + i] = log(r);
      tab[40 + i] = r;
      tab[60 + i] = G - lgy1;
      tab[80 + i] = r * D1;
      tab[100 + i] = r * r * D2;
    }
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int n = lane; n < 400; n += 64) {
    const int i = n / 20, j = n - 20 * i;
    const double w = GH20_WN[i] * GH20_WN[j];
    const double r = tab[40 + j], z = tab[i] - tab[20 + j];
    const double a = exp(-fabs(z)), inv = 1.0 / (1.0 + a), ai = a * inv;
    const double sp = fmax(z, 0.0) + log1p(a);
    const double p = z >= 0.0 ? inv : ai, q = z >= 0.0 ? ai : inv;
    const double rp = r * p, d0 = y * q - rp, ppq = (r + y) * p * q, c = tab[80 + j] - r * sp;
    ve += w * (tab[60 + j] + y * z - (r + y) * sp);
    g0 += w * d0;
    h0 -= w * ppq;
    g1 += w * (c - d0);
    h1 += w * (c + tab[100 + j] + 2.0 * rp - ppq);
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

// ------------------------------------------------------------------------------------------- Weibull with right-censoring, 20 x 20
// DESIGN 9i (no counterpart in the reference): a time to an event y > 0 with the indicator delta = 1 (the event was observed at y) or
// 0 (right-censored: the event is later than y).  f0 = log of the scale lambda, f1 = log of the shape
// k = clip(safe_exp(f1), 1e-3, 1e3), lk = log k.  With ly = log y (formed once per row on the host), z = min(k (ly - f0), 680),
// e = exp(z) = (y / lambda)^k (never formed by pow: y^k overflows where the quotient does not):
//   log p   = delta (lk - ly + z) - e            (delta = 0: the log survival function -e)
//   d/df0   = k (e - delta)                      d2/df0^2 = -k^2 e
//   d/df1   = delta (1 + z) - e z                d2/df1^2 = z (delta - e - e z)      (the clips are ignored in the derivatives)
// The clip of z keeps every addend finite: k^2 e <= 1e301.4, e z^2 <= 1e301.  delta is 0.0 or 1.0 exactly (checked on the host),
// so the products with it are exact and the row needs no branch.
#define HMOGP_WEIBULL_ZMAX 680.0
__device__ __forceinline__ double weibull_shape(double f1) { return clip(safe_exp(f1), 1e-3, 1e3); }

// The full log p at one f (Monte-Carlo log predictive): a censored row scores its survival probability
__device__ __forceinline__ double lik_weibull_logpdf(double ly, double delta, const double* f) {
  const double k = weibull_shape(f[1]);
  const double z = fmin(k * (ly - f[0]), HMOGP_WEIBULL_ZMAX);
  return delta * (log(k) - ly + z) - exp(z);
}

// 20 x 20 Gauss-Hermite tensor rule, weights w/sqrt(pi) once per dimension (Student's convention).  Lanes 0-19 write ly - f0(node i) into
// the wave's LDS slice, lanes 20-39 k_j and lk_j; each of the 400 nodes then costs one exp.
__device__ __forceinline__ void lik_weibull_wave(double ly, double delta, const double* m, const double* v, int lane, double* tab,
                                                 LikOut& o) {
  static_assert(60 <= HMOGP_ETAB, "Weibull table");
  if (lane < 40) {
    const int dim = lane / 20, i = lane - 20 * dim;
    const double f = GH20_X[i] * sqrt(2.0 * v[dim]) + m[dim];
    if (dim == 0) {
      tab[i] = ly - f;
    } else {
      const double k = weibull_shape(f);
      tab[20 + i] = k;
      tab[40 + i] = log(k);
    }
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int n = lane; n < 400; n += 64) {
    const int i = n / 20, j = n - 20 * i;
    const double w = GH20_WN[i] * GH20_WN[j];
    const double k = tab[20 + j];
    const double z = fmin(k * tab[i], HMOGP_WEIBULL_ZMAX), e = exp(z), ez = e * z;
    ve += w * (delta * (tab[40 + j] - ly + z) - e);
    g0 += w * (k * (e - delta));
    h0 -= w * (k * k * e);
    g1 += w * (delta * (1.0 + z) - ez);
    h1 += w * (z * (delta - e - ez));
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

// Predictive moments of the event time under independent q(f0), q(f1): E[lambda^p] in closed form, E[Gamma(1 + p / k)] by the
// 20-node rule over f1 (lgamma, then exp); no clip of the result: overflow is +inf.
__device__ __forceinline__ void lik_weibull_predictive(const double* m, const double* v, double& mean, double& var) {
  const double s1 = sqrt(2.0 * v[1]);
  double g1 = 0.0, g2 = 0.0;
  for (int j = 0; j < 20; ++j) {
    const double ik = 1.0 / weibull_shape(GH20_X[j] * s1 + m[1]);
    g1 += GH20_WN[j] * exp(lgamma(1.0 + ik));
    g2 += GH20_WN[j] * exp(lgamma(1.0 + 2.0 * ik));
  }
  mean = exp(m[0] + 0.5 * v[0]) * g1;
  const double e2 = exp(2.0 * m[0] + 2.0 * v[0]) * g2;
  var = e2 < INFINITY ? e2 - mean * mean : INFINITY;
}

// ------------------------------------------------------------------------------------------- Categorical
// categorical.py:37-46,77-82,102-222.  K classes, D = K-1 functions, labels 1..K (class K = reference class),
// 10^D tensor nodes.  The node dependence factorises through exp(f_k) per dimension: a per-wave LDS
// table holds exp(f_k(node i)) and f_k(node i), [D][10] each.  The LAST min(D,3) dimensions are strided over the lanes
// (their digits, table entries and weight product are formed once per lane and chunk); the remaining leading dimensions
// are a uniform outer loop.  A node whose probabilities are not touched by the reference's clip to [1e-9, 1-1e-9] takes
//   log p_y = f_y - log(den),  d2 = -p_d (1 + sum_{j != d} e_j)/den      (one reciprocal, one log per node)
// which equals the reference's clipped / renormalised expressions to rounding; any other node (clip active, overflow)
// takes the literal formulas.
template <int D>
__device__ __forceinline__ void cat_node_literal(const double (&e)[D], double w, int label, bool exact_dm, double& ve,
                                                 double (&hv)[D], double (&gx)[D]) {
  constexpr int K = D + 1;
  double esum = 0.0;
#pragma unroll
  for (int k = D - 1; k >= 0; --k) esum += e[k];
  const double den = 1.0 + esum;
  double psum = 0.0, py = 0.0;  // class probabilities, clipped then renormalised (:41-44)
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double pk = clip(e[k] / den, 1e-9, 1.0 - 1e-9);
    psum += pk;
    if (label == k + 1) py = pk;
  }
  const double pK = clip(1.0 / den, 1e-9, 1.0 - 1e-9);
  psum += pK;
  if (label == K) py = pK;
  ve += w * log(py / psum);
  // second derivative of log p wrt f_d (:115-128): -(e_d + sum_{j != d} e^{f_j + f_d}) / den^2, independent of y
  const double den2 = safe_square(den);
#pragma unroll
  for (int d = 0; d < D; ++d) {
    double num = e[d];
#pragma unroll
    for (int j = 0; j < D; ++j)
      if (j != d) num += fmin(e[j] * e[d], 1.79769313486231570815e308);
    hv[d] += w * (num / den2);
    if (exact_dm) gx[d] += w * ((label == d + 1 ? 1.0 : 0.0) - e[d] / den);  // E[d log p_y / d f_d], softmax
  }
}

// rest_d = den - e_d = 1 + sum_{j != d} e_j, formed by prefix and suffix sums and never by the subtraction: where one function
// dominates (e_d >> 1 + the others) den - e_d cancels to nothing in float64, while the reference adds e_d + sum_j e^{f_j + f_d}
// and loses no digit.  SKIP >= 0 leaves function SKIP out of the sums (the register dimension, added by the caller).
template <int D, int SKIP = -1>
__device__ __forceinline__ void cat_rest(const double (&e)[D], double (&rest)[D]) {
  double pre = 1.0;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    rest[d] = pre;
    if (d != SKIP) pre += e[d];
  }
  double suf = 0.0;
#pragma unroll
  for (int d = D - 1; d >= 0; --d) {
    if (d < D - 1) rest[d] += suf;
    if (d != SKIP) suf += e[d];
  }
}

// One node whose probabilities ARE touched by the clip, denominators far from overflow (den < 1e150): the literal formulas
// with every division replaced by a multiplication with a Newton-refined reciprocal and the library log by fast_log_pos
// (<= 2 ulp away from the reference's IEEE divisions; a clip comparison can only flip for a value within an ulp of the bound).
template <int D>
__device__ __forceinline__ void cat_node_clipped(const double (&e)[D], double den, double w, int label, bool exact_dm,
                                                 double& ve, double (&hv)[D], double (&gx)[D]) {
  constexpr int K = D + 1;
  const double rden = fast_rcp_pos(den);
  double psum = 0.0, py = 0.0;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double pk = clip(e[k] * rden, 1e-9, 1.0 - 1e-9);
    psum += pk;
    if (label == k + 1) py = pk;
  }
  const double pK = clip(rden, 1e-9, 1.0 - 1e-9);
  psum += pK;
  if (label == K) py = pK;
  ve = fma(w, fast_log_pos(py) - fast_log_pos(psum), ve);
  double rest[D];
  cat_rest<D>(e, rest);
#pragma unroll
  for (int d = 0; d < D; ++d) {   // (e_d + sum_{j != d} e_j e_d) / den^2 = e_d (1 + sum_{j != d} e_j) / den^2, no overflow below 1e150
    const double pd = e[d] * rden;
    hv[d] = fma(w * pd, rest[d] * rden, hv[d]);
    if (exact_dm) gx[d] = fma(w, (label == d + 1 ? 1.0 : 0.0) - pd, gx[d]);
  }
}

// One node on the "clip inactive" path: log p_y = f_y - log(den), d2 log p / df_d^2 = -p_d (1 + sum_{j != d} e_j) / den.
template <int D>
__device__ __forceinline__ void cat_node_fast(const double (&e)[D], double den, double w, double fy, int label, bool exact_dm,
                                              double& ve, double (&hv)[D], double (&gx)[D]) {
  const double rden = fast_rcp_pos(den);
  ve = fma(w, fy - fast_log_pos(den), ve);
  double rest[D];
  cat_rest<D>(e, rest);
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double pd = e[d] * rden;
    hv[d] = fma(w * pd, rest[d] * rden, hv[d]);
    if (exact_dm) gx[d] = fma(w, (label == d + 1 ? 1.0 : 0.0) - pd, gx[d]);
  }
}

// Loop structure (D functions, nodes in the reference's C order, function 0 slowest):
//   * the LAST min(D,3) dimensions are strided over the 64 lanes in chunks; their digits, table entries, weight product
//     and partial sum are formed once per lane and chunk;
//   * when D > 3, dimension D-4 is the REGISTER dimension: its ten table entries (exp f, f, weight) are preloaded into
//     registers once per row and its loop is fully unrolled -- ten independent nodes per trip, no LDS access and no index
//     arithmetic inside, so the scheduler can interleave their reciprocal / logarithm chains;
//   * dimensions 0 .. D-5 (D > 4) form a uniform outer loop whose table reads are amortised over those ten nodes.
// Whether the ten nodes of a trip may all take the fast path is decided once per trip from the largest / smallest
// denominator of the trip; otherwise each node of the trip is routed individually.
template <int D>
__device__ __forceinline__ void lik_categorical_t(double y, const double* m, const double* v, int lane, double* tab,
                                                  unsigned quirks, LikOut& o) {
  constexpr int K = D + 1;
  constexpr int DI = D < 3 ? D : 3;                          // lane-strided inner dimensions: functions D-DI .. D-1
  constexpr int HASR = D > 3 ? 1 : 0;                        // register dimension: function D-4
  constexpr int DS = D - DI - HASR;                          // slow (uniform) outer dimensions: functions 0 .. DS-1
  constexpr int NIN = DI == 1 ? 10 : (DI == 2 ? 100 : 1000);
  constexpr int RD = D - DI - 1;                             // index of the register dimension (valid when HASR)
  int NSLOW = 1;
#pragma unroll
  for (int k = 0; k < DS; ++k) NSLOW *= 10;
  double* etab = tab;
  double* ftab = tab + 80;
  double* wtab = tab + 160;
  for (int t = lane; t < D * 10; t += 64) {
    const int k = t / 10, i = t - 10 * k;
    const double f = GH10_X[i] * sqrt(2.0 * v[k]) + m[k];
    etab[t] = safe_exp(f), ftab[t] = f;
  }
  if (lane < 10) wtab[lane] = GH10_WN[lane];
  __builtin_amdgcn_wave_barrier();  // the tables are written and read by this wave only (LDS ops are in order)
  const int label = (int)y;  // 1..K
  const bool valid = (y == (double)label) && label >= 1 && label <= K;
  const bool exact_dm = (quirks & HMOGP_QUIRK_CATEGORICAL_DM) == 0;
  double er[HASR ? 10 : 1], wr[HASR ? 10 : 1], fr[HASR ? 10 : 1];
  if (HASR) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      er[i] = etab[RD * 10 + i], wr[i] = wtab[i];
      fr[i] = (label == RD + 1) ? ftab[RD * 10 + i] : 0.0;
    }
  }
  double ve = 0.0, hv[D], gx[D];
#pragma unroll
  for (int k = 0; k < D; ++k) hv[k] = gx[k] = 0.0;
  for (int base = 0; base < NIN; base += 64) {
    const int idx = base + lane;
    if (idx >= NIN) continue;
    // A node takes the fast path when the reference's clip to [1e-9, 1-1e-9] cannot touch any of its K probabilities
    // t / den, t in {e_0 .. e_{D-1}, 1}:  min t >= 1e-9 den  and  max t <= (1 - 1e-9) den  (and den finite).  The smallest /
    // largest t of the inner and slow dimensions are hoisted out of the register dimension's loop.
    double e[D], fy_in = 0.0, win = 1.0, sin_ = 0.0, lo_in = 1.0, hi_in = 1.0;
    int rem = idx;
#pragma unroll
    for (int t = DI - 1; t >= 0; --t) {  // digits of the inner dimensions, fastest first (the reference's weight order)
      const int i = rem % 10;
      rem /= 10;
      const int k = D - DI + t;
      e[k] = etab[k * 10 + i];
      if (label == k + 1) fy_in = ftab[k * 10 + i];
      win *= wtab[i];
      sin_ += e[k];
      lo_in = fmin(lo_in, e[k]), hi_in = fmax(hi_in, e[k]);
    }
    for (int sc = 0; sc < NSLOW; ++sc) {
      double ws = win, fys = fy_in, ss = sin_, lo = lo_in, hi = hi_in;
      int r2 = sc;
#pragma unroll
      for (int k = DS - 1; k >= 0; --k) {  // uniform digits of the slow outer dimensions
        const int i = r2 % 10;
        r2 /= 10;
        e[k] = etab[k * 10 + i];
        if (label == k + 1) fys = ftab[k * 10 + i];
        ws *= wtab[i];
        ss += e[k];
        lo = fmin(lo, e[k]), hi = fmax(hi, e[k]);
      }
      if (!HASR) {
        const double den = 1.0 + ss;
        if (den < 1e300 && den * 1e-9 <= lo && den * (1.0 - 1e-9) >= hi)
          cat_node_fast<D>(e, den, ws, fys, label, exact_dm, ve, hv, gx);
        else if (den < 1e150)
          cat_node_clipped<D>(e, den, ws, label, exact_dm, ve, hv, gx);
        else
          cat_node_literal<D>(e, ws, label, exact_dm, ve, hv, gx);
      } else {
        // NB the weight of the register dimension multiplies BEFORE the slow dimensions' in the reference's order; the
        // product of ten normalised weights is formed here as (inner * register) * slow -- same factors, and the fast
        // path only promises 1e-15 anyway; the literal path below restores the reference's order exactly.
        bool all_fast = true;
#pragma unroll
        for (int i = 0; i < 10; ++i) {
          const double den = 1.0 + (ss + er[i]);
          all_fast = all_fast && den < 1e300 && den * 1e-9 <= fmin(lo, er[i]) && den * (1.0 - 1e-9) >= fmax(hi, er[i]);
        }
        if (all_fast) {
          // Ten fast-path nodes that differ in the register dimension only.  For every OTHER dimension d the entry e_d is the
          // same in all ten and den_i - e_d = rest_d + er_i with rest_d = 1 + the entries of the remaining dimensions, so
          //   sum_i w_i p_di (1 - p_di) = e_d (rest_d B + C),  B = sum_i w_i / den_i^2,  C = sum_i w_i er_i / den_i^2
          // (all terms positive: no cancellation where one function dominates), and for the register dimension itself
          // den_i - er_i = 1 + ss:  sum_i w_i p_i (1 - p_i) = (1 + ss) C.  sum_i w_i (delta - p_di) = delta W - e_d A with
          // A = sum_i w_i / den_i.  Three running sums per node instead of five operations per node and dimension.
          double A = 0.0, B = 0.0, Cs = 0.0, Wt = 0.0;
#pragma unroll
          for (int i = 0; i < 10; ++i) {
            const double den = 1.0 + (ss + er[i]), w = ws * wr[i];
            const double rden = fast_rcp_pos(den);
            ve = fma(w, (fys + fr[i]) - fast_log_pos(den), ve);
            const double w1 = w * rden, w2 = w1 * rden;
            A += w1, B += w2;
            Cs = fma(w2, er[i], Cs);
            if (exact_dm) {
              Wt += w;
              gx[RD] = fma(-w1, er[i], gx[RD]);
            }
          }
          hv[RD] = fma(1.0 + ss, Cs, hv[RD]);
          if (exact_dm && label == RD + 1) gx[RD] += Wt;
          double rest[D];
          cat_rest<D, RD>(e, rest);
#pragma unroll
          for (int d = 0; d < D; ++d) {
            if (d == RD) continue;
            hv[d] = fma(e[d], fma(rest[d], B, Cs), hv[d]);
            if (exact_dm) gx[d] += (label == d + 1 ? Wt : 0.0) - e[d] * A;
          }
        } else {
#pragma unroll 1
          for (int i = 0; i < 10; ++i) {
            e[RD] = etab[RD * 10 + i];
            double w = win * wtab[i];  // reference order: inner dims (fastest first), then RD, then the slow dims
            int r3 = sc;
#pragma unroll
            for (int k = DS - 1; k >= 0; --k) {
              w *= wtab[r3 % 10];
              r3 /= 10;
            }
            const double den = 1.0 + (ss + e[RD]);
            if (den < 1e300 && den * 1e-9 <= fmin(lo, e[RD]) && den * (1.0 - 1e-9) >= fmax(hi, e[RD]))
              cat_node_fast<D>(e, den, w, fys + ((label == RD + 1) ? ftab[RD * 10 + i] : 0.0), label, exact_dm, ve, hv, gx);
            else if (den < 1e150)
              cat_node_clipped<D>(e, den, w, label, exact_dm, ve, hv, gx);
            else
              cat_node_literal<D>(e, w, label, exact_dm, ve, hv, gx);
          }
        }
      }
    }
  }
  o.ve = valid ? wave_sum(ve) : nan("");
  double wpow = 1.0;
#pragma unroll
  for (int k = 0; k < D; ++k) wpow *= GH10_WSUM_OVER_SQRTPI;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const double s = wave_sum(hv[d]);
    o.gv[d] = valid ? -0.5 * s : 0.0;
    if (exact_dm) {
      const double g = wave_sum(gx[d]);
      o.gm[d] = valid ? g : 0.0;
    } else {
      o.gm[d] = ((label == d + 1 ? 1.0 : 0.0) - (valid ? 1.0 : 0.0)) * wpow;  // quirk Q2
    }
  }
}

// ============================================================================ predictive moments
// `<likelihood>.predictive(m, v)`: mean and variance of y under q(f) = N(m, diag v).  One lane per row for the closed
// forms and 1-D rules, one wave per row for the T x T (Gamma, Beta) and 10^(K-1) (Categorical) tensor rules.
// T = 20 on a fresh reference instance, 10 when var_exp ran first on it (GPy caches the first rule, quirk Q7).
__device__ __forceinline__ double gh_x(int T, int i) { return T == 10 ? GH10_X[i] : GH20_X[i]; }
__device__ __forceinline__ double gh_wn(int T, int i) { return T == 10 ? GH10_WN[i] : GH20_WN[i]; }

template <int LIK>
__device__ __forceinline__ void lik_predictive(const double* m, const double* v, double param, int T, int lane, double* etab,
                                               double* mean, double* var) {
  if (LIK == HMOGP_LIK_GAUSSIAN) {  // gaussian.py:64-67
    mean[0] = m[0];
    var[0] = param * param + v[0];
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {  // hetgaussian.py:75-88
    const double s1 = sqrt(2.0 * v[0]), s2 = sqrt(2.0 * v[1]);
    double e2 = 0.0, sq = 0.0;
    for (int i = 0; i < T; ++i) {
      const double w = gh_wn(T, i);
      e2 += safe_exp(gh_x(T, i) * s2 + m[1]) * w;
      sq += safe_square(gh_x(T, i) * s1 + m[0]) * w;
    }
    mean[0] = m[0];
    var[0] = e2 + sq - m[0] * m[0];
  } else if (LIK == HMOGP_LIK_BERNOULLI || LIK == HMOGP_LIK_POISSON || LIK == HMOGP_LIK_EXPONENTIAL) {
    const double s = sqrt(2.0 * v[0]);  // bernoulli.py:113-128, poisson.py:97-112, exponential.py:101-116
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = 0; i < T; ++i) {
      const double f = gh_x(T, i) * s + m[0], w = gh_wn(T, i);
      double mu, vr, ms;
      if (LIK == HMOGP_LIK_BERNOULLI) {
        const double ef = safe_exp(f);
        const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
        mu = p, vr = p * (1.0 - p), ms = p * p;
      } else if (LIK == HMOGP_LIK_POISSON) {
        const double ef = safe_exp(f);
        mu = ef, vr = ef, ms = ef * ef;
      } else {
        const double b = clip(safe_exp(-f), 1e-9, 1e9);
        mu = b, vr = safe_square(b), ms = safe_square(b);
      }
      a0 += mu * w;
      a1 += vr * w;
      a2 += ms * w;
    }
    mean[0] = a0;
    var[0] = a1 + a2 - a0 * a0;
  } else if (LIK == HMOGP_LIK_GAMMA || LIK == HMOGP_LIK_BETA) {  // gamma.py:196-238, beta.py:199-241 (quirk Q1)
    const double s1 = sqrt(2.0 * v[0]), s2 = sqrt(2.0 * v[1]);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int n = lane; n < T * T; n += 64) {
      const int i = n / T, j = n - T * i;
      const double w = (gh_wn(T, i) * INV_SQRT_PI) * (gh_wn(T, j) * INV_SQRT_PI);
      const double a = clip(safe_exp(gh_x(T, i) * s1 + m[0]), 1e-9, 1e9);
      const double b = clip(safe_exp(gh_x(T, j) * s2 + m[1]), 1e-9, 1e9);
      double mu, vr;
      if (LIK == HMOGP_LIK_GAMMA) {
        mu = a / b;
        vr = a / (b * b);
      } else {
        mu = a / (a + b);
        vr = a * b / ((a + b) * (a + b) * (a + b + 1.0));
      }
      a0 += w * mu;
      a1 += w * vr;
      a2 += w * mu * mu;
    }
    a0 = wave_sum(a0), a1 = wave_sum(a1), a2 = wave_sum(a2);
    mean[0] = a0;
    var[0] = a1 + a2 - safe_square(a0);
  } else if (LIK == HMOGP_LIK_STUDENT) {  // closed form: the moments do not exist for nu <= 1 / nu <= 2
    mean[0] = param > 1.0 ? m[0] : nan("");
    var[0] = param > 2.0 ? v[0] + param / (param - 2.0) * safe_exp(m[1] + 0.5 * v[1]) : INFINITY;
  } else if (LIK == HMOGP_LIK_NEGBINOMIAL) {  // closed form: q(f0), q(f1) independent; no clip, overflow is +inf
    const double mu = exp(m[0] + 0.5 * v[0]);
    mean[0] = mu;
    var[0] = mu + exp(2.0 * m[0] + 2.0 * v[0] - m[1] + 0.5 * v[1]) + (v[0] > 0.0 ? expm1(v[0]) * exp(2.0 * m[0] + v[0]) : 0.0);
  } else if (LIK == HMOGP_LIK_WEIBULL) {  // one lane per row, GH20 over f1
    lik_weibull_predictive(m, v, mean[0], var[0]);
  } else if (LIK == HMOGP_LIK_BINOMIAL) {  // one lane per row, param = the trial count n*
    lik_binomial_predictive(m[0], v[0], param, T, mean[0], var[0]);
  } else if (LIK == HMOGP_LIK_BETABINOMIAL) {
    lik_betabinomial_predictive(m, v, param, T, mean[0], var[0]);
  } else if (LIK == HMOGP_LIK_ZIPOISSON) {  // one lane per row, the T nodes over f1
    lik_zipoisson_predictive(m, v, T, mean[0], var[0]);
  } else {  // Categorical, categorical.py:84-99,224-269: E[rho_d], rho normalised over the K-1 columns; variance zeros
    const int D = (int)param - 1;
    for (int e = lane; e < D * 10; e += 64) {
      const int k = e / 10, i = e - 10 * k;
      etab[e] = safe_exp(GH10_X[i] * sqrt(2.0 * v[k]) + m[k]);
    }
    __builtin_amdgcn_wave_barrier();
    int total = 1;
    for (int k = 0; k < D; ++k) total *= 10;
    double acc[HMOGP_MAXJ];
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k) acc[k] = 0.0;
    for (int n = lane; n < total; n += 64) {
      double e[HMOGP_MAXJ];
      double w = 1.0, esum = 0.0;
      int rem = n;
#pragma unroll
      for (int k = HMOGP_MAXJ - 1; k >= 0; --k) {
        if (k < D) {
          const int i = rem % 10;
          rem /= 10;
          e[k] = etab[k * 10 + i];
          w *= GH10_WN[i];
          esum += e[k];
        } else {
          e[k] = 0.0;
        }
      }
      double rs = 0.0;
#pragma unroll
      for (int k = 0; k < HMOGP_MAXJ; ++k)
        if (k < D) {
          e[k] = clip(e[k] / (1.0 + esum), 1e-9, 1.0 - 1e-9);
          rs += e[k];
        }
#pragma unroll
      for (int k = 0; k < HMOGP_MAXJ; ++k)
        if (k < D) acc[k] += w * (e[k] / rs);
    }
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k)
      if (k < D) {
        mean[k] = wave_sum(acc[k]);
        var[k] = 0.0;
      }
  }
}

// ---- Dirichlet
// predictive moments of the composition under q(f), T^K tensor rule, one wave per row:
//   mean_k = E[a_k / A],   var_k = E[a_k (A - a_k) / (A^2 (A + 1))] + E[(a_k / A)^2] - mean_k^2
template <int K>
__device__ __forceinline__ void lik_dirichlet_predictive(const double* m, const double* v, int T, int lane, double* tab,
                                                         double* mean, double* var) {
  dirichlet_stage_mv<K>(m, v, lane, tab + 80);
  for (int e = lane; e < K * T; e += 64) {
    const int k = e / T, i = e - T * k;
    tab[e] = dirichlet_alpha(tab + 80, k, gh_x(T, i));
  }
  __builtin_amdgcn_wave_barrier();
  int total = 1;
#pragma unroll
  for (int k = 0; k < K; ++k) total *= T;
  double a0[K], a1[K], a2[K];
#pragma unroll
  for (int k = 0; k < K; ++k) a0[k] = a1[k] = a2[k] = 0.0;
  for (int n = lane; n < total; n += 64) {
    double a[K], W = 1.0;
    int rem = n;
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
      const int i = rem % T;
      rem /= T;
      a[k] = tab[k * T + i];
      W *= gh_wn(T, i);
    }
    double A = a[0];
#pragma unroll
    for (int k = 1; k < K; ++k) A += a[k];
    const double den = A * A * (A + 1.0);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const double p = a[k] / A;
      a0[k] += W * p;
      a1[k] += W * (a[k] * (A - a[k]) / den);
      a2[k] += W * (p * p);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double mu = wave_sum(a0[k]);
    mean[k] = mu;
    var[k] = wave_sum(a1[k]) + wave_sum(a2[k]) - mu * mu;
  }
}

// the full log p at one sample f of q(f) (Monte-Carlo log predictive)
template <int K>
__device__ __forceinline__ double lik_dirichlet_logpdf(const double (&ly)[K], const double* f) {
  double A = 0.0, r = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double a = clip(safe_exp(f[k]), 1e-9, 1e9);
    A += a;
    r += (a - 1.0) * ly[k] - lgamma(a);
  }
  return lgamma(A) + r;
}

// ============================================================================ Monte-Carlo log predictive
// log p(y|f) at ONE sample f of q(f), as the reference's `log_predictive` evaluates it (gaussian.py:28-34 -- sigma is
// ignored, quirk Q6 --, bernoulli.py:31-36, hetgaussian.py:35-39, poisson.py:31-34, exponential.py:28-32,
// categorical.py:48-63; Student: the full log p of DESIGN 9; Ordinal: the un-clipped log p of DESIGN 9b, y / yaux = the row's
// lower / upper cut point and param = sigma as in the quadrature).  Gamma and Beta have no log_predictive in the reference.
template <int LIK>
__device__ __forceinline__ double lik_logpdf_sample(double y, double yaux, const double* f, double param) {
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    const double d = y - f[0];
    return -0.5 * log(2.0 * M_PI) - 0.5 * d * d;
  } else if (LIK == HMOGP_LIK_BERNOULLI) {
    const double ef = safe_exp(f[0]);
    const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
    return y * log(p) + (1.0 - y) * log(1.0 - p);
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    const double ev = safe_exp(f[1]);
    return -0.5 * log(2.0 * M_PI) - 0.5 * f[1] - 0.5 * (safe_square(y - f[0]) / ev);
  } else if (LIK == HMOGP_LIK_POISSON) {
    return -safe_exp(f[0]) + y * f[0] - yaux;
  } else if (LIK == HMOGP_LIK_EXPONENTIAL) {
    const double b = clip(safe_exp(-f[0]), 1e-9, 1e9);
    return -log(b) - y / b;
  } else if (LIK == HMOGP_LIK_CATEGORICAL) {
    const int K = (int)param, D = K - 1, label = (int)y;
    double esum = 0.0, e[HMOGP_MAXJ];
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k) {
      e[k] = (k < D) ? safe_exp(f[k]) : 0.0;
      esum += e[k];
    }
    const double den = 1.0 + esum;
    double psum = 0.0, py = 0.0;
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k)
      if (k < D) {
        const double pk = clip(e[k] / den, 1e-9, 1.0 - 1e-9);
        psum += pk;
        if (label == k + 1) py = pk;
      }
    const double pK = clip(1.0 / den, 1e-9, 1.0 - 1e-9);
    psum += pK;
    if (label == K) py = pK;
    return log(py / psum);
  } else if (LIK == HMOGP_LIK_STUDENT) {
    const double r = y - f[0];
    return student_logc(param) - 0.5 * f[1] - 0.5 * (param + 1.0) * log1p(r * r * safe_exp(-f[1]) / param);
  } else if (LIK == HMOGP_LIK_ORDINAL) {
    double lp, g, h;
    ordinal_node((y - f[0]) / param, (yaux - f[0]) / param, lp, g, h);
    return lp;
  } else if (LIK == HMOGP_LIK_NEGBINOMIAL) {  // yaux = lgamma(y + 1)
    return lik_negbinomial_logpdf(y, yaux, f);
  } else if (LIK == HMOGP_LIK_WEIBULL) {  // y = log of the time, yaux = delta
    return lik_weibull_logpdf(y, yaux, f);
  } else if (LIK == HMOGP_LIK_BINOMIAL) {  // y = k, yaux = lc, param = the row's own trial count n
    return lik_binomial_logpdf(y, param, yaux, f);
  } else if (LIK == HMOGP_LIK_BETABINOMIAL) {
    return lik_betabinomial_logpdf(y, param, yaux, f);
  } else if (LIK == HMOGP_LIK_ZIPOISSON) {  // yaux = lgamma(y + 1)
    return lik_zipoisson_logpdf(y, yaux, f);
  }
  return nan("");
}

// counter-based generator: two standard normals from (seed, row, sample, pair) via splitmix64 + Box-Muller
__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ULL;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
  return x ^ (x >> 31);
}
__device__ __forceinline__ void normal_pair(unsigned long long seed, long long n, int s, int pair, double& z0, double& z1) {
  const unsigned long long h = splitmix64(splitmix64(seed ^ (unsigned long long)n * 0xD1342543DE82EF95ULL) ^
                                          ((unsigned long long)s << 8) ^ (unsigned long long)pair);
  const unsigned long long h2 = splitmix64(h);
  const double u1 = ((double)(h >> 11) + 1.0) * (1.0 / 9007199254740993.0);  // (0, 1)
  const double u2 = (double)(h2 >> 11) * (1.0 / 9007199254740992.0);         // [0, 1)
  const double r = sqrt(-2.0 * log(u1));
  z0 = r * cos(2.0 * M_PI * u2);
  z1 = r * sin(2.0 * M_PI * u2);
}

// ============================================================================ data generation (`samples`)
// One draw y ~ p(y | f) per row with the link functions and clips of the reference's `<likelihood>.samples`
// (gaussian.py:36-39, bernoulli.py:59-64, hetgaussian.py:41-44, poisson.py:51-54, exponential.py:52-56, gamma.py:43-50,
// beta.py:38-45, categorical.py:65-75).  Counter-based generator (reproducible per (seed, row); a different stream than
// NumPy's, so only the DISTRIBUTION is comparable with the reference): uniforms from splitmix64, normals by Box-Muller,
// Poisson by multiplication (lambda < 10) / Hoermann's PTRS transformed rejection, Gamma by Marsaglia-Tsang.
struct RowRng {
  unsigned long long key, ctr;
  __device__ RowRng(unsigned long long seed, long long row) : key(splitmix64(seed ^ (unsigned long long)row * 0xD1342543DE82EF95ULL)), ctr(0) {}
  __device__ double uniform() {  // (0, 1)
    const unsigned long long h = splitmix64(key ^ (++ctr * 0x9E3779B97F4A7C15ULL));
    return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0);
  }
  __device__ double normal() {
    const double u1 = uniform(), u2 = uniform();
    return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
  }
  __device__ double gamma(double a) {  // shape a > 0, scale 1
    double boost = 1.0;
    if (a < 1.0) {
      boost = pow(uniform(), 1.0 / a);
      a += 1.0;
    }
    const double d = a - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    for (int it = 0; it < 1000; ++it) {
      const double x = normal(), t = 1.0 + c * x;
      if (t <= 0.0) continue;
      const double vv = t * t * t, u = uniform();
      if (u < 1.0 - 0.0331 * (x * x) * (x * x) || log(u) < 0.5 * x * x + d * (1.0 - vv + log(vv))) return boost * d * vv;
    }
    return boost * d;
  }
  __device__ double poisson(double lam) {
    if (!(lam > 0.0)) return 0.0;
    if (lam < 10.0) {
      const double L = exp(-lam);
      double k = 0.0, p = uniform();
      while (p > L) {
        k += 1.0;
        p *= uniform();
      }
      return k;
    }
    if (lam > 1e15) return lam;  // beyond float64 integer resolution the distribution is its mean
    const double slam = sqrt(lam), loglam = log(lam), b = 0.931 + 2.53 * slam, a = -0.059 + 0.02483 * b;
    const double invalpha = 1.1239 + 1.1328 / (b - 3.4), vr = 0.9277 - 3.6224 / (b - 2.0);
    for (int it = 0; it < 1000; ++it) {
      const double U = uniform() - 0.5, V = uniform(), us = 0.5 - fabs(U);
      const double k = floor((2.0 * a / us + b) * U + lam + 0.43);
      if (us >= 0.07 && V <= vr) return k;
      if (k < 0.0 || (us < 0.013 && V > us)) continue;
      if (log(V) + log(invalpha) - log(a / (us * us) + b) <= -lam + k * loglam - lgamma(k + 1.0)) return k;
    }
    return floor(lam);
  }
  __device__ double binomial(double n, double p);  // DESIGN 9l; defined in the last section of this file
};

template <int LIK>
__device__ __forceinline__ double lik_sample(RowRng& g, const double* f, double param) {
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    return f[0] + param * g.normal();
  } else if (LIK == HMOGP_LIK_BERNOULLI) {
    const double ef = safe_exp(f[0]);
    return g.uniform() < clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9) ? 1.0 : 0.0;
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    return f[0] + sqrt(safe_exp(f[1])) * g.normal();
  } else if (LIK == HMOGP_LIK_POISSON) {
    return g.poisson(safe_exp(f[0]));
  } else if (LIK == HMOGP_LIK_EXPONENTIAL) {
    return -clip(safe_exp(-f[0]), 1e-9, 1e9) * log(g.uniform());
  } else if (LIK == HMOGP_LIK_GAMMA) {
    const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
    return g.gamma(a) / b;
  } else if (LIK == HMOGP_LIK_BETA) {
    const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
    const double x = g.gamma(a), yv = g.gamma(b);
    // (both variates underflow where a and b are tiny, from e^f near 7e-3 down: 0 / 0.  The mass sits on 0 and 1 there, 1 with probability
    // a / (a + b), the limit of the law -- as in the Beta-Binomial and Dirichlet draws below)
    return x + yv > 0.0 ? x / (x + yv) : (g.uniform() * (a + b) < a ? 1.0 : 0.0);
  } else if (LIK == HMOGP_LIK_STUDENT) {  // location + scale * t(nu):  z / sqrt(chi2_nu / nu),  chi2_nu = 2 Gamma(nu/2, 1)
    const double z = g.normal(), G = g.gamma(0.5 * param);
    return f[0] + safe_exp(0.5 * f[1]) * z * sqrt(param / (2.0 * G));
  } else if (LIK == HMOGP_LIK_NEGBINOMIAL) {  // Gamma-Poisson mixture: lambda = mu Gamma(r, 1) / r, y ~ Poisson(lambda)
    const double r = clip(safe_exp(f[1]), 1e-9, 1e9);
    return g.poisson(safe_exp(f[0]) * g.gamma(r) / r);
  } else if (LIK == HMOGP_LIK_WEIBULL) {  // inversion of the survival function: an event time, never censored
    return safe_exp(f[0]) * pow(-log(g.uniform()), 1.0 / weibull_shape(f[1]));
  } else if (LIK == HMOGP_LIK_BINOMIAL) {  // param = the trial count n* (0: 1)
    const double ef = safe_exp(f[0]);
    return g.binomial(param > 0.0 ? param : 1.0, clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9));
  } else if (LIK == HMOGP_LIK_BETABINOMIAL) {  // Beta's own draw p = Gamma_a / (Gamma_a + Gamma_b), then Binomial(n*, p)
    const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
    const double x = g.gamma(a), yv = g.gamma(b);
    // (both variates underflow where a and b are tiny: the mass sits on p = 0 and p = 1, p = 1 with probability a / (a + b))
    const double p = x + yv > 0.0 ? x / (x + yv) : (g.uniform() * (a + b) < a ? 1.0 : 0.0);
    return g.binomial(param > 0.0 ? param : 1.0, p);
  } else if (LIK == HMOGP_LIK_ZIPOISSON) {  // a structural zero with probability pi, else a Poisson count
    const double ef = safe_exp(f[1]);
    return g.uniform() < clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9) ? 0.0 : g.poisson(safe_exp(f[0]));
  } else {  // Categorical: labels 1..K, probabilities clipped then renormalised (categorical.py:66-71)
    const int K = (int)param, D = K - 1;
    double e[HMOGP_MAXJ], esum = 0.0;
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k) {
      e[k] = (k < D) ? safe_exp(f[k]) : 0.0;
      esum += e[k];
    }
    const double den = 1.0 + esum;
    double psum = clip(1.0 / den, 1e-9, 1.0 - 1e-9);
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k)
      if (k < D) {
        e[k] = clip(e[k] / den, 1e-9, 1.0 - 1e-9);
        psum += e[k];
      }
    const double u = g.uniform() * psum;
    double cum = 0.0, label = (double)K;
    bool found = false;
#pragma unroll
    for (int k = 0; k < HMOGP_MAXJ; ++k)
      if (k < D && !found) {
        cum += e[k];
        if (u < cum) label = (double)(k + 1), found = true;
      }
    return label;
  }
}

// Ordinal: y = 1 + #{k : f + sigma eps > b_k}, eps ~ N(0, 1)
__device__ __forceinline__ double lik_ordinal_sample(RowRng& g, const OrdinalTable& tb, double f) {
  const double z = f + tb.sigma * g.normal();
  int label = 1;
  for (int k = 0; k < tb.K - 1; ++k) label += (z > tb.edge[k]) ? 1 : 0;
  return (double)label;
}

// Dirichlet: K Gamma(a_k, 1) variates, normalised.  Where every variate underflows to zero (all a_k tiny: the mass sits on the
// vertices) the draw is the vertex k with probability a_k / A, the limit of the distribution.
template <int K>
__device__ __forceinline__ void lik_dirichlet_sample(RowRng& g, const double* f, double* y) {
  double a[K], x[K], A = 0.0, s = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    a[k] = clip(safe_exp(f[k]), 1e-9, 1e9);
    x[k] = g.gamma(a[k]);
    A += a[k];
    s += x[k];
  }
  if (s > 0.0) {
#pragma unroll
    for (int k = 0; k < K; ++k) y[k] = x[k] / s;
    return;
  }
  const double u = g.uniform() * A;
  double cum = 0.0;
  bool found = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    cum += a[k];
    const bool hit = !found && (u < cum || k == K - 1);
    y[k] = hit ? 1.0 : 0.0;
    found = found || hit;
  }
}

// Dispatch.  For 64-lane likelihoods every lane of the wave must call with the same row; the result is valid in
// every lane.  `etab` (per-wave LDS, HMOGP_ETAB doubles) is used by the one-wave-per-row likelihoods.
// CATD: number of functions (K-1) of a Categorical likelihood -- a template parameter so that each K gets its own register
// allocation (0 for every other likelihood).
template <int LIK, int CATD = 0>
__device__ __forceinline__ void lik_eval(double y, double yaux, const double* m, const double* v, double param, int lane,
                                         double* etab, unsigned quirks, LikOut& o) {
  if (LIK == HMOGP_LIK_GAUSSIAN)
    lik_gaussian(y, m[0], v[0], param, o);
  else if (LIK == HMOGP_LIK_HETGAUSSIAN)
    lik_hetgaussian(y, m, v, o);
  else if (LIK == HMOGP_LIK_BERNOULLI || LIK == HMOGP_LIK_POISSON || LIK == HMOGP_LIK_EXPONENTIAL)
    lik_quad1d<LIK>(y, yaux, m[0], v[0], o);
  else if (LIK == HMOGP_LIK_GAMMA)
    lik_gamma(y, m, v, o);
  else if (LIK == HMOGP_LIK_BETA)
    lik_beta_wave(y, m, v, lane, etab, o);
  else if (LIK == HMOGP_LIK_STUDENT)
    lik_student_wave(y, m, v, param, lane, etab, o);
  else if (LIK == HMOGP_LIK_ORDINAL)
    lik_ordinal(y, yaux, m[0], v[0], param, o);   // y / yaux: the row's lower / upper cut point, param: sigma
  else if (LIK == HMOGP_LIK_NEGBINOMIAL)
    lik_negbinomial_wave(y, yaux, m, v, lane, etab, o);   // yaux: lgamma(y + 1)
  else if (LIK == HMOGP_LIK_WEIBULL)
    lik_weibull_wave(y, yaux, m, v, lane, etab, o);   // y: log of the time, yaux: delta
  else if (LIK == HMOGP_LIK_BINOMIAL)
    lik_binomial_quad(y, param, yaux, m[0], v[0], o);   // y: k, param: the row's own trial count n, yaux: lc
  else if (LIK == HMOGP_LIK_BETABINOMIAL)
    lik_betabinomial_wave(y, param, yaux, m, v, lane, etab, o);
  else if (LIK == HMOGP_LIK_ZIPOISSON)
    lik_zipoisson_wave(y, yaux, m, v, lane, etab, o);   // yaux: lgamma(y + 1)
  else
    lik_categorical_t<(CATD > 0 ? CATD : 1)>(y, m, v, lane, etab, quirks, o);
  if ((LIK == HMOGP_LIK_GAMMA || LIK == HMOGP_LIK_BETA) && !(quirks & HMOGP_QUIRK_GAMMA_BETA_PI)) {
    o.ve *= M_PI;  // exact mode: undo the second division of each dimension's weights by sqrt(pi) (quirk Q1)
#pragma unroll
    for (int j = 0; j < 2; ++j) o.gm[j] *= M_PI, o.gv[j] *= M_PI;
  }
}

// ============================================================================ derivatives with respect to the likelihoods' own parameters
// DESIGN 9e.  What a Gaussian (sigma), a Student (nu) and an Ordinal (its cut points and sigma) likelihood can learn: the derivative of
// the row's variational expectation -- of exactly the finite rule above -- with respect to that parameter.  Nothing above this line
// changes: the quadrature kernels keep their code and registers.

// Gaussian: ve = -log(2 pi)/2 - log sigma - ((y - m)^2 + v) / (2 sigma^2)
__device__ __forceinline__ double lik_gaussian_dsigma(double y, double m, double v, double sigma) {
  const double r = y - m;
  return -1.0 / sigma + (r * r + v) / (sigma * sigma * sigma);
}

// C'(nu) of the Student constant C(nu) = lgamma((nu+1)/2) - lgamma(nu/2) - log(nu pi)/2:
//   C'(nu) = psi((nu+1)/2)/2 - psi(nu/2)/2 - 1/(2 nu)
// is O(nu^-2) while its terms are O(log nu): from nu = 64 on it is the derivative of student_logc's series in x = nu/2 (two more
// terms than student_logc keeps: the truncation error has to stay below the rounding of a result that is itself ~1e-4),
//   dC/dx = 1/(8x^2) - 1/(64x^4) + 1/(128x^6) - 17/(2048x^8) + 31/(2048x^10) - 691/(16384x^12),    C'(nu) = dC/dx / 2.
__device__ __forceinline__ double student_dlogc(double nu) {
  if (nu < 64.0) return 0.5 * digamma_pos(0.5 * (nu + 1.0)) - 0.5 * digamma_pos(0.5 * nu) - 0.5 / nu;
  const double ix = 2.0 / nu, z = ix * ix;
  return 0.5 * z *
         (1.0 / 8.0 + z * (-1.0 / 64.0 + z * (1.0 / 128.0 + z * (-17.0 / 2048.0 + z * (31.0 / 2048.0 + z * (-691.0 / 16384.0))))));
}

// Student, 20 x 20 rule, one wave per row, nodes strided over the lanes as in lik_student_wave (same node tables in the wave's LDS slice):
//   d ve / d nu = C'(nu) + sum_ij w_i w_j [ -log1p(u)/2 + (nu+1)/(2 nu) u/(1+u) ],     u = r^2 s / nu
__device__ __forceinline__ double lik_student_dnu_wave(double y, const double* m, const double* v, double nu, int lane, double* tab) {
  if (lane < 40) {
    const int dim = lane / 20, i = lane - 20 * dim;
    const double f = GH20_X[i] * sqrt(2.0 * v[dim]) + m[dim];
    if (dim == 0)
      tab[i] = y - f;
    else
      tab[40 + i] = safe_exp(-f);
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  const double rnu = 1.0 / nu, kn = 0.5 * (nu + 1.0) * rnu;
  double acc = 0.0;
  for (int n = lane; n < 400; n += 64) {
    const int i = n / 20, j = n - 20 * i;
    const double w = GH20_WN[i] * GH20_WN[j];
    const double r = tab[i], s = tab[40 + j];
    const double u = r * r * s * rnu;
    acc += w * (kn * (u / (1.0 + u)) - 0.5 * log1p(u));
  }
  return student_dlogc(nu) + wave_sum(acc);
}

// Ordinal: the sibling of ordinal_node for the parameters.  With P = Phi(b) - Phi(a) it returns qa = phi(a) / P, qb = phi(b) / P and
// h = (a phi(a) - b phi(b)) / P, from which
//   d lp / d lo = -qa / sigma,    d lp / d hi = qb / sigma,    d lp / d sigma = h / sigma.
// Same three branches as ordinal_node (the mirror step swaps the two ratios; h is even under it):
//   branch             qa                               qb
//   P = 1 - Q          phi(a) / (1 - Q)                 phi(b) / (1 - Q)
//   erfcx              sqrt(2/pi) exp(-d) / D           sqrt(2/pi) / D
// exp(-d) = 1 + expm1(-d) is evaluated as an exponential of its own: beyond d = 37 the sum 1 + expm1(-d) is 0 in float64, while
// d/d lo of a bin far from f IS exp(-d) times a number of order 1 and has nothing to hide a lost factor behind (h has: its -b).
// An infinite cut contributes 0 (phi = 0; exp(-d) = 0).
__device__ __forceinline__ void ordinal_node_dparam(double a, double b, double& qa, double& qb, double& h) {
  bool mir = false;
  if (a + b > 0.0) {
    const double t = a;
    a = -b, b = -t, mir = true;
  }
  double ra, rb;
  bool done = false;
  if (b > 0.0) {
    const double Q = 0.5 * (erfc(-a * M_SQRT1_2) + erfc(b * M_SQRT1_2));
    if (Q < 0.5) {
      const double rP = 1.0 / (1.0 - Q);
      const double pa = ORD_INV_SQRT_2PI * exp(-0.5 * a * a), pb = ORD_INV_SQRT_2PI * exp(-0.5 * b * b);
      ra = pa * rP, rb = pb * rP;
      h = ((isinf(a) ? 0.0 : a * pa) - (isinf(b) ? 0.0 : b * pb)) * rP;
      done = true;
    }
  }
  if (!done) {
    const double Ea = erfcx(-a * M_SQRT1_2), Eb = erfcx(-b * M_SQRT1_2);  // a = -inf: E = 0
    const double x = 0.5 * (b - a) * (a + b);                              // -d
    const double em = expm1(x), ed = exp(x);                               // a = -inf: expm1 = -1, exp = 0
    const double D = (Eb - Ea) - em * Ea;
    const double rD = ORD_SQRT_2_OVER_PI / D;
    ra = ed * rD, rb = rD;
    h = ((isinf(a) ? 0.0 : a * ed) - b) * rD;
  }
  qa = mir ? rb : ra;
  qb = mir ? ra : rb;
}

// 20-node rule, one lane per row: the derivatives of lik_ordinal's ve with respect to the row's own two cut points and to sigma
__device__ __forceinline__ void lik_ordinal_dparam(double lo, double hi, double m, double v, double sigma, double& dlo, double& dhi,
                                                   double& dsig) {
  const double s = sqrt(2.0 * v);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 1
  for (int i = 0; i < 20; ++i) {
    const double f = GH20_X[i] * s + m, w = GH20_WN[i];
    double qa, qb, h;
    ordinal_node_dparam((lo - f) / sigma, (hi - f) / sigma, qa, qb, h);
    a0 += qa * w;
    a1 += qb * w;
    a2 += h * w;
  }
  dlo = -a0 / sigma;
  dhi = a1 / sigma;
  dsig = a2 / sigma;
}

// ============================================================================ deterministic log predictive density
// log p(y|f) at one node of the rule for the two families lik_logpdf_sample has no branch for (the reference defines no log_predictive for
// them).  The families' own links and clips, a = clip(safe_exp(f0), 1e-9, 1e9), b likewise; no division by pi (Q1 is a quirk of the
// reference's var_exp).  Appended, like DESIGN 9e's functions above, so that nothing in front changes.
__device__ __forceinline__ double lik_gamma_logpdf(double y, const double* f) {
  const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
  return -lgamma(a) + a * log(b) + (a - 1.0) * log(y) - b * y;
}
__device__ __forceinline__ double lik_beta_logpdf(double y, const double* f) {
  const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
  return (a - 1.0) * log(y) + (b - 1.0) * log(1.0 - y) - (lgamma(a) + lgamma(b) - lgamma(a + b));
}

// ============================================================================ predictive cdf / survival function
// The conditional pair C = P(Y <= y | f), S = P(Y > y | f) at one node of the rule, for the six families whose pair is closed-form in exp,
// expm1, log and erfc.  Each is evaluated directly, never as 1 - the other: a tail of 1e-200 keeps its relative precision.  Links and clips
// are those of lik_logpdf_sample<LIK> / lik_weibull_logpdf.  What the arguments mean per family:
//   Gaussian      z = (y - f0) / param                           param: the standard deviation (sqrt(sigma^2 + v) folds q(f) in exactly)
//   HetGaussian   z = (y - f0) / sqrt(yaux + safe_exp(f1))       yaux: the variance of f0 integrated out analytically (0: the plain conditional)
//   Ordinal       z = (yaux - f0) / param                        yaux: the label's UPPER cut point (+inf for class K), param as Gaussian's
//                 C = erfc(-z / sqrt 2) / 2,  S = erfc(z / sqrt 2) / 2
//   Bernoulli     p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9):  (0, 1) for y < 0, (1 - p, p) for 0 <= y < 1, (1, 0) for y >= 1
//   Exponential   b = clip(safe_exp(-f0), 1e-9, 1e9):  (0, 1) for y <= 0, else S = exp(-y / b), C = -expm1(-y / b)
//   Weibull       y is log(time) (-inf: time <= 0 -> (0, 1)), k = weibull_shape(f1), z = min(k (y - f0), HMOGP_WEIBULL_ZMAX), e = exp(z),
//                 S = exp(-e), C = -expm1(-e)
// Appended, like the sections above, so that nothing in front changes.
__device__ __forceinline__ void phi_cdf_sf(double z, double& C, double& S) {
  C = 0.5 * erfc(-z * M_SQRT1_2);
  S = 0.5 * erfc(z * M_SQRT1_2);
}
template <int LIK>
__device__ __forceinline__ void lik_cdf_sf(double y, double yaux, const double* f, double param, double& C, double& S) {
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    phi_cdf_sf((y - f[0]) / param, C, S);
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    phi_cdf_sf((y - f[0]) / sqrt(yaux + safe_exp(f[1])), C, S);
  } else if (LIK == HMOGP_LIK_ORDINAL) {
    phi_cdf_sf((yaux - f[0]) / param, C, S);
  } else if (LIK == HMOGP_LIK_BERNOULLI) {
    const double ef = safe_exp(f[0]);
    const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
    C = y < 0.0 ? 0.0 : (y < 1.0 ? 1.0 - p : 1.0);
    S = y < 0.0 ? 1.0 : (y < 1.0 ? p : 0.0);
    if (y != y) C = S = y;
  } else if (LIK == HMOGP_LIK_EXPONENTIAL) {
    const double b = clip(safe_exp(-f[0]), 1e-9, 1e9);
    const double a = -(y / b);
    C = y <= 0.0 ? 0.0 : -expm1(a);
    S = y <= 0.0 ? 1.0 : exp(a);
  } else if (LIK == HMOGP_LIK_WEIBULL) {
    const double k = weibull_shape(f[1]);
    const double e = exp(fmin(k * (y - f[0]), HMOGP_WEIBULL_ZMAX));
    C = y == -INFINITY ? 0.0 : -expm1(-e);
    S = y == -INFINITY ? 1.0 : exp(-e);
  } else {
    C = S = nan("");
  }
}

// ============================================================================ Binomial and Beta-Binomial
// k successes out of n trials, n the row's own: Y is (k, n) per row, both integer-valued doubles with 1 <= n <= 1e9, 0 <= k <= n (checked
// on the host), and lc = lgamma(n+1) - lgamma(k+1) - lgamma(n-k+1) is formed once per row on the host, as gammaln(y+1) is for Poisson.
// The dispatchers above hand the row over as (y, param, yaux) = (k, n, lc): the task's lik_param is the trial count n* of `predictive` and
// `sample` only (no y reaches them) and is ignored wherever y carries n.  Appended, like the sections above, so that nothing in front changes.
__device__ __forceinline__ double lik_pred_trials(double param) { return param > 0.0 ? param : 1.0; }   // 0.0 means 1 (checked on the host)

// ---- Binomial, T = 20, one lane per row.  Bernoulli's link and clip, p = clip(e^f / (1 + e^f), 1e-9, 1 - 1e-9), and its expression shapes:
//   lp = lc + k log p + (n - k) log(1 - p)      d1 = ((k - n p) / (1 - p)) (1 / (1 + e^f))      d2 = -(n p) / (1 + e^f)
// so that a row (k, n) is n Bernoulli rows collapsed into one, and at n = 1 (lc = 0, k and n - k one of them 0 and the other 1: every product
// with them is exact) each operation is lik_quad1d<BERNOULLI>'s on the same operands.  A loop of its own: the three instantiations of
// lik_quad1d keep their code.
__device__ __forceinline__ void lik_binomial_quad(double k, double n, double lc, double m, double v, LikOut& o) {
  const double s = sqrt(2.0 * v), nk = n - k;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 4
  for (int i = 0; i < 20; ++i) {
    const double f = GH20_X[i] * s + m, w = GH20_WN[i];
    const double ef = safe_exp(f);
    const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
    const double lp = (k * log(p) + nk * log(1.0 - p)) + lc;
    const double d1 = ((k - n * p) / (1.0 - p)) * (1.0 / (1.0 + ef));
    const double d2 = -(n * p) / (1.0 + ef);
    a0 += lp * w;
    a1 += d1 * w;
    a2 += d2 * w;
  }
  o.ve = a0;
  o.gm[0] = a1;
  o.gv[0] = 0.5 * a2;
}

// The full log p at one f (Monte-Carlo and deterministic log predictive)
__device__ __forceinline__ double lik_binomial_logpdf(double k, double n, double lc, const double* f) {
  const double ef = safe_exp(f[0]);
  const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
  return (k * log(p) + (n - k) * log(1.0 - p)) + lc;
}

// mean = n* E[p],  var = n* E[p (1 - p)] + n*^2 (E[p^2] - E[p]^2) over the T nodes.  The second term is the variance of p under the rule,
// formed in a second pass as sum w (p - E[p])^2: as a difference of two numbers of order one it would carry n*^2 eps, n* eps of the result.
__device__ __forceinline__ void lik_binomial_predictive(double m, double v, double param, int T, double& mean, double& var) {
  const double s = sqrt(2.0 * v), nt = lik_pred_trials(param);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (int i = 0; i < T; ++i) {
    const double ef = safe_exp(gh_x(T, i) * s + m), w = gh_wn(T, i);
    const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
    a0 += p * w;
    a1 += p * (1.0 - p) * w;
  }
  for (int i = 0; i < T; ++i) {
    const double ef = safe_exp(gh_x(T, i) * s + m), w = gh_wn(T, i);
    const double d = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9) - a0;
    a2 += d * d * w;
  }
  mean = nt * a0;
  var = nt * a1 + nt * nt * a2;
}

// ---- Beta-Binomial, 20 x 20, one wave per row.  Beta's links and clips, a = clip(safe_exp(f0), 1e-9, 1e9), b likewise, s = a + b.  With
// G(y, r) = lgamma(y+r) - lgamma(r), D1 = psi(y+r) - psi(r), D2 = psi'(y+r) - psi'(r) -- nb_gamma_diffs' three regimes, never the plain
// difference of two large numbers (s <= 2e9: the y <= 32 product stays below 1e298) --
//   log p    = lc + G(k, a) + G(n-k, b) - G(n, s)
//   d/df0    = a [D1(k, a) - D1(n, s)]           d2/df0^2 = d/df0 + a^2 [D2(k, a) - D2(n, s)]
//   d/df1    = b [D1(n-k, b) - D1(n, s)]         d2/df1^2 = d/df1 + b^2 [D2(n-k, b) - D2(n, s)]      (the clips are ignored, as for Beta)
// Only the three functions of s couple the dimensions (alpha = exp f keeps the tables separable; a mean / precision pair would not): lanes
// 0-19 write a_i, G(k, a_i), a_i D1(k, a_i), a_i^2 D2(k, a_i) into the wave's LDS slice, lanes 20-39 the same four for b_j with n - k.
// Each of the 400 nodes then costs one nb_gamma_diffs(n, a_i + b_j); n is the same in the whole wave, so its y <= 32 loop does not
// diverge, and beyond it the r >= 16 / r < 16 branch is taken per lane, both sides bounded.
__device__ __forceinline__ void lik_betabinomial_wave(double k, double n, double lc, const double* m, const double* v, int lane,
                                                      double* tab, LikOut& o) {
  static_assert(160 <= HMOGP_ETAB, "Beta-Binomial table");
  if (lane < 40) {
    const int dim = lane / 20, i = lane - 20 * dim;
    const double x = clip(safe_exp(GH20_X[i] * sqrt(2.0 * (dim == 0 ? v[0] : v[1])) + (dim == 0 ? m[0] : m[1])), 1e-9, 1e9);
    double G, D1, D2;
    nb_gamma_diffs(dim == 0 ? k : n - k, x, G, D1, D2);
    double* t = tab + 80 * dim + i;
    t[0] = x, t[20] = G, t[40] = x * D1, t[60] = x * x * D2;
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int nd = lane; nd < 400; nd += 64) {
    const int i = nd / 20, j = nd - 20 * i;
    const double w = GH20_WN[i] * GH20_WN[j];
    const double a = tab[i], b = tab[80 + j];
    double G, D1, D2;
    nb_gamma_diffs(n, a + b, G, D1, D2);
    const double d0 = tab[40 + i] - a * D1, d1 = tab[120 + j] - b * D1;
    ve += w * (lc + tab[20 + i] + tab[100 + j] - G);
    g0 += w * d0;
    g1 += w * d1;
    h0 += w * (d0 + (tab[60 + i] - a * a * D2));
    h1 += w * (d1 + (tab[140 + j] - b * b * D2));
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

__device__ __forceinline__ double lik_betabinomial_logpdf(double k, double n, double lc, const double* f) {
  const double a = clip(safe_exp(f[0]), 1e-9, 1e9), b = clip(safe_exp(f[1]), 1e-9, 1e9);
  return lc + nb_lgamma_diff(k, a) + nb_lgamma_diff(n - k, b) - nb_lgamma_diff(n, a + b);
}

// With mu = a / s over the T x T nodes (one lane per row; b_j is formed again per node rather than kept in an indexed array):
//   mean = n* E[mu],  var = n* E[mu (1 - mu) (s + n*) / (s + 1)] + n*^2 (E[mu^2] - E[mu]^2),   the last term in a second pass, as above
__device__ __forceinline__ void lik_betabinomial_predictive(const double* m, const double* v, double param, int T, double& mean,
                                                            double& var) {
  const double s0 = sqrt(2.0 * v[0]), s1 = sqrt(2.0 * v[1]), nt = lik_pred_trials(param);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const double e1 = a0;   // (complete in the second pass)
    for (int i = 0; i < T; ++i) {
      const double a = clip(safe_exp(gh_x(T, i) * s0 + m[0]), 1e-9, 1e9), wi = gh_wn(T, i);
#pragma unroll 1
      for (int j = 0; j < T; ++j) {
        const double b = clip(safe_exp(gh_x(T, j) * s1 + m[1]), 1e-9, 1e9), w = wi * gh_wn(T, j);
        const double s = a + b, mu = a / s;
        if (pass == 0) {
          a0 += w * mu;
          a1 += w * (mu * (b / s) * ((s + nt) / (s + 1.0)));
        } else {
          a2 += w * ((mu - e1) * (mu - e1));
        }
      }
    }
  }
  mean = nt * a0;
  var = nt * a1 + nt * nt * a2;
}

// ---- Binomial(n, p) variates.  Every loop is bounded at compile time.  The draw is made for q = min(p, 1 - p) and reflected.
//   n q < 10    sequential inversion from 0 with P(0) = (1 - q)^n, P(j + 1) = P(j) (n - j) / (j + 1) q / (1 - q): at most 256 trips (the mass
//               beyond them is below 1e-150 at a mean below 10); at exhaustion the trip count is the draw
//   otherwise   Hoermann's BTRS transformed rejection (1993), at most 1000 trials, then floor(n q): the shape of the Poisson PTRS loop above
__device__ inline double RowRng::binomial(double n, double p) {
  if (!(p > 0.0)) return 0.0;
  if (!(p < 1.0)) return n;
  const bool flip = p > 0.5;
  const double q = flip ? 1.0 - p : p;
  double k = 0.0;
  if (n * q < 10.0) {
    const double r = q / (1.0 - q);
    double pk = exp(n * log1p(-q)), u = uniform();
    for (int it = 0; it < 256; ++it) {
      if (u <= pk || k >= n) break;
      u -= pk;
      pk *= r * ((n - k) / (k + 1.0));
      k += 1.0;
    }
  } else {
    const double spq = sqrt(n * q * (1.0 - q)), b = 1.15 + 2.53 * spq, a = -0.0873 + 0.0248 * b + 0.01 * q, c = n * q + 0.5;
    const double vr = 0.92 - 4.2 / b, alpha = (2.83 + 5.1 / b) * spq, lr = log(q / (1.0 - q)), md = floor((n + 1.0) * q);
    const double h = lgamma(md + 1.0) + lgamma(n - md + 1.0);
    k = floor(n * q);
    for (int it = 0; it < 1000; ++it) {
      const double U = uniform() - 0.5, V = uniform(), us = 0.5 - fabs(U);
      const double kk = floor((2.0 * a / us + b) * U + c);
      if (kk < 0.0 || kk > n) continue;
      if ((us >= 0.07 && V <= vr) || log(V * alpha / (a / (us * us) + b)) <= h - lgamma(kk + 1.0) - lgamma(n - kk + 1.0) + (kk - md) * lr) {
        k = kk;
        break;
      }
    }
  }
  return flip ? n - k : k;
}

// ============================================================================ Zero-inflated Poisson
// Counts with more zeros than a rate explains: a structural zero with probability pi, else Poisson(lambda).  f0 = log of the rate,
// lambda = safe_exp(f0) (Poisson's link); f1 = logit of pi = clip(e^f1 / (1 + e^f1), 1e-9, 1 - 1e-9) (Bernoulli's link and clip, in Bernoulli's
// expression shapes).  The clip's own derivative is ignored, as for every clipped family.  Appended so that nothing in front changes.
//   y >= 1   log p = [-lambda + y f0 - lgamma(y+1)] + log(1 - pi): Poisson's log p in f0 plus Bernoulli's log p of the label 0 in f1.  The row
//            is the SUM of two 20-node rules (the weights sum to 1 per dimension): 40 nodes, not 400.
//   y  = 0   log p0 = lpi + softplus(u),  lpi = log pi, l1 = log(1 - pi), u = l1 - lambda - lpi,  rho = sigmoid(u) the Poisson component's
//            share of the zero (rho and 1 - rho from the one exp(-|u|)), t = lambda rho, g = pi (1 - pi) (-expm1(-lambda)) exp(-log p0):
//              d/df0 = -t     d2/df0^2 = -t + (lambda t) (1 - rho)     d/df1 = g     d2/df1^2 = g (rho - pi)
//            In this order no product is inf * 0: once lambda is so large that rho is exactly 0, t is exactly 0 although lambda^2 would
//            overflow.  g is a product of positive factors, never the difference (1 - rho) - pi, which cancels to nothing for small lambda.
// y is the same in the whole wave (one wave per row): the branch on y = 0 does not diverge.
__device__ __forceinline__ double lik_zipoisson_logpdf(double y, double lgy1, const double* f) {
  const double lam = safe_exp(f[0]), ef = safe_exp(f[1]);
  const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
  if (y > 0.0) return (-lam + y * f[0] - lgy1) + log(1.0 - p);
  const double lpi = log(p), u = log(1.0 - p) - lam - lpi;
  return lpi + (fmax(u, 0.0) + log1p(exp(-fabs(u))));
}

__device__ __forceinline__ void lik_zipoisson_wave(double y, double lgy1, const double* m, const double* v, int lane, double* tab, LikOut& o) {
  static_assert(120 <= HMOGP_ETAB, "zero-inflated Poisson table");
  const bool on = lane < 40;   // lanes 0-19: node i of f0, lanes 20-39: node j of f1, lanes 40-63: idle here (index 0, weight 0)
  const int dim = lane >= 20 ? 1 : 0, i = on ? lane - 20 * dim : 0;
  const double f = on ? GH20_X[i] * sqrt(2.0 * (dim == 0 ? v[0] : v[1])) + (dim == 0 ? m[0] : m[1]) : 0.0;
  const double ef = safe_exp(f);
  if (y > 0.0) {
    // lanes 0-19: lik_quad1d<POISSON>'s node i; lanes 20-39: lik_quad1d<BERNOULLI>'s node j at the label 0, both in their expression shapes
    const double w = on ? GH20_WN[i] : 0.0;
    const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
    const double lp = dim == 0 ? -ef + y * f - lgy1 : log(1.0 - p);
    const double d1 = dim == 0 ? -ef + y : ((0.0 - p) / (1.0 - p)) * (1.0 / (1.0 + ef));
    const double d2 = dim == 0 ? -ef : -p / (1.0 + ef);
    const double w0 = dim == 0 ? w : 0.0, w1 = dim == 0 ? 0.0 : w;
    o.ve = wave_sum(lp * w0) + wave_sum(lp * w1);
    o.gm[0] = wave_sum(d1 * w0);
    o.gv[0] = 0.5 * wave_sum(d2 * w0);
    o.gm[1] = wave_sum(d1 * w1);
    o.gv[1] = 0.5 * wave_sum(d2 * w1);
    return;
  }
  if (on) {
    if (dim == 0) {
      tab[i] = ef;
      tab[20 + i] = -expm1(-ef);
    } else {
      const double p = clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9);
      tab[40 + i] = log(p);
      tab[60 + i] = log(1.0 - p);
      tab[80 + i] = p;
      tab[100 + i] = p * (1.0 - p);
    }
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
  double ve = 0.0, g0 = 0.0, g1 = 0.0, h0 = 0.0, h1 = 0.0;
  for (int n = lane; n < 400; n += 64) {
    const int a = n / 20, b = n - 20 * a;
    const double w = GH20_WN[a] * GH20_WN[b];
    const double lam = tab[a], lpi = tab[40 + b], pi = tab[80 + b];
    const double u = tab[60 + b] - lam - lpi;
    const double e = exp(-fabs(u)), inv = 1.0 / (1.0 + e), ei = e * inv;
    const double lp0 = lpi + (fmax(u, 0.0) + log1p(e));
    const double rho = u >= 0.0 ? inv : ei, rhoc = u >= 0.0 ? ei : inv;
    const double t = lam * rho;
    const double g = tab[100 + b] * tab[20 + a] * exp(-lp0);
    ve += w * lp0;
    g0 -= w * t;
    h0 += w * (-t + (lam * t) * rhoc);
    g1 += w * g;
    h1 += w * (g * (rho - pi));
  }
  o.ve = wave_sum(ve);
  o.gm[0] = wave_sum(g0);
  o.gm[1] = wave_sum(g1);
  o.gv[0] = 0.5 * wave_sum(h0);
  o.gv[1] = 0.5 * wave_sum(h1);
}

// With q(f0), q(f1) independent and pbar = E[pi] over the T nodes of f1 (pi's clip kept, every other clip ignored, overflow is +inf):
//   mean = (1 - pbar) exp(m0 + v0/2),   variance = (1 - pbar) (exp(m0 + v0/2) + exp(2 m0 + 2 v0)) - mean^2
// (E[y | f] = (1 - pi) lambda, E[y^2 | f] = (1 - pi) (lambda + lambda^2)).  One lane per row.
__device__ __forceinline__ void lik_zipoisson_predictive(const double* m, const double* v, int T, double& mean, double& var) {
  const double s = sqrt(2.0 * v[1]);
  double pb = 0.0;
  for (int j = 0; j < T; ++j) {
    const double ef = safe_exp(gh_x(T, j) * s + m[1]);
    pb += clip(ef / (1.0 + ef), 1e-9, 1.0 - 1e-9) * gh_wn(T, j);
  }
  const double e1 = exp(m[0] + 0.5 * v[0]), e2 = exp(2.0 * m[0] + 2.0 * v[0]);
  const double e2nd = (1.0 - pb) * (e1 + e2);
  mean = (1.0 - pb) * e1;
  var = e2nd < INFINITY ? e2nd - mean * mean : INFINITY;   // (mean^2 <= e2: finite wherever e2nd is)
}
