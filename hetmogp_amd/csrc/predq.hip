// predq.hip -- predictive cdf, survival function and quantiles per row: for a test row with q(f) = N(m, diag v),
//   cdf(y) = sum_nodes w C(y | f_node),   sf(y) = sum_nodes w S(y | f_node),   quantile(p) = the y with cdf(y) = p,
// over the nodes and normalised weights of logpred.hip's rule.  C and S are lik_cdf_sf<LIK>'s pair, each summed on its own and
// never formed as 1 - the other.  Six families: Gaussian and Ordinal are closed forms (the probit integrates exactly), HetGaussian
// integrates f0 analytically (T nodes over f1), Bernoulli and Exponential take T nodes, Weibull the T x T tensor rule.
// Kernels, the split logpred.hip makes: rules of at most 20 nodes run one lane per row, the node values of the row formed once and kept in
// registers (static indices: the node loops are unrolled over the compile-time T); Weibull runs one wave per row, four rows per block,
// the node tables in the wave's HMOGP_ETAB slice, filled once per row, each lane's share of the T^2 nodes then held in registers.
//
// The quantile solver.  Every loop is bounded at compile time: ONE loop of at most PQ_MAXEVAL trips holds the only call of the rule, and a
// small state machine picks the next abscissa, so a row makes at most PQ_MAXEVAL evaluations whatever its inputs are (budget exhausted:
// NaN).  For p <= 1/2 it solves cdf(x) = p, otherwise sf(x) = 1 - p (exact for p >= 1/2); x is y (Gaussian, HetGaussian) or log y
// (Exponential, Weibull).  From a moment-based first guess the bracket grows by at most PQ_MAXDBL doubling steps (each step cut down to
// twice the Newton step when that is shorter); then safeguarded Newton steps on log G (the derivative is the predictive density, from
// the same nodes), at most PQ_MAXNEWTON of them; a candidate outside the bracket, or none left, is replaced by the midpoint of the
// bracket's ORDERED BIT PATTERNS, which closes any bracket of doubles in at most 64 halvings.  The iterate of the wave kernel is formed
// from wave_sum's results, which are the same bits in all 64 lanes, so its branches do not diverge.
#include "lik_launch.h"
#include "lik_device.h"
#include "lik_dispatch.h"

#define PQ_MAXEVAL 128
#define PQ_MAXDBL 64
#define PQ_MAXNEWTON 24
#define PQ_INV_SQRT_2PI 0.3989422804014327

namespace {

struct PqProbs {
  double p[HMOGP_QUANT_MAXP];
};

// double <-> a signed integer that orders as the doubles do (-0 and +0 share 0)
__device__ __forceinline__ long long pq_ord(double x) {
  const long long b = __double_as_longlong(x);
  return b < 0 ? (long long)(0x8000000000000000ULL - (unsigned long long)b) : b;
}
__device__ __forceinline__ double pq_unord(long long k) {
  return __longlong_as_double(k < 0 ? (long long)(0x8000000000000000ULL - (unsigned long long)k) : k);
}

// z >= 0 with Phi(-z) ~ q for 0 < q <= 1/2: Abramowitz & Stegun 26.2.23, |error| < 4.5e-4 -- a first guess, nothing more
__device__ __forceinline__ double pq_z_guess(double q) {
  const double t = sqrt(-2.0 * log(q));
  return t - (2.515517 + t * (0.802853 + t * 0.010328)) / (1.0 + t * (1.432788 + t * (0.189269 + t * 0.001308)));
}
// log(-log(1 - p)) for the solved tail: q = p (cdf) or 1 - p (sf); the first guess of the log-variable families
__device__ __forceinline__ double pq_loglog(double q, bool use_sf) { return log(use_sf ? -log(q) : -log1p(-q)); }

// The state machine between two evaluations of the rule.  G: the solved tail (cdf or sf) at x, D >= 0: the predictive density at x.
struct PqSolver {
  double x, lo, hi, d, target, result;
  int have, ndbl, nnewton;
  bool use_sf;
  __device__ __forceinline__ void init(double q, bool sf, double x0, double d0) {
    x = x0, lo = hi = x0, d = d0, target = q, result = nan("");
    have = ndbl = nnewton = 0;
    use_sf = sf;
  }
  // true: finished, `result` holds the answer (NaN: no bracket within PQ_MAXDBL steps, or the rule returned NaN)
  __device__ __forceinline__ bool step(double G, double D) {
    if (!(G == G)) return true;
    if (fabs(G - target) <= 8.9e-16 * target) {   // 4 eps backward: inside what the rule itself resolves
      result = x;
      return true;
    }
    const bool right = use_sf ? G > target : G < target;   // the root lies to the right of x
    if (right) lo = x, have |= 1;
    else hi = x, have |= 2;
    const double dx = G * log(G / target) / D;              // Newton on log G: exact for an exponential tail
    const double xn = use_sf ? x + dx : x - dx;
    if (fabs(xn - x) <= 2.3e-16 * fabs(x)) {                // the Newton step no longer moves x by an ulp (false for a NaN step)
      result = x;
      return true;
    }
    if (have != 3) {
      if (ndbl >= PQ_MAXDBL) return true;
      ++ndbl;
      double stp = 2.0 * fabs(xn - x);
      if (!(stp <= d)) stp = d;                             // (also: a NaN or infinite candidate)
      stp = fmax(stp, fmax(fabs(x) * 8.9e-16, d * 0x1p-40));
      x = right ? x + stp : x - stp;
      d *= 2.0;
      return false;
    }
    if ((unsigned long long)pq_ord(hi) - (unsigned long long)pq_ord(lo) <= 1ULL) {   // neighbouring doubles
      result = x;
      return true;
    }
    if (nnewton < PQ_MAXNEWTON && xn > lo && xn < hi) {
      ++nnewton;
      x = xn;
      return false;
    }
    const long long ol = pq_ord(lo);
    x = pq_unord(ol + (long long)(((unsigned long long)pq_ord(hi) - (unsigned long long)ol) >> 1));
    return false;
  }
};

__device__ __forceinline__ bool pq_valid_p(double p) { return p > 0.0 && p < 1.0; }

// ---- rules of at most 20 nodes: one lane per row ----------------------------------------------------------------------------------
// Node values the solver keeps (nv[T]): HetGaussian sd_j = sqrt(v0 + safe_exp(f1_j)), Exponential b_j = clip(safe_exp(-f_j));
// Gaussian none (closed form).  One evaluation at x: G = the solved tail, D = the density in x.
template <int LIK, int T>
__device__ __forceinline__ void pq_lane_eval(double x, double m0, double s, const double (&nv)[T], bool use_sf, double& G, double& D) {
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    const double z = (x - m0) / s;
    G = 0.5 * erfc((use_sf ? z : -z) * M_SQRT1_2);
    D = PQ_INV_SQRT_2PI * exp(-0.5 * z * z) / s;
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    double g = 0.0, dd = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const double z = (x - m0) / nv[j], w = gh_wn(T, j);
      g += w * (0.5 * erfc((use_sf ? z : -z) * M_SQRT1_2));
      dd += w * (PQ_INV_SQRT_2PI * exp(-0.5 * z * z) / nv[j]);
    }
    G = g, D = dd;
  } else {  // Exponential, x = log y
    const double y = exp(x);
    double g = 0.0, dd = 0.0;
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const double a = y / nv[j], w = gh_wn(T, j), ea = exp(-a);
      g += w * (use_sf ? ea : -expm1(-a));
      dd += w * (a * ea);
    }
    G = g, D = dd;
  }
}

// y: [N]; Ordinal [2][ldy], the label's upper cut point in row 1; m, v: row n at m[n * ldf] (the task's columns of a wider q(f) array)
template <int LIK>
__global__ __launch_bounds__(256) void pcdf_lane_kernel(double param, int T, long long N, const double* __restrict__ y, long long ldy,
                                                        const double* __restrict__ m, const double* __restrict__ v, int ldf, int absv,
                                                        double* __restrict__ cdf, double* __restrict__ sf) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double yy = y[n];
  const double m0 = m[n * ldf];
  double v0 = v[n * ldf];
  if (absv) v0 = fabs(v0);
  double C = 0.0, S = 0.0;
  if (LIK == HMOGP_LIK_GAUSSIAN || LIK == HMOGP_LIK_ORDINAL) {
    lik_cdf_sf<LIK>(yy, LIK == HMOGP_LIK_ORDINAL ? y[ldy + n] : 0.0, &m0, sqrt(param * param + v0), C, S);
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    const double m1 = m[n * ldf + 1];
    double v1 = v[n * ldf + 1];
    if (absv) v1 = fabs(v1);
    const double s = sqrt(2.0 * v1);
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const double f[2] = {m0, gh_x(T, i) * s + m1};
      double c1, s1;
      lik_cdf_sf<LIK>(yy, v0, f, param, c1, s1);
      C += gh_wn(T, i) * c1, S += gh_wn(T, i) * s1;
    }
  } else {
    const double s = sqrt(2.0 * v0);
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const double f = gh_x(T, i) * s + m0;
      double c1, s1;
      lik_cdf_sf<LIK>(yy, 0.0, &f, param, c1, s1);
      C += gh_wn(T, i) * c1, S += gh_wn(T, i) * s1;
    }
  }
  if (cdf) cdf[n] = C;
  if (sf) sf[n] = S;
}

// q: [N][nP].  Bernoulli and Ordinal return the smallest point of the support whose cdf is >= p; the others run the solver.
template <int LIK, int T>
__global__ __launch_bounds__(256) void pquant_lane_kernel(double param, OrdinalTable tb, long long N, int nP, PqProbs pr,
                                                          const double* __restrict__ m, const double* __restrict__ v, int ldf, int absv,
                                                          double* __restrict__ q) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const double m0 = m[n * ldf];
  double v0 = v[n * ldf];
  if (absv) v0 = fabs(v0);
  double* qn = q + n * nP;
  if (LIK == HMOGP_LIK_BERNOULLI) {
    const double s = sqrt(2.0 * v0);
    double p0 = 0.0;
#pragma unroll 1
    for (int i = 0; i < T; ++i) {
      const double f = gh_x(T, i) * s + m0;
      double c1, s1;
      lik_cdf_sf<LIK>(0.0, 0.0, &f, param, c1, s1);
      p0 += gh_wn(T, i) * c1;
    }
    for (int ip = 0; ip < nP; ++ip) {
      const double p = pr.p[ip];
      qn[ip] = (pq_valid_p(p) && p0 == p0) ? (p0 >= p ? 0.0 : 1.0) : nan("");
    }
    return;
  }
  if (LIK == HMOGP_LIK_ORDINAL) {
    const double sd = sqrt(param * param + v0);
    for (int ip = 0; ip < nP; ++ip) {
      const double p = pr.p[ip];
      double lab = (double)tb.K;
      for (int k = tb.K - 2; k >= 0; --k) {
        double c1, s1;
        lik_cdf_sf<LIK>(0.0, tb.edge[k], &m0, sd, c1, s1);
        if (c1 >= p) lab = (double)(k + 1);
      }
      qn[ip] = (pq_valid_p(p) && m0 == m0 && sd == sd) ? lab : nan("");
    }
    return;
  }
  // Gaussian, HetGaussian, Exponential: the solver
  double nv[T];
  double s, x0s;   // s: the scale of the first guess and of the first bracket step
  if (LIK == HMOGP_LIK_GAUSSIAN) {
    s = sqrt(param * param + v0);
#pragma unroll
    for (int j = 0; j < T; ++j) nv[j] = 0.0;
  } else if (LIK == HMOGP_LIK_HETGAUSSIAN) {
    const double m1 = m[n * ldf + 1];
    double v1 = v[n * ldf + 1];
    if (absv) v1 = fabs(v1);
    const double s1 = sqrt(2.0 * v1);
#pragma unroll
    for (int j = 0; j < T; ++j) nv[j] = sqrt(v0 + safe_exp(gh_x(T, j) * s1 + m1));
    s = sqrt(v0 + safe_exp(m1 + 0.5 * v1));   // the predictive variance: E[exp f1] = exp(m1 + v1 / 2)
  } else {
    const double s1 = sqrt(2.0 * v0);
#pragma unroll
    for (int j = 0; j < T; ++j) nv[j] = clip(safe_exp(-(gh_x(T, j) * s1 + m0)), 1e-9, 1e9);
    s = 1.0 + s1;
  }
  x0s = s;
  for (int ip = 0; ip < nP; ++ip) {
    const double p = pr.p[ip];
    if (!pq_valid_p(p)) {
      qn[ip] = nan("");
      continue;
    }
    const bool use_sf = p > 0.5;
    const double tq = use_sf ? 1.0 - p : p;
    double x0;
    if (LIK == HMOGP_LIK_EXPONENTIAL) x0 = clip(-m0, -20.72326583694641, 20.72326583694641) + pq_loglog(tq, use_sf);
    else x0 = use_sf ? m0 + pq_z_guess(tq) * x0s : m0 - pq_z_guess(tq) * x0s;
    PqSolver sv;
    sv.init(tq, use_sf, x0, s);
#pragma unroll 1
    for (int ev = 0; ev < PQ_MAXEVAL; ++ev) {
      double G, D;
      pq_lane_eval<LIK, T>(sv.x, m0, s, nv, use_sf, G, D);
      if (sv.step(G, D)) break;
    }
    qn[ip] = LIK == HMOGP_LIK_EXPONENTIAL ? exp(sv.result) : sv.result;
  }
}

// ---- Weibull: one wave per row, four rows per block ---------------------------------------------------------------------------------
// The wave's table: [0, T) f0(node i), [20, 20 + T) k_j = weibull_shape(f1(node j)).  Lane l owns the nodes l, l + 64, .. of the T^2
// (i = node / T, j = node % T, weight w_i w_j); a slot past the end carries weight 0.
template <int T>
struct WbNodes {
  static constexpr int U = (T * T + 63) / 64;
  double f0[U], k[U], w[U];
};
template <int T>
__device__ __forceinline__ void wb_fill(WbNodes<T>& nd, double* tab, long long n, const double* __restrict__ m, const double* __restrict__ v,
                                        int ldf, int absv, int lane) {
  if (lane < 2 * T) {
    const int dim = lane / T, i = lane - dim * T;
    double vk = v[n * ldf + dim];
    if (absv) vk = fabs(vk);
    const double f = gh_x(T, i) * sqrt(2.0 * vk) + m[n * ldf + dim];
    tab[20 * dim + i] = dim == 0 ? f : weibull_shape(f);
  }
  __builtin_amdgcn_wave_barrier();  // written and read by this wave only (LDS operations of a wave are in order)
#pragma unroll
  for (int u = 0; u < WbNodes<T>::U; ++u) {
    const int node = lane + 64 * u;
    const bool in = node < T * T;
    const int i = in ? node / T : 0, j = in ? node - i * T : 0;
    nd.f0[u] = tab[i], nd.k[u] = tab[20 + j];
    nd.w[u] = in ? gh_wn(T, i) * gh_wn(T, j) : 0.0;
  }
}
// cdf, sf and the density in x = log y, each the same bits in every lane
template <int T>
__device__ __forceinline__ void wb_eval(const WbNodes<T>& nd, double x, double& C, double& S, double& D) {
  double c = 0.0, s = 0.0, d = 0.0;
#pragma unroll
  for (int u = 0; u < WbNodes<T>::U; ++u) {
    const double e = exp(fmin(nd.k[u] * (x - nd.f0[u]), HMOGP_WEIBULL_ZMAX)), em = exp(-e);
    c += nd.w[u] * -expm1(-e);
    s += nd.w[u] * em;
    d += nd.w[u] * (nd.k[u] * e * em);
  }
  C = wave_sum(c), S = wave_sum(s), D = wave_sum(d);
}

// y: [N] log of the time (-inf: a time <= 0)
template <int T>
__global__ __launch_bounds__(256) void pcdf_wave_kernel(long long N, const double* __restrict__ y, const double* __restrict__ m,
                                                        const double* __restrict__ v, int ldf, int absv, double* __restrict__ cdf,
                                                        double* __restrict__ sf) {
  static_assert(40 <= HMOGP_ETAB, "node table");
  __shared__ double etab[4][HMOGP_ETAB];
  const int lane = threadIdx.x & 63, w4 = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * 4 + w4;
  if (n >= N) return;
  WbNodes<T> nd;
  wb_fill<T>(nd, etab[w4], n, m, v, ldf, absv, lane);
  const double ly = y[n];
  double C, S, D;
  wb_eval<T>(nd, ly, C, S, D);
  if (ly == -INFINITY) C = 0.0, S = 1.0;
  if (lane == 0) {
    if (cdf) cdf[n] = C;
    if (sf) sf[n] = S;
  }
}

template <int T>
__global__ __launch_bounds__(256) void pquant_wave_kernel(long long N, int nP, PqProbs pr, const double* __restrict__ m,
                                                          const double* __restrict__ v, int ldf, int absv, double* __restrict__ q) {
  static_assert(40 <= HMOGP_ETAB, "node table");
  __shared__ double etab[4][HMOGP_ETAB];
  const int lane = threadIdx.x & 63, w4 = threadIdx.x >> 6;
  const long long n = (long long)blockIdx.x * 4 + w4;
  if (n >= N) return;
  WbNodes<T> nd;
  wb_fill<T>(nd, etab[w4], n, m, v, ldf, absv, lane);
  const double m0 = m[n * ldf];
  double v0 = v[n * ldf];
  if (absv) v0 = fabs(v0);
  const double rk = 1.0 / weibull_shape(m[n * ldf + 1]);
  const double d0 = 1.0 + rk + sqrt(2.0 * v0);
  for (int ip = 0; ip < nP; ++ip) {
    const double p = pr.p[ip];
    double res = nan("");
    if (pq_valid_p(p)) {
      const bool use_sf = p > 0.5;
      const double tq = use_sf ? 1.0 - p : p;
      PqSolver sv;
      sv.init(tq, use_sf, m0 + pq_loglog(tq, use_sf) * rk, d0);
#pragma unroll 1
      for (int ev = 0; ev < PQ_MAXEVAL; ++ev) {
        double C, S, D;
        wb_eval<T>(nd, sv.x, C, S, D);
        if (sv.step(use_sf ? S : C, D)) break;
      }
      res = exp(sv.result);
    }
    if (lane == 0) q[n * nP + ip] = res;
  }
}

// the five of the six families whose rule runs one lane per row (Weibull, the sixth: one wave per row)
constexpr bool predq_lane(int lik) {
  return lik == HMOGP_LIK_GAUSSIAN || lik == HMOGP_LIK_HETGAUSSIAN || lik == HMOGP_LIK_BERNOULLI || lik == HMOGP_LIK_EXPONENTIAL ||
         lik == HMOGP_LIK_ORDINAL;
}

}  // namespace

const char* predq_refusal(int lik) {
  switch (lik) {
    case HMOGP_LIK_GAUSSIAN:
    case HMOGP_LIK_HETGAUSSIAN:
    case HMOGP_LIK_BERNOULLI:
    case HMOGP_LIK_EXPONENTIAL:
    case HMOGP_LIK_ORDINAL:
    case HMOGP_LIK_WEIBULL: return nullptr;
    case HMOGP_LIK_POISSON: return "predictive cdf / quantile: Poisson needs a regularised incomplete gamma function, which is not built";
    case HMOGP_LIK_GAMMA: return "predictive cdf / quantile: Gamma needs a regularised incomplete gamma function, which is not built";
    case HMOGP_LIK_BETA: return "predictive cdf / quantile: Beta needs a regularised incomplete beta function, which is not built";
    case HMOGP_LIK_STUDENT: return "predictive cdf / quantile: Student needs a regularised incomplete beta function, which is not built";
    case HMOGP_LIK_NEGBINOMIAL:
      return "predictive cdf / quantile: NegBinomial needs a regularised incomplete beta function, which is not built";
    case HMOGP_LIK_BINOMIAL: return "predictive cdf / quantile: Binomial needs a regularised incomplete beta function, which is not built";
    case HMOGP_LIK_BETABINOMIAL:
      return "predictive cdf / quantile: BetaBinomial needs a regularised incomplete beta function, which is not built";
    case HMOGP_LIK_ZIPOISSON: return "predictive cdf / quantile: ZIPoisson needs a regularised incomplete gamma function, which is not built";
    case HMOGP_LIK_CATEGORICAL: return "predictive cdf / quantile: Categorical has no order";
    case HMOGP_LIK_DIRICHLET: return "predictive cdf / quantile: Dirichlet is multivariate";
    default: return "predictive cdf / quantile: unknown likelihood id";
  }
}

static void predq_check(const PqArgs& a) {
  if (predq_refusal(a.lik)) throw HipError{hipErrorInvalidValue, predq_refusal(a.lik), __FILE__, __LINE__};
  if (a.T != 10 && a.T != 20)
    throw HipError{hipErrorInvalidValue, "predictive cdf / quantile: nodes per dimension must be 10 or 20", __FILE__, __LINE__};
}

void launch_predictive_cdf(const PqArgs& a, hipStream_t s) {
  predq_check(a);
  if (a.N <= 0) return;
  const dim3 glane((unsigned)((a.N + 255) / 256)), gwave((unsigned)((a.N + 3) / 4));
  visit_family(a.lik, 0, [&](auto fam) {   // (predq_check let only the six families through: none of them has a function count)
    constexpr int L = decltype(fam)::LIK;
    if constexpr (predq_lane(L)) {
      hipLaunchKernelGGL((pcdf_lane_kernel<L>), glane, dim3(256), 0, s, a.param, a.T, a.N, a.y, a.ldy, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.cdf, a.sf);
    } else if constexpr (L == HMOGP_LIK_WEIBULL) {
      if (a.T == 10) hipLaunchKernelGGL((pcdf_wave_kernel<10>), gwave, dim3(256), 0, s, a.N, a.y, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.cdf, a.sf);
      else hipLaunchKernelGGL((pcdf_wave_kernel<20>), gwave, dim3(256), 0, s, a.N, a.y, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.cdf, a.sf);
    } else {
      throw HipError{hipErrorInvalidValue, predq_refusal(L), __FILE__, __LINE__};
    }
  });
}

void launch_predictive_quantile(const PqArgs& a, hipStream_t s) {
  predq_check(a);
  if (a.nP < 1 || a.nP > HMOGP_QUANT_MAXP)
    throw HipError{hipErrorInvalidValue, "predictive quantile: 1 <= nP <= HMOGP_QUANT_MAXP", __FILE__, __LINE__};
  if (a.N <= 0) return;
  const dim3 glane((unsigned)((a.N + 255) / 256)), gwave((unsigned)((a.N + 3) / 4));
  PqProbs pr;
  for (int i = 0; i < HMOGP_QUANT_MAXP; ++i) pr.p[i] = i < a.nP ? a.p[i] : 0.5;
  const OrdinalTable tb = a.table ? *a.table : OrdinalTable();
  visit_family(a.lik, 0, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK;
    if constexpr (L == HMOGP_LIK_GAUSSIAN || L == HMOGP_LIK_ORDINAL) {   // (closed form: no nodes)
      hipLaunchKernelGGL((pquant_lane_kernel<L, 10>), glane, dim3(256), 0, s, a.param, tb, a.N, a.nP, pr, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.q);
    } else if constexpr (predq_lane(L)) {
      if (a.T == 10) hipLaunchKernelGGL((pquant_lane_kernel<L, 10>), glane, dim3(256), 0, s, a.param, tb, a.N, a.nP, pr, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.q);
      else hipLaunchKernelGGL((pquant_lane_kernel<L, 20>), glane, dim3(256), 0, s, a.param, tb, a.N, a.nP, pr, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.q);
    } else if constexpr (L == HMOGP_LIK_WEIBULL) {
      if (a.T == 10) hipLaunchKernelGGL((pquant_wave_kernel<10>), gwave, dim3(256), 0, s, a.N, a.nP, pr, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.q);
      else hipLaunchKernelGGL((pquant_wave_kernel<20>), gwave, dim3(256), 0, s, a.N, a.nP, pr, a.m, a.v, a.ldf, a.absv ? 1 : 0, a.q);
    } else {
      throw HipError{hipErrorInvalidValue, predq_refusal(L), __FILE__, __LINE__};
    }
  });
}
