// lik_host.hip -- what the host knows about the likelihood families, in one place: functions per row, parameter checks, the checks of a
// family's Y and the image of it the row kernels read, the Ordinal registry, the node counts of the deterministic rules.  No kernels,
// and nothing here needs a device except the two uploads.  Declarations: engine_impl.h (ordinal_table: lik_launch.h).
#include "engine_impl.h"

#include <memory>
#include <mutex>

namespace hmogp_detail {

int lik_dimf(int lik, double param) {
  switch (lik) {
    case HMOGP_LIK_GAUSSIAN:
    case HMOGP_LIK_BERNOULLI:
    case HMOGP_LIK_POISSON:
    case HMOGP_LIK_EXPONENTIAL:
    case HMOGP_LIK_ORDINAL:
    case HMOGP_LIK_BINOMIAL: return 1;
    case HMOGP_LIK_HETGAUSSIAN:
    case HMOGP_LIK_GAMMA:
    case HMOGP_LIK_BETA:
    case HMOGP_LIK_STUDENT:
    case HMOGP_LIK_NEGBINOMIAL:
    case HMOGP_LIK_WEIBULL:
    case HMOGP_LIK_BETABINOMIAL:
    case HMOGP_LIK_ZIPOISSON: return 2;
    case HMOGP_LIK_CATEGORICAL: return (int)param - 1;
    case HMOGP_LIK_DIRICHLET: return (param >= 2.0 && param <= (double)HMOGP_DIRICHLET_MAXK) ? (int)param : -1;
    default: return -1;
  }
}

void check_lik_param(int lik, double param) {
  if (lik == HMOGP_LIK_STUDENT && !(std::isfinite(param) && param > 0.0))
    throw EngineError{HMOGP_E_INVALID, "Student: deg_free must be finite and > 0"};
  if (lik == HMOGP_LIK_ORDINAL) (void)ordinal_table(param);
  if (lik == HMOGP_LIK_DIRICHLET && !(param >= 2.0 && param <= (double)HMOGP_DIRICHLET_MAXK && param == std::floor(param)))
    throw EngineError{HMOGP_E_INVALID, "Dirichlet: K must be an integer in 2 .. HMOGP_DIRICHLET_MAXK"};
  // Binomial, Beta-Binomial: the trial count n* of predictive / sample; 0.0 means 1
  if (lik_has_trials(lik) && param != 0.0 &&
      !(param >= 1.0 && param <= 1e9 && param == std::floor(param)))
    throw EngineError{HMOGP_E_INVALID, lik == HMOGP_LIK_BINOMIAL ? "Binomial: the trial count n* (lik_param) must be an integer in 1 .. 1e9, or 0 for 1"
                                                                 : "BetaBinomial: the trial count n* (lik_param) must be an integer in 1 .. 1e9, or 0 for 1"};
}

// ------------------------------------------------------------------------------------ Binomial / Beta-Binomial rows
void binomial_check_rows(int lik, const double* y, long long N, double* img) {
  const bool bb = lik == HMOGP_LIK_BETABINOMIAL;
  for (long long i = 0; i < N; ++i) {
    const double k = y[2 * i], n = y[2 * i + 1];
    if (!(std::isfinite(n) && n >= 1.0 && n <= 1e9 && n == std::floor(n)))
      throw EngineError{HMOGP_E_INVALID, bb ? "BetaBinomial: every trial count n must be an integer in 1 .. 1e9"
                                            : "Binomial: every trial count n must be an integer in 1 .. 1e9"};
    if (!(std::isfinite(k) && k >= 0.0 && k <= n && k == std::floor(k)))
      throw EngineError{HMOGP_E_INVALID, bb ? "BetaBinomial: every count k must be an integer in 0 .. n"
                                            : "Binomial: every count k must be an integer in 0 .. n"};
    img[i] = k;
    img[N + i] = n;
    img[2 * N + i] = std::lgamma(n + 1.0) - std::lgamma(k + 1.0) - std::lgamma(n - k + 1.0);
  }
}

// ------------------------------------------------------------------------------------ zero-inflated Poisson rows
void zipoisson_check_rows(const double* y, long long N) {
  for (long long n = 0; n < N; ++n)
    if (!(std::isfinite(y[n]) && y[n] >= 0.0 && y[n] == std::floor(y[n])))
      throw EngineError{HMOGP_E_INVALID, "ZIPoisson: every y must be a finite, non-negative integer"};
}

// ------------------------------------------------------------------------------------ Negative Binomial rows
void negbinomial_check_rows(const double* y, long long N) {
  for (long long n = 0; n < N; ++n)
    if (!(std::isfinite(y[n]) && y[n] >= 0.0 && y[n] == std::floor(y[n])))
      throw EngineError{HMOGP_E_INVALID, "NegBinomial: every y must be a finite, non-negative integer"};
}

// ------------------------------------------------------------------------------------ Weibull rows
void weibull_check_rows(const double* y, long long N, double* img) {
  for (long long n = 0; n < N; ++n) {
    const double t = y[2 * n], d = y[2 * n + 1];
    if (!(std::isfinite(t) && t > 0.0)) throw EngineError{HMOGP_E_INVALID, "Weibull: every time y must be finite and > 0"};
    if (!(d == 0.0 || d == 1.0))
      throw EngineError{HMOGP_E_INVALID, "Weibull: every event indicator must be exactly 1 (observed) or 0 (right-censored)"};
    img[n] = std::log(t);
    img[N + n] = d;
  }
}

// ------------------------------------------------------------------------------------ Dirichlet rows
void dirichlet_log_rows(int K, const double* y, long long N, double* ly) {
  for (long long n = 0; n < N; ++n) {
    double s = 0.0;
    for (int k = 0; k < K; ++k) {
      const double yk = y[n * K + k];
      if (!(std::isfinite(yk) && yk > 0.0))
        throw EngineError{HMOGP_E_INVALID, "Dirichlet: every y_k must be finite and > 0 (replace zeros before the call)"};
      s += yk;
      ly[(long long)k * N + n] = std::log(yk);
    }
    if (!(std::fabs(s - 1.0) <= 1e-6)) throw EngineError{HMOGP_E_INVALID, "Dirichlet: a row of Y does not sum to 1 (within 1e-6)"};
  }
}

// ------------------------------------------------------------------------------------ Ordinal tables
// Every entry point carries one double per task; an Ordinal task needs K numbers.  They are registered once, in a process-wide
// append-only registry, and the id (1, 2, ...) travels as lik_param.  Entries are heap-allocated and never freed or moved, so a
// reference handed out stays valid without the lock.
namespace {
std::mutex g_ord_mutex;
std::vector<std::unique_ptr<OrdinalTable>> g_ord_tables;
}  // namespace

double ordinal_register(int K, const double* edges, double sigma) {
  if (K < 2 || K > HMOGP_ORDINAL_MAXK) throw EngineError{HMOGP_E_INVALID, "Ordinal: 2 <= K <= HMOGP_ORDINAL_MAXK"};
  if (!edges) throw EngineError{HMOGP_E_INVALID, "Ordinal: edges is NULL"};
  if (!(std::isfinite(sigma) && sigma > 0.0)) throw EngineError{HMOGP_E_INVALID, "Ordinal: sigma must be finite and > 0"};
  for (int k = 0; k < K - 1; ++k)
    if (!std::isfinite(edges[k]) || (k > 0 && !(edges[k] > edges[k - 1])))
      throw EngineError{HMOGP_E_INVALID, "Ordinal: the cut points must be finite and strictly increasing"};
  std::lock_guard<std::mutex> lock(g_ord_mutex);
  for (size_t i = 0; i < g_ord_tables.size(); ++i) {
    const OrdinalTable& t = *g_ord_tables[i];
    if (t.K == K && t.sigma == sigma && std::equal(edges, edges + (K - 1), t.edge)) return (double)(i + 1);
  }
  if (g_ord_tables.size() >= HMOGP_ORDINAL_MAXTABLES)
    throw EngineError{HMOGP_E_INVALID, "Ordinal: HMOGP_ORDINAL_MAXTABLES distinct tables are registered already"};
  std::unique_ptr<OrdinalTable> t(new OrdinalTable());
  t->K = K, t->sigma = sigma;
  for (int k = 0; k < HMOGP_ORDINAL_MAXK - 1; ++k) t->edge[k] = k < K - 1 ? edges[k] : INFINITY;
  g_ord_tables.push_back(std::move(t));
  return (double)g_ord_tables.size();
}

void ordinal_row_cuts(const OrdinalTable& tb, const double* y, long long N, double* lo, double* hi) {
  for (long long n = 0; n < N; ++n) {
    const double l = y[n];
    if (!(l >= 1.0 && l <= (double)tb.K && l == std::floor(l)))
      throw EngineError{HMOGP_E_INVALID, "Ordinal: a label is not an integer in 1..K"};
    const int k = (int)l;
    lo[n] = k == 1 ? -INFINITY : tb.edge[k - 2];
    hi[n] = k == tb.K ? INFINITY : tb.edge[k - 1];
  }
}

int lik_dparam_cols(int lik) {
  return (lik == HMOGP_LIK_GAUSSIAN || lik == HMOGP_LIK_STUDENT) ? 1 : (lik == HMOGP_LIK_ORDINAL ? 3 : 0);
}

// ------------------------------------------------------------------------------------ a family's Y, checked, as the row kernels read it
std::vector<double> lik_y_image(int lik, const OrdinalTable* tb, int K, const double* y, long long N) {
  std::vector<double> img;
  if (lik == HMOGP_LIK_ORDINAL) {
    img.resize(2 * (size_t)N);
    ordinal_row_cuts(*tb, y, N, img.data(), img.data() + N);
  } else if (lik == HMOGP_LIK_DIRICHLET) {
    img.resize((size_t)K * N);
    dirichlet_log_rows(K, y, N, img.data());
  } else if (lik == HMOGP_LIK_NEGBINOMIAL) {
    negbinomial_check_rows(y, N);
  } else if (lik == HMOGP_LIK_ZIPOISSON) {
    zipoisson_check_rows(y, N);
  } else if (lik == HMOGP_LIK_WEIBULL) {
    img.resize(2 * (size_t)N);
    weibull_check_rows(y, N, img.data());
  } else if (lik_has_trials(lik)) {
    img.resize(3 * (size_t)N);
    binomial_check_rows(lik, y, N, img.data());
  }
  return img;
}

void upload_y_image(int lik_id, double lik_param, const OrdinalTable* tb, const double* y, long long N, DevBuf& dy) {
  if (lik_id == HMOGP_LIK_ORDINAL && !tb) tb = &ordinal_table(lik_param);
  const std::vector<double> img = lik_y_image(lik_id, tb, (int)lik_param, y, N);
  const size_t bytes = sizeof(double) * (img.empty() ? (size_t)N : img.size());
  dy.ensure(bytes);
  HIP_TRY(hipMemcpy(dy.p, img.empty() ? y : img.data(), bytes, hipMemcpyHostToDevice));
}
void upload_y_cdf(int lik_id, double lik_param, const OrdinalTable* tb, const double* y, long long N, DevBuf& dy) {
  if (lik_id != HMOGP_LIK_WEIBULL) {
    upload_y_image(lik_id, lik_param, tb, y, N, dy);
    return;
  }
  std::vector<double> ly((size_t)N);
  for (long long n = 0; n < N; ++n) ly[n] = y[n] > 0.0 ? std::log(y[n]) : (y[n] <= 0.0 ? -INFINITY : y[n]);
  dy.ensure(sizeof(double) * N);
  HIP_TRY(hipMemcpy(dy.p, ly.data(), sizeof(double) * N, hipMemcpyHostToDevice));
}

int predq_nodes(int lik_id, int gh_T) {
  if (const char* why = predq_refusal(lik_id)) throw EngineError{HMOGP_E_INVALID, why};
  if (gh_T != 0 && gh_T != 10 && gh_T != 20) throw EngineError{HMOGP_E_INVALID, "gh_T must be 0, 10 or 20"};
  return gh_T == 0 ? 20 : gh_T;
}

int lpd_nodes(int lik_id, int gh_T) {
  const bool tensor10 = lik_tensor10(lik_id);
  if (gh_T == 0) return tensor10 ? 10 : 20;
  if (tensor10 ? gh_T != 10 : (gh_T != 10 && gh_T != 20))
    throw EngineError{HMOGP_E_INVALID, tensor10 ? "gh_T must be 0 or 10 for Categorical / Dirichlet" : "gh_T must be 0, 10 or 20"};
  return gh_T;
}

}  // namespace hmogp_detail

// (global scope: declared in lik_launch.h, which the kernel launchers share)
const OrdinalTable& ordinal_table(double lik_param) {
  std::lock_guard<std::mutex> lock(hmogp_detail::g_ord_mutex);
  if (!(lik_param >= 1.0 && lik_param <= (double)hmogp_detail::g_ord_tables.size() && lik_param == std::floor(lik_param)))
    throw hmogp_detail::EngineError{HMOGP_E_INVALID, "Ordinal: lik_param is not an id returned by hmogp_ordinal_table"};
  return *hmogp_detail::g_ord_tables[(size_t)lik_param - 1];
}
