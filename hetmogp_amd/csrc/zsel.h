// zsel.h -- inducing inputs chosen from the data by greedy conditional variance (zsel.hip).  Not part of the public interface.
#pragma once
#include <stdint.h>

namespace hmogp_detail {
// The two halves of hmogp_select_inducing (include/hetmogp_hip.h states the contract); the C ABI selects the device in between.
// _check: every host-side refusal (EngineError, HMOGP_E_INVALID), nothing else.  _run, on the current device: the memory question, then two
// launches per pick on one stream with no host synchronisation in between, then the results.  Throws EngineError / HipError.
void select_inducing_check(int64_t N, int P, const double* X, int Q, const double* variance, const double* lengthscale, int Mmax, double tol,
                           int n_forced, const int64_t* forced, const int64_t* pivots, const double* Z, const double* dpiv,
                           const double* trace, const int32_t* Mout);
void select_inducing_run(int64_t N, int P, const double* X, int Q, const double* variance, const double* lengthscale, int Mmax, double tol,
                         int n_forced, const int64_t* forced, int64_t* pivots, double* Z, double* dpiv, double* trace, double* L, double* d,
                         int32_t* Mout);
}  // namespace hmogp_detail
