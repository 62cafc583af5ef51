// lik_dispatch.h -- the one place where a run-time (likelihood id, function count) becomes a compile-time family: every launcher
// that picks a kernel instantiation per family is one generic lambda handed to visit_family, and names the families it treats
// differently with `if constexpr`.  A family a launcher does not provide for fails to compile or reaches that launcher's own `else`.
#pragma once
#include "common.h"
#include "../../include/hetmogp_hip.h"

template <int LIK_, int D_ = 0>
struct Family {
  static constexpr int LIK = LIK_, D = D_;
};

// calls f(Family<LIK, D>{}); D = the function count of Categorical (1 .. 8: K - 1) and Dirichlet (2 .. HMOGP_DIRICHLET_MAXK: K), 0 for every
// other family, whose `dimf` is not looked at
template <class F>
void visit_family(int lik, int dimf, F&& f) {
  static_assert(HMOGP_DIRICHLET_MAXK == 4, "visit_family lists Dirichlet K = 2 .. 4");
  switch (lik) {
    case HMOGP_LIK_GAUSSIAN: f(Family<HMOGP_LIK_GAUSSIAN>{}); break;
    case HMOGP_LIK_BERNOULLI: f(Family<HMOGP_LIK_BERNOULLI>{}); break;
    case HMOGP_LIK_HETGAUSSIAN: f(Family<HMOGP_LIK_HETGAUSSIAN>{}); break;
    case HMOGP_LIK_CATEGORICAL:
      switch (dimf) {
        case 1: f(Family<HMOGP_LIK_CATEGORICAL, 1>{}); break;
        case 2: f(Family<HMOGP_LIK_CATEGORICAL, 2>{}); break;
        case 3: f(Family<HMOGP_LIK_CATEGORICAL, 3>{}); break;
        case 4: f(Family<HMOGP_LIK_CATEGORICAL, 4>{}); break;
        case 5: f(Family<HMOGP_LIK_CATEGORICAL, 5>{}); break;
        case 6: f(Family<HMOGP_LIK_CATEGORICAL, 6>{}); break;
        case 7: f(Family<HMOGP_LIK_CATEGORICAL, 7>{}); break;
        case 8: f(Family<HMOGP_LIK_CATEGORICAL, 8>{}); break;
        default: throw HipError{hipErrorInvalidValue, "Categorical needs 2 <= K <= 9", __FILE__, __LINE__};
      }
      break;
    case HMOGP_LIK_POISSON: f(Family<HMOGP_LIK_POISSON>{}); break;
    case HMOGP_LIK_EXPONENTIAL: f(Family<HMOGP_LIK_EXPONENTIAL>{}); break;
    case HMOGP_LIK_GAMMA: f(Family<HMOGP_LIK_GAMMA>{}); break;
    case HMOGP_LIK_BETA: f(Family<HMOGP_LIK_BETA>{}); break;
    case HMOGP_LIK_STUDENT: f(Family<HMOGP_LIK_STUDENT>{}); break;
    case HMOGP_LIK_ORDINAL: f(Family<HMOGP_LIK_ORDINAL>{}); break;
    case HMOGP_LIK_DIRICHLET:
      switch (dimf) {
        case 2: f(Family<HMOGP_LIK_DIRICHLET, 2>{}); break;
        case 3: f(Family<HMOGP_LIK_DIRICHLET, 3>{}); break;
        case 4: f(Family<HMOGP_LIK_DIRICHLET, 4>{}); break;
        default: throw HipError{hipErrorInvalidValue, "Dirichlet needs 2 <= K <= HMOGP_DIRICHLET_MAXK", __FILE__, __LINE__};
      }
      break;
    case HMOGP_LIK_NEGBINOMIAL: f(Family<HMOGP_LIK_NEGBINOMIAL>{}); break;
    case HMOGP_LIK_WEIBULL: f(Family<HMOGP_LIK_WEIBULL>{}); break;
    case HMOGP_LIK_BINOMIAL: f(Family<HMOGP_LIK_BINOMIAL>{}); break;
    case HMOGP_LIK_BETABINOMIAL: f(Family<HMOGP_LIK_BETABINOMIAL>{}); break;
    case HMOGP_LIK_ZIPOISSON: f(Family<HMOGP_LIK_ZIPOISSON>{}); break;
    default: throw HipError{hipErrorInvalidValue, "unknown likelihood id", __FILE__, __LINE__};
  }
}
