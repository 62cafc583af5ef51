// paths.hip -- pathwise (Matheron) posterior samples (gfx950): the kernels that join the existing building blocks
// (launch_rbf, the FP64-MFMA GEMM, the row solves against Luu) into hmogp_paths_create / hmogp_paths_eval.
//
//   paths_feature   Phi[q][i][l] = c_q cos(pi t), Phi[q][i][Lf + l] = c_q sin(pi t), t = sum_p omega[q][l][p] x_ip: the random Fourier
//                   features of a chunk of rows, every latent (grid.z).  One sincospi per (row, frequency): its argument reduction is
//                   exact, so there is no large-argument slow path -- no Payne-Hanek tables, no scratch.  Lanes run along l: a wave
//                   instruction stores 64 x 16 B = 1 KiB of one row, the cosines at l and the sines at Lf + l.  Writer of
//                   rows x Q x 2 Lf x 8 B; the same kernel forms Phi_q(Z_q) for the draw.
//   paths_omega     omega[q][l][p] = zeta / (pi ell_q), zeta = z0 of normal_pair(seed, l, 4 q + p, 1)
//   paths_normal    out[q][s][k] = z0 of normal_pair(seed, k, s Q + q, pair): theta (pair 2, k < 2 Lf) and eps (pair 3, k < M; with
//                   u[q][s][m] = m_q[m] written beside it, for u += eps L_q^T to accumulate onto)
//   paths_scale     Theta~ = w theta + sqrt(kappa) theta' (theta' = pair 4 at n = d 2 Lf + k), V~ = w v, both [rows][S nD]: the operands
//                   of the two accumulating products of an evaluation
#include <algorithm>

#include "rowpass.h"
#include "lik_device.h"
#include "rbf_device.h"

namespace {

constexpr int FR = 16;            // rows per block of the feature kernel: four waves, four rows each

// stream tags of the draws (the `pair` argument of normal_pair; below 256: its hash packs s << 8 with the pair)
constexpr int TAG_FREQ = 1, TAG_PRIOR = 2, TAG_QU = 3, TAG_KAPPA = 4;

template <int P, bool VEC>
__global__ __launch_bounds__(256) void paths_feature_kernel(PathsArgs a) {
  constexpr int LPT = VEC ? 2 : 1;                       // frequencies per lane: a 16-byte store where Lf is even, else 8 bytes
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, q = blockIdx.z;
  const int l0 = ((int)blockIdx.y * 64 + tx) * LPT;
  if (l0 >= a.Lf) return;                                // (VEC: Lf and l0 are even, so l0 + 1 < Lf too)
  double w[LPT][P];
  const double* om = a.omega + ((long long)q * a.Lf + l0) * P;
#pragma unroll
  for (int e = 0; e < LPT; ++e)
#pragma unroll
    for (int p = 0; p < P; ++p) w[e][p] = om[e * P + p];
  const double c = a.cq[q];
  const double* X = a.X + (long long)q * a.sX;
  double* Phi = a.Phi + (long long)q * a.rows * 2 * a.Lf;
  const long long r0 = (long long)blockIdx.x * FR + ty * (FR / 4);
#pragma unroll
  for (int r = 0; r < FR / 4; ++r) {
    const long long i = r0 + r;
    if (i >= a.rows) break;                              // (wave-uniform)
    double x[P];
#pragma unroll
    for (int p = 0; p < P; ++p) x[p] = X[i * a.ldx + p];
    double cs[LPT], sn[LPT];
#pragma unroll
    for (int e = 0; e < LPT; ++e) {
      double t = w[e][0] * x[0];                         // in p order, one rounding per further term
#pragma unroll
      for (int p = 1; p < P; ++p) t = fma(w[e][p], x[p], t);
      double s_, c_;
      sincospi(t, &s_, &c_);
      cs[e] = c * c_, sn[e] = c * s_;
    }
    double* row = Phi + i * 2 * a.Lf + l0;
    if (VEC) {
      *reinterpret_cast<f64x2*>(row) = f64x2{cs[0], cs[LPT - 1]};
      *reinterpret_cast<f64x2*>(row + a.Lf) = f64x2{sn[0], sn[LPT - 1]};
    } else {
      row[0] = cs[0];
      row[a.Lf] = sn[0];
    }
  }
}

__global__ __launch_bounds__(256) void paths_omega_kernel(unsigned long long seed, int Q, int P, int Lf, const double* __restrict__ ell,
                                                          double* __restrict__ omega) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)Q * Lf * P) return;
  const int p = (int)(i % P), l = (int)((i / P) % Lf), q = (int)(i / ((long long)P * Lf));
  double z0, z1;
  normal_pair(seed, l, q * 4 + p, TAG_FREQ, z0, z1);
  omega[i] = z0 / (M_PI * ell[q]);
}

// out[q][s][k] = z0 of normal_pair(seed, k, s Q + q, pair) for k < K; with u (and mu [K][Q]): u[q][s][k] = mu[k][q] beside it
__global__ __launch_bounds__(256) void paths_normal_kernel(unsigned long long seed, int Q, int S, int K, int pair, double* __restrict__ out,
                                                           const double* __restrict__ mu, double* __restrict__ u) {
  const int k = (int)blockIdx.x * 256 + threadIdx.x, q = blockIdx.z;
  if (k >= K) return;
  const double m = u ? mu[(long long)k * Q + q] : 0.0;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    double z0, z1;
    normal_pair(seed, k, s * Q + q, pair, z0, z1);
    const long long o = ((long long)q * S + s) * K + k;
    out[o] = z0;
    if (u) u[o] = m;
  }
}

// rows r < 2 Lf: Theta~[q][r][c] = w theta[q][s][r] + sk theta'(d_j, q, s)[r]; rows 2 Lf + m: V~[q][m][c] = w v[q][s][m]; c = s nD + j
__global__ __launch_bounds__(256) void paths_scale_kernel(unsigned long long seed, int Q, int Lf, int S, int M, int nD,
                                                          const int* __restrict__ d, const double* __restrict__ w,
                                                          const double* __restrict__ sk, const double* __restrict__ theta,
                                                          const double* __restrict__ v, double* __restrict__ Theta, double* __restrict__ V) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x, q = blockIdx.z, nc = S * nD, K2 = 2 * Lf;
  if (c >= nc) return;
  const int s = c / nD, j = c - s * nD;
  const double wj = w[q * nD + j], sj = sk[q * nD + j];
  const int dj = d[j];
  for (int r = blockIdx.y; r < K2 + M; r += gridDim.y) {
    if (r < K2) {
      double z0, z1;
      normal_pair(seed, (long long)dj * K2 + r, s * Q + q, TAG_KAPPA, z0, z1);
      Theta[((long long)q * K2 + r) * nc + c] = fma(sj, z0, wj * theta[((long long)q * S + s) * K2 + r]);
    } else {
      const int m = r - K2;
      V[((long long)q * M + m) * nc + c] = wj * v[((long long)q * S + s) * M + m];
    }
  }
}

template <int P>
void launch_features_p(const PathsArgs& a, hipStream_t s) {
  const bool vec = (a.Lf & 1) == 0;
  const int per = vec ? 128 : 64;                        // frequencies per block
  const dim3 grid((unsigned)((a.rows + FR - 1) / FR), (unsigned)((a.Lf + per - 1) / per), (unsigned)a.Q);
  if (vec) hipLaunchKernelGGL((paths_feature_kernel<P, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((paths_feature_kernel<P, false>), grid, dim3(256), 0, s, a);
}

}  // namespace

void launch_paths_features(const PathsArgs& a, hipStream_t s) {
  if (a.rows <= 0 || a.Lf <= 0 || a.Q <= 0) return;
  if (a.Q > HMOGP_MAXQ) throw HipError{hipErrorInvalidValue, "latent count must be 1..HMOGP_MAXQ", __FILE__, __LINE__};
  if (a.rows > 0x7fffffffLL) throw HipError{hipErrorInvalidValue, "paths: too many rows in one chunk", __FILE__, __LINE__};
  DISPATCH_P(a.P, launch_features_p<PP>(a, s));
}

void launch_paths_draw(unsigned long long seed, int Q, int P, int Lf, int S, int M, const double* ell, const double* mu, double* omega,
                       double* theta, double* eps, double* u, hipStream_t s) {
  if (Q <= 0 || Lf <= 0 || S <= 0 || M <= 0) return;
  const long long no = (long long)Q * Lf * P;
  hipLaunchKernelGGL(paths_omega_kernel, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, s, seed, Q, P, Lf, ell, omega);
  const unsigned gy = (unsigned)std::min(S, 1024);
  hipLaunchKernelGGL(paths_normal_kernel, dim3((unsigned)((2 * Lf + 255) / 256), gy, (unsigned)Q), dim3(256), 0, s, seed, Q, S, 2 * Lf,
                     TAG_PRIOR, theta, nullptr, nullptr);
  hipLaunchKernelGGL(paths_normal_kernel, dim3((unsigned)((M + 255) / 256), gy, (unsigned)Q), dim3(256), 0, s, seed, Q, S, M, TAG_QU, eps,
                     mu, u);
}

void launch_paths_scale(unsigned long long seed, int Q, int Lf, int S, int M, int nD, const int* d, const double* w, const double* sk,
                        const double* theta, const double* v, double* Theta, double* V, hipStream_t s) {
  if (Q <= 0 || Lf <= 0 || S <= 0 || M <= 0 || nD <= 0) return;
  const int nc = S * nD;
  hipLaunchKernelGGL(paths_scale_kernel, dim3((unsigned)((nc + 255) / 256), (unsigned)std::min(2 * Lf + M, 4096), (unsigned)Q), dim3(256),
                     0, s, seed, Q, Lf, S, M, nD, d, w, sk, theta, v, Theta, V);
}
