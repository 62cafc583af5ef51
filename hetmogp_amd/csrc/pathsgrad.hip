// pathsgrad.hip -- gradients of posterior sample paths with respect to the new inputs (gfx950): the kernels that join the
// state of a path set (paths.hip) and the existing FP64-MFMA GEMM into hmogp_paths_eval_grad.  Both parts of a path are linear
// in what the set stores, so its gradient is the SAME two products against a rotated operand and P derivative images:
//
//   paths_dtheta   Theta~(p)[q][p][l][c]      =  (pi omega[q][l][p]) Theta~[q][Lf + l][c]
//                  Theta~(p)[q][p][Lf + l][c] = -(pi omega[q][l][p]) Theta~[q][l][c]          (c = s nD + j, k-major like Theta~)
//                  d/dx_p (phi^T Theta~) = phi^T Theta~(p): the feature image of the evaluation serves the gradient, no further sincospi.
//                  One product pi omega (the STORED omega is the contract), one product per entry; the sign flip is exact.  Built once
//                  per set, at its first gradient call.
//   rbf_dx         D(p)[p][q][i][m] = A_q[i][m] ((z_qmp - x_ip) inv_l2), inv_l2 = 1 / (l_q l_q): the derivative images of A_q = k_q(X, Z_q),
//                  the image the values were formed with, read back from memory, never recomputed.  (z - x) is ONE subtraction per
//                  term -- never sum a z v - x sum a v, which cancels when x sits on an inducing input.  Lanes run along m (neighbouring
//                  pairs in 16-byte loads and stores where M is even, 8-byte ones where it is odd: chosen on the host); the lane's
//                  inducing inputs are loaded once and serve the DX_ROWS rows of its wave.  An entry depends on its own row, m and p
//                  alone: no LDS, no atomics.  HBM-bound: reads rows M Q 8 B, writes P times that.
//   paths_gtrans   Gt[c][i][p] = G[p][c][i]: the chunk's gradient workspace (what the products write, rows innermost) into the caller's
//                  layout, P innermost, on the device: coalesced reads along the rows, one pitched download per chunk.  (P strided
//                  downloads of 8-byte elements would move every double as its own row of a 2-D copy.)
#include <algorithm>

#include "rowpass.h"
#include "rbf_device.h"

namespace {

constexpr int DX_WAVES = 4;       // waves per 256-thread block
constexpr int DX_ROWS = 8;        // rows a wave takes with one load of its lanes' inducing inputs

__global__ __launch_bounds__(256) void paths_dtheta_kernel(int P, int Lf, int nc, const double* __restrict__ omega,
                                                           const double* __restrict__ Theta, double* __restrict__ dTheta) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x, q = (int)blockIdx.z / P, p = (int)blockIdx.z - q * P, K2 = 2 * Lf;
  if (c >= nc) return;
  const double* Tq = Theta + (long long)q * K2 * nc;
  double* out = dTheta + ((long long)q * P + p) * K2 * nc;
  for (int k = blockIdx.y; k < K2; k += gridDim.y) {
    const int l = k < Lf ? k : k - Lf;
    const double pw = M_PI * omega[((long long)q * Lf + l) * P + p];
    const double t = pw * Tq[(long long)(k < Lf ? Lf + l : l) * nc + c];
    out[(long long)k * nc + c] = k < Lf ? t : -t;
  }
}

template <int P, bool VEC>
__global__ __launch_bounds__(256) void rbf_dx_kernel(RbfDxArgs g) {
#pragma clang fp contract(off)
  constexpr int LPT = VEC ? 2 : 1;                       // inducing inputs per lane
  const int lane = threadIdx.x & 63, q = blockIdx.z;
  const int m0 = ((int)blockIdx.y * 64 + lane) * LPT;
  if (m0 >= g.M) return;                                 // (VEC: M and m0 are even, so m0 + 1 < M too)
  const double ell = g.ell[q], inv_l2 = 1.0 / (ell * ell);
  double z[LPT][P];
#pragma unroll
  for (int e = 0; e < LPT; ++e)
#pragma unroll
    for (int p = 0; p < P; ++p) z[e][p] = g.Z[(long long)(m0 + e) * g.ldz + q * P + p];
  const double* __restrict__ Aq = g.A + (long long)q * g.sK;
  const long long i0 = ((long long)blockIdx.x * DX_WAVES + (threadIdx.x >> 6)) * DX_ROWS;
#pragma unroll
  for (int r = 0; r < DX_ROWS; ++r) {
    const long long i = i0 + r;
    if (i >= g.n) break;                                 // (wave-uniform)
    double x[P];
#pragma unroll
    for (int p = 0; p < P; ++p) x[p] = g.X[i * P + p];
    const long long o = i * g.M + m0;
    double a[LPT];
    if (VEC) {
      const f64x2 v = *reinterpret_cast<const f64x2*>(Aq + o);
      a[0] = v[0], a[LPT - 1] = v[1];
    } else {
      a[0] = Aq[o];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      double d[LPT];
#pragma unroll
      for (int e = 0; e < LPT; ++e) d[e] = a[e] * ((z[e][p] - x[p]) * inv_l2);
      double* out = g.D + ((long long)p * g.Q + q) * g.sK + o;
      if (VEC) *reinterpret_cast<f64x2*>(out) = f64x2{d[0], d[LPT - 1]};
      else out[0] = d[0];
    }
  }
}

// one thread per (column, row) of the chunk: P coalesced reads along the rows, P neighbouring doubles written
__global__ __launch_bounds__(256) void paths_gtrans_kernel(const double* __restrict__ G, int P, long long tot, double* __restrict__ Gt) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= tot) return;
  for (int p = 0; p < P; ++p) Gt[e * P + p] = G[(long long)p * tot + e];
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

template <int P>
void launch_rbf_dx_p(const RbfDxArgs& g, bool vec, hipStream_t s) {
  const int per = vec ? 128 : 64;                        // inducing inputs per block
  const long long rpb = (long long)DX_WAVES * DX_ROWS;
  const dim3 grid((unsigned)((g.n + rpb - 1) / rpb), (unsigned)((g.M + per - 1) / per), (unsigned)g.Q);
  if (vec) hipLaunchKernelGGL((rbf_dx_kernel<P, true>), grid, dim3(64 * DX_WAVES), 0, s, g);
  else hipLaunchKernelGGL((rbf_dx_kernel<P, false>), grid, dim3(64 * DX_WAVES), 0, s, g);
}

}  // namespace

void launch_paths_dtheta(int Q, int P, int Lf, int nc, const double* omega, const double* Theta, double* dTheta, hipStream_t s) {
  if (Q <= 0 || Lf <= 0 || nc <= 0) return;
  if (Q > HMOGP_MAXQ || P < 1 || P > 4) throw HipError{hipErrorInvalidValue, "paths gradient: Q must be 1..HMOGP_MAXQ and P 1..4", __FILE__, __LINE__};
  hipLaunchKernelGGL(paths_dtheta_kernel, dim3((unsigned)((nc + 255) / 256), (unsigned)std::min(2 * Lf, 4096), (unsigned)(Q * P)), dim3(256), 0, s,
                     P, Lf, nc, omega, Theta, dTheta);
}

void launch_rbf_dx(const RbfDxArgs& g, hipStream_t s) {
  if (g.n <= 0) return;
  if (g.Q < 1 || g.Q > HMOGP_MAXQ) throw HipError{hipErrorInvalidValue, "latent count must be 1..HMOGP_MAXQ", __FILE__, __LINE__};
  if (g.M < 1 || g.sK < g.n * g.M || g.n > (1LL << 20)) throw HipError{hipErrorInvalidValue, "bad derivative-image shapes", __FILE__, __LINE__};
  const bool vec = (g.M & 1) == 0 && (g.sK & 1) == 0 && al16(g.A) && al16(g.D);
  DISPATCH_P(g.P, launch_rbf_dx_p<PP>(g, vec, s));
}

void launch_paths_gtrans(const double* G, int P, long long nc, long long n, double* Gt, hipStream_t s) {
  const long long tot = nc * n;
  if (tot <= 0 || P <= 0) return;
  hipLaunchKernelGGL(paths_gtrans_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, G, P, tot, Gt);
}
