// xgrad.hip -- gradients of q(f) with respect to the new inputs (gfx950): the two kernels behind hmogp_qf_input_grad /
// hmogp_predict_f_grad.  With A_q = k_q(X, Z_q) (the image the mean was formed with, read back from memory, never recomputed here) and
// T_q = A_q C_q (the existing FP64-MFMA GEMM):
//
//   qf_xgrad           gp[q][i][j] = (1 / l_q^2) sum_m a_qm   A_q[i][m] (z_qmj - x_ij)          (d p_q / d x_j)
//                      gc[q][i][j] = (2 / l_q^2) sum_m T_q[i][m] A_q[i][m] (z_qmj - x_ij)       (d c_q / d x_j)
//                      (z - x) is ONE subtraction per term -- never sum k z - x sum k, which cancels when x sits on an inducing input.
//                      A wave owns R rows (4 for P <= 2, 2 for P = 3, 4), four waves per block; the lanes walk m in neighbouring pairs
//                      (16-byte loads of the A and T rows when M is even, 8-byte loads when it is odd); the lane's pair of a and its two
//                      inducing inputs (through L2: every wave reads the same ones) are loaded once per round and serve the R rows;
//                      every lane keeps 2 P fma chains PER ROW in its own fixed m-order, then the fixed xor tree of wave_sum.  No LDS,
//                      no atomics, nothing shared between rows but the loaded a and z: a row's bits depend on that row's own inputs
//                      alone -- not on N, not on its slot in the wave, its place in the block, grid or chunk.  HBM-bound reader:
//                      2 n M Q 8 B.  Measured: one row per wave 3.69 TB/s (bound by the re-reads of a and Z, 56 KB of L1
//                      traffic per 32 KB of HBM at M = 1024), two rounds of it in flight 3.45, this shape 5.99.
//   qf_xgrad_combine   dm[i][d][j] = sum_q W_qd gp[q][i][j],  dv[i][d][j] = sum_q W_qd^2 gc[q][i][j], q from left to right as
//                      qf_combine_kernel adds them.  (The prior term of v_d is constant in x: the kernel is stationary.)
#include "rowpass.h"
#include "rbf_device.h"

namespace {

constexpr int XG_WAVES = 4;       // waves per 256-thread block

// rows a wave takes through the m-loop side by side: the lane's pair of a and its two inducing inputs are loaded once per round and serve
// every one of them (with one row per wave the kernel was bound by those re-reads, not by HBM); 2 P R accumulators per lane
template <int P>
constexpr int xg_rows() { return P <= 2 ? 4 : 2; }

template <int P>
__device__ __forceinline__ void xg_term(double k, double t, double am, const double (&z)[P], const double (&x)[P], double (&gp)[P],
                                        double (&gc)[P]) {
  const double ak = am * k, tk = t * k;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const double d = z[j] - x[j];
    gp[j] = fma(ak, d, gp[j]);
    gc[j] = fma(tk, d, gc[j]);
  }
}

template <int P>
__global__ __launch_bounds__(256) void qf_xgrad_kernel(XgradArgs g) {
  constexpr int R = xg_rows<P>();
  const int lane = threadIdx.x & 63;
  const long long i0 = ((long long)blockIdx.x * XG_WAVES + (threadIdx.x >> 6)) * R;
  if (i0 >= g.n) return;                                 // (wave-uniform: a wave owns R rows)
  const int q = blockIdx.y, M = g.M;
  const double* __restrict__ Aq = g.A + (long long)q * g.sK;
  const double* __restrict__ Tq = g.T + (long long)q * g.sK;
  const double* __restrict__ Zq = g.Z + (long long)q * P;
  const double* __restrict__ aq = g.a + (long long)q * M;
  long long ro[R];                                       // offset of the row in A and T; a slot beyond the last row re-reads the last row
  double x[R][P], gp[R][P], gc[R][P];                    // (and is never stored): every index below is a compile-time constant
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const long long i = i0 + r < g.n ? i0 + r : g.n - 1;
    ro[r] = i * M;
#pragma unroll
    for (int j = 0; j < P; ++j) x[r][j] = g.X[i * P + j], gp[r][j] = 0.0, gc[r][j] = 0.0;
  }
  for (int m = 2 * lane; m < M; m += 2 * HMOGP_WAVE) {
    const bool two = m + 1 < M;                          // (always, when M is even)
    const int m1 = two ? m + 1 : m;
    const double a0 = aq[m], a1 = aq[m1];
    double z0[P], z1[P];
#pragma unroll
    for (int j = 0; j < P; ++j) z0[j] = Zq[(long long)m * g.ldz + j], z1[j] = Zq[(long long)m1 * g.ldz + j];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      double k0, k1, t0, t1;
      if (g.vec) {                                       // M even, rows 16-byte aligned: the pair (m, m + 1) in one load each
        const f64x2 k = *reinterpret_cast<const f64x2*>(Aq + ro[r] + m), t = *reinterpret_cast<const f64x2*>(Tq + ro[r] + m);
        k0 = k[0], k1 = k[1], t0 = t[0], t1 = t[1];
      } else {
        k0 = Aq[ro[r] + m], t0 = Tq[ro[r] + m], k1 = Aq[ro[r] + m1], t1 = Tq[ro[r] + m1];
      }
      xg_term<P>(k0, t0, a0, z0, x[r], gp[r], gc[r]);
      if (two) xg_term<P>(k1, t1, a1, z1, x[r], gp[r], gc[r]);
    }
  }
  const double ell = g.ell[q], inv_l2 = 1.0 / (ell * ell);
#pragma unroll
  for (int r = 0; r < R; ++r) {
#pragma unroll
    for (int j = 0; j < P; ++j) gp[r][j] = wave_sum(gp[r][j]), gc[r][j] = wave_sum(gc[r][j]);
    if (lane == 0 && i0 + r < g.n) {
      double* op = g.gp + ((long long)q * g.ldo + i0 + r) * P;
      double* oc = g.gc + ((long long)q * g.ldo + i0 + r) * P;
#pragma unroll
      for (int j = 0; j < P; ++j) op[j] = inv_l2 * gp[r][j], oc[j] = (2.0 * inv_l2) * gc[r][j];
    }
  }
}

// one thread per (row, function, input dimension)
__global__ void qf_xgrad_combine_kernel(const double* __restrict__ gp, const double* __restrict__ gc, long long ldo, long long n, int Q,
                                        int Df, int P, const double* __restrict__ W, double* __restrict__ dm, double* __restrict__ dv) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * Df * P) return;
  const int j = (int)(e % P), d = (int)((e / P) % Df);
  const long long i = e / ((long long)P * Df);
  double mm = 0.0, vv = 0.0;
  for (int q = 0; q < Q; ++q) {
    const double w = W[q * Df + d];
    const long long o = ((long long)q * ldo + i) * P + j;
    mm += w * gp[o];
    vv += w * w * gc[o];
  }
  dm[e] = mm;
  dv[e] = vv;
}

bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void launch_qf_xgrad(const XgradArgs& a, hipStream_t s) {
  if (a.n <= 0) return;
  if (a.Q < 1 || a.Q > HMOGP_MAXQ) throw HipError{hipErrorInvalidValue, "latent count must be 1..HMOGP_MAXQ", __FILE__, __LINE__};
  if (a.M < 1 || a.sK < a.n * a.M || a.ldo < a.n) throw HipError{hipErrorInvalidValue, "bad input-gradient shapes", __FILE__, __LINE__};
  XgradArgs g = a;
  g.vec = ((a.M & 1) == 0 && (a.sK & 1) == 0 && al16(a.A) && al16(a.T)) ? 1 : 0;
  DISPATCH_P(a.P, {
    const long long per = (long long)XG_WAVES * xg_rows<PP>();
    hipLaunchKernelGGL((qf_xgrad_kernel<PP>), dim3((unsigned)((a.n + per - 1) / per), (unsigned)a.Q), dim3(64 * XG_WAVES), 0, s, g);
  });
}

void launch_qf_xgrad_combine(const double* gp, const double* gc, long long ldo, long long n, int Q, int Df, int P, const double* W,
                             double* dm, double* dv, hipStream_t s) {
  if (n <= 0) return;
  const long long tot = n * Df * P;
  hipLaunchKernelGGL(qf_xgrad_combine_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, gp, gc, ldo, n, Q, Df, P, W, dm,
                     dv);
}
