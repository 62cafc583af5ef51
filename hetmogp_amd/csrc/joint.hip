// joint.hip -- the joint posterior at new inputs (gfx950): the two kernels that join the existing building blocks
// (launch_rbf, the FP64-MFMA GEMM, the row solves, the blocked potrf with GPy's jitter ladder) into hmogp_predict_f_joint /
// hmogp_sample_f_joint.
//
//   joint_assemble   cov[(j, i), (j', i')] = sum_q (w_jq w_j'q + kap_jq [j == j']) k_q(x_i, x_i') + w_jq w_j'q G_q[i, i']
//                    one 64 x 64 tile of (i, i') per block, for EVERY pair of functions: k_q is evaluated once, in registers, and the
//                    G_q tiles are read once (no n x n K** per latent exists anywhere).  HBM-bound writer: n^2 * 8 B.
//   joint_normal     Z[s][i] = z0 of normal_pair(seed, row i, sample s, pair 0); F[s][i] = mean[i] beside it (F = mean + Z L^T then
//                    is ONE beta = 1 product of the existing GEMM)
//   joint_gather     the function-major mean out of q(f)'s [N][Df] rows
#include <algorithm>

#include "rowpass.h"
#include "lik_device.h"
#include "rbf_device.h"

namespace {

// Tile shape.  The kernel is bound by its stores (every (j, j') pair writes the tile two to four times), so the shape follows the
// store path: 16 B per lane, a wave instruction = two 512-byte row segments (32 lanes x 16 B each).  64 columns are those 32 lanes;
// 64 rows make the tile square, so that "lower tile" and "mirror image" are plain tile transposes.  A thread holds k_q and G_q of its
// entries for ALL latents while it loops over the function pairs: 2 * Q * (entries per thread) doubles.  With 16 entries (a whole
// 64 x 64 tile on 256 threads) that is 512 VGPRs at Q = 8 -- so the tile is walked as two 32-row halves of 8 entries per thread
// (256 VGPRs at Q = 8, 128 at Q = 4), and the latent count is a template parameter (1, 2, 4, 8) so that every index is a
// compile-time constant: no scratch.
constexpr int JT = 64;            // tile edge
constexpr int JH = 32;            // rows per half
constexpr int JA = JH / 8;        // row steps per thread: rows ty + 8 a of the half

__device__ __forceinline__ void put2(double* p, double v0, double v1, bool vec, bool ok0, bool ok1) {
  if (vec) {
    if (ok0) *reinterpret_cast<f64x2*>(p) = f64x2{v0, v1};     // (vec: N even, the column index even -> ok1 == ok0, 16-byte aligned)
  } else {
    if (ok0) p[0] = v0;
    if (ok1) p[1] = v1;
  }
}

template <int P, int QM>
__global__ __launch_bounds__(256) void joint_assemble_kernel(JointArgs a) {
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (tj > ti) return;                                   // lower tiles only; the upper ones are their mirror images
  __shared__ double xr[JT][P + 1], xc[JT][P + 1];       // inputs of the tile's rows / columns, |x|^2 in the last slot
  __shared__ double tr[JH][JT + 1];                     // one half tile on its way to the transposed store
  const int t = threadIdx.x;
  const long long N = a.N, n = (long long)a.nD * N;
  const long long i0 = (long long)ti * JT, c0 = (long long)tj * JT;
  for (int e = t; e < JT * P; e += 256) {
    const int r = e / P, p = e % P;
    xr[r][p] = (i0 + r < N) ? a.X[(i0 + r) * P + p] : 0.0;
    xc[r][p] = (c0 + r < N) ? a.X[(c0 + r) * P + p] : 0.0;
  }
  __syncthreads();
  if (t < 2 * JT) {
    double (*xs)[P + 1] = t < JT ? xr : xc;
    const int r = t & (JT - 1);
    double xv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xv[p] = xs[r][p];
    xs[r][P] = sumsq<P>(xv);
  }
  __syncthreads();
  const int tx = t & 31, ty = t >> 5;                    // direct stores: columns 2 tx, 2 tx + 1; rows ty + 8 a
  const int ux = t & 15, uy = t >> 4;                    // transposed stores: columns 2 ux, 2 ux + 1 (rows of the half); rows uy + 16 b
  const bool diag = ti == tj;
  const bool vec = (N & 1) == 0;
  const long long NN = N * N;
  const long long c = c0 + 2 * tx;
  const bool okc0 = c < N, okc1 = c + 1 < N;
  double z0[P], z1[P];
#pragma unroll
  for (int p = 0; p < P; ++p) z0[p] = xc[2 * tx][p], z1[p] = xc[2 * tx + 1][p];
  const double zs0 = xc[2 * tx][P], zs1 = xc[2 * tx + 1][P];

  for (int half = 0; half < 2; ++half) {
    if (i0 + half * JH >= N) break;                      // (block-uniform)
    // ---- k_q and G_q of this thread's 8 entries, every latent
    double kk[QM][2 * JA], gg[QM][2 * JA];
#pragma unroll
    for (int q = 0; q < QM; ++q) {
      const bool live = q < a.Q;
      const double var = live ? a.var[q] : 0.0, ell = live ? a.ell[q] : 1.0;
      const double* Gq = a.G + (live ? q : 0) * NN;
#pragma unroll
      for (int s = 0; s < JA; ++s) {
        const int r = half * JH + ty + 8 * s;
        const long long i = i0 + r;
        double xv[P];
#pragma unroll
        for (int p = 0; p < P; ++p) xv[p] = xr[r][p];
        const double xsq = xr[r][P];
        // GPy's rounding order, as K_uu is built (both arguments passed): symmetric in (i, i') bit for bit, the diagonal exactly `var`
        const double r20 = rbf_r2<P>(xv, xsq, z0, zs0, ell), r21 = rbf_r2<P>(xv, xsq, z1, zs1, ell);
        kk[q][2 * s] = var * exp(-0.5 * r20);
        kk[q][2 * s + 1] = var * exp(-0.5 * r21);
        // only the lower triangle of G_q is read: the entry depends on the unordered pair {i, i'} alone
        const bool in0 = live && i < N && okc0, in1 = live && i < N && okc1;
        double g0 = 0.0, g1 = 0.0;
        if (!diag) {
          if (vec) {
            if (in0) {
              const f64x2 g = *reinterpret_cast<const f64x2*>(Gq + i * N + c);
              g0 = g[0], g1 = g[1];
            }
          } else {
            if (in0) g0 = Gq[i * N + c];
            if (in1) g1 = Gq[i * N + c + 1];
          }
        } else {
          if (in0) g0 = Gq[max(i, c) * N + min(i, c)];
          if (in1) g1 = Gq[max(i, c + 1) * N + min(i, c + 1)];
        }
        gg[q][2 * s] = g0, gg[q][2 * s + 1] = g1;
      }
    }
    // ---- every pair of functions from the same registers
    for (int j = 0; j < a.nD; ++j) {
      const int dj = a.d[j];
      for (int jp = 0; jp <= j; ++jp) {
        const int djp = a.d[jp];
        double v[2 * JA];
#pragma unroll
        for (int e = 0; e < 2 * JA; ++e) v[e] = 0.0;
#pragma unroll
        for (int q = 0; q < QM; ++q)
          if (q < a.Q) {
            const double ww = a.W[q * a.Df + dj] * a.W[q * a.Df + djp];
            const double ck = j == jp ? ww + a.kap[q * a.Df + dj] : ww;
#pragma unroll
            for (int e = 0; e < 2 * JA; ++e) v[e] = fma(ww, gg[q][e], fma(ck, kk[q][e], v[e]));
          }
        double* blk = a.cov + ((long long)j * N) * n + (long long)jp * N;     // block (j, j'), on or below the block diagonal
        double* blkT = a.cov + ((long long)jp * N) * n + (long long)j * N;    // block (j', j), its image
#pragma unroll
        for (int s = 0; s < JA; ++s) {
          const long long i = i0 + half * JH + ty + 8 * s;
          const bool oki = i < N;
          put2(blk + i * n + c, v[2 * s], v[2 * s + 1], vec, oki && okc0, oki && okc1);
          if (j != jp) put2(blkT + i * n + c, v[2 * s], v[2 * s + 1], vec, oki && okc0, oki && okc1);
        }
        if (!diag) {                                     // (block-uniform) the tile's mirror image: transposed through LDS
#pragma unroll
          for (int s = 0; s < JA; ++s) tr[ty + 8 * s][2 * tx] = v[2 * s], tr[ty + 8 * s][2 * tx + 1] = v[2 * s + 1];
          __syncthreads();
          const long long ci = i0 + half * JH + 2 * ux;  // output columns: rows of the half
          const bool ok0 = ci < N, ok1 = ci + 1 < N;
#pragma unroll
          for (int b = 0; b < JT / 16; ++b) {
            const int cT = uy + 16 * b;
            const long long ri = c0 + cT;                // output row: a column of the tile (always < N: tj < ti)
            const double w0 = tr[2 * ux][cT], w1 = tr[2 * ux + 1][cT];
            put2(blk + ri * n + ci, w0, w1, vec, ok0, ok1);
            if (j != jp) put2(blkT + ri * n + ci, w0, w1, vec, ok0, ok1);
          }
          __syncthreads();
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void joint_normal_kernel(unsigned long long seed, int S, long long n, double* __restrict__ Z,
                                                           const double* __restrict__ mean, double* __restrict__ F) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double mu = F ? mean[i] : 0.0;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    double z0, z1;
    normal_pair(seed, i, s, 0, z0, z1);
    Z[(long long)s * n + i] = z0;
    if (F) F[(long long)s * n + i] = mu;
  }
}

__global__ __launch_bounds__(256) void joint_gather_kernel(const double* __restrict__ m, int Df, const int* __restrict__ d, int nD,
                                                           long long N, long long i0, long long nrows, double* __restrict__ mean) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nrows) return;
  for (int j = blockIdx.y; j < nD; j += gridDim.y) mean[(long long)j * N + i0 + i] = m[i * Df + d[j]];
}

template <int P>
void launch_assemble_p(const JointArgs& a, dim3 grid, hipStream_t s) {
  if (a.Q <= 1) hipLaunchKernelGGL((joint_assemble_kernel<P, 1>), grid, dim3(256), 0, s, a);
  else if (a.Q <= 2) hipLaunchKernelGGL((joint_assemble_kernel<P, 2>), grid, dim3(256), 0, s, a);
  else if (a.Q <= 4) hipLaunchKernelGGL((joint_assemble_kernel<P, 4>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((joint_assemble_kernel<P, 8>), grid, dim3(256), 0, s, a);
}

}  // namespace

void launch_joint_assemble(const JointArgs& a, hipStream_t s) {
  if (a.N <= 0 || a.nD <= 0) return;
  if (a.Q < 1 || a.Q > HMOGP_MAXQ) throw HipError{hipErrorInvalidValue, "latent count must be 1..HMOGP_MAXQ", __FILE__, __LINE__};
  const unsigned tiles = (unsigned)((a.N + JT - 1) / JT);
  const dim3 grid(tiles, tiles);
  DISPATCH_P(a.P, launch_assemble_p<PP>(a, grid, s));
}

void launch_joint_normal(unsigned long long seed, int S, long long n, double* Z, const double* mean, double* F, hipStream_t s) {
  if (S <= 0 || n <= 0) return;
  hipLaunchKernelGGL(joint_normal_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)std::min(S, 1024)), dim3(256), 0, s, seed, S,
                     n, Z, mean, F);
}

void launch_joint_gather(const double* m, int Df, const int* d, int nD, long long N, long long i0, long long nrows, double* mean,
                         hipStream_t s) {
  if (nrows <= 0 || nD <= 0) return;
  hipLaunchKernelGGL(joint_gather_kernel, dim3((unsigned)((nrows + 255) / 256), (unsigned)std::min(nD, 1024)), dim3(256), 0, s, m,
                     Df, d, nD, N, i0, nrows, mean);
}
