// kuf.hip -- the cross-covariance writer of the row pass and its exact-zero windows (gfx950).
//
//   rbf_cross_cov   K^[n,m] = s2 exp(-r2/2)          HBM-bound writer (N*M*8 B), util.py:145-164 / GPy RBF.K
//   windows         per 128-row tile / 128-column block, the range outside which K^ is exactly 0.0
// Declarations: rowpass.h.
#include <type_traits>

#include "rowpass.h"
#include "rbf_device.h"

namespace {

constexpr int RBF_ROWS = 32;  // rows per block; 256 threads x 2 columns = 512 columns per block

// EXACT = GPy's rounding order r = sqrt(clip(r2))/l; K = s2 exp(-0.5 r*r)   (used for K_uu, whose inverse amplifies
// rounding);  !EXACT = s2 exp(-0.5 clip(r2) * (1/l^2)): no sqrt / divide per element -- the K_uf kernel is otherwise bound
// by the FP64 VALU (sqrt + divide cost as much as the exp), not by HBM.  The two differ by <= 2 ulp of the exponent.
template <int P, bool EXACT>
__global__ __launch_bounds__(256) void rbf_kernel(const double* __restrict__ X, int ldx, long long N,
                                                  const double* __restrict__ Z, int ldz, int M, double var, double ell,
                                                  double* __restrict__ K, int same, const int* __restrict__ rowwin,
                                                  RbfBatch bt) {
  if (bt.var) {  // batched over the latents (grid.z): per-latent inducing block, hyper-parameters, output and windows
    const int q = blockIdx.z;
    X += (long long)q * bt.sX;
    Z += (long long)q * bt.sZ;
    K += (long long)q * bt.sK;
    var = bt.var[q], ell = bt.ell[q];
    if (rowwin) rowwin += (long long)q * bt.sWin;
  }
  __shared__ double xs[RBF_ROWS][P + 1];
  const int t = threadIdx.x;
  const long long n0 = (long long)blockIdx.x * RBF_ROWS;
  const int c = blockIdx.y * 512 + 2 * t;
  for (int e = t; e < RBF_ROWS * P; e += 256) {
    const int r = e / P, p = e % P;
    xs[r][p] = (n0 + r < N) ? X[(n0 + r) * ldx + p] : 0.0;
  }
  __syncthreads();
  if (t < RBF_ROWS) {
    double xv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xv[p] = xs[t][p];
    xs[t][P] = sumsq<P>(xv);
  }
  __syncthreads();
  if (c >= M) return;
  if (rowwin) {  // exact-zero windows: a wave owns one 128-column block; skip it if no consumer will read it
    const int T = (int)(n0 >> 7), cb0 = (c >> 7) << 7;
    if (cb0 >= rowwin[2 * T + 1] || cb0 + 128 <= rowwin[2 * T]) return;
  }
  const bool two = (c + 1) < M;
  double z0[P], z1[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    z0[p] = Z[(long long)c * ldz + p];
    z1[p] = two ? Z[(long long)(c + 1) * ldz + p] : 0.0;
  }
  const double zs0 = sumsq<P>(z0), zs1 = sumsq<P>(z1);
  const bool vec = two && ((M & 1) == 0);
  const int nr = (int)min((long long)RBF_ROWS, N - n0);
  // (the row loop is instantiated for the vector-store and the scalar-store case: no per-row branch on a loop-invariant condition)
  auto rows = [&](auto vec_c) {
    constexpr bool VEC = decltype(vec_c)::value;
    for (int r = 0; r < nr; ++r) {
      double xv[P];
#pragma unroll
      for (int p = 0; p < P; ++p) xv[p] = xs[r][p];
      const double xsq = xs[r][P];
      double r20, r21;
      if (EXACT) {
        r20 = rbf_r2<P>(xv, xsq, z0, zs0, ell), r21 = rbf_r2<P>(xv, xsq, z1, zs1, ell);
      } else {
        const double il2 = 1.0 / (ell * ell);
        r20 = rbf_r2_fast<P>(xv, xsq, z0, zs0, il2), r21 = rbf_r2_fast<P>(xv, xsq, z1, zs1, il2);
      }
      if (EXACT && same) {  // GPy's X2=None branch forces the diagonal distance to 0 (kern/stationary; K_uu-side calls only)
        if (n0 + r == c) r20 = 0.0;
        if (n0 + r == c + 1) r21 = 0.0;
      }
      // exp(-r2/2) underflows to exactly 0.0 beyond r2 ~ 1490.3: a wave whose 128 columns are all past that writes the
      // zeros without evaluating the exponential (same values; NaNs fail the comparison and take the full path)
      double k0 = 0.0, k1 = 0.0;
      if (!__all(r20 > 1492.0 && r21 > 1492.0)) k0 = var * exp(-0.5 * r20), k1 = var * exp(-0.5 * r21);
      double* out = K + (n0 + r) * M + c;
      if (VEC)
        *reinterpret_cast<f64x2*>(out) = f64x2{k0, k1};
      else {
        out[0] = k0;
        if (two) out[1] = k1;
      }
    }
  };
  if (vec) rows(std::true_type{});
  else rows(std::false_type{});
}

// ---- exact-zero windows ----------------------------------------------------------------------------------------
// K^[n][m] = s2 exp(-r2/2) is EXACTLY 0.0 in float64 once r2 > ~1490.3 (exp underflows below the smallest subnormal).
// For spatially sorted inputs K^ is therefore banded, and every product the row pass forms with an entry outside the
// band is a product with an exact zero.  window_kernel finds, per 128-row tile, the column range [lo, hi) that holds all
// possibly-nonzero entries (distance to the tile's bounding box <= sqrt(1491) lengthscales: a superset), and per
// 128-column block the hull of the row tiles that touch it;
// window_fix_kernel falls back to full ranges when the data is not banded (a row tile inside a block's hull that does not
// touch the block), so arbitrary inputs stay correct.  No host synchronisation is involved.
constexpr double WINDOW_R2_MAX = 1491.0;

__global__ void window_init_kernel(int* __restrict__ colwin, int ncb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ncb) {
    colwin[2 * i] = 0x7fffffff;
    colwin[2 * i + 1] = 0;
  }
}

template <int P>
__global__ __launch_bounds__(256) void window_kernel(const double* __restrict__ X, long long N, const double* __restrict__ Z,
                                                     int ldz, int M, double ell, int* __restrict__ rowwin,
                                                     int* __restrict__ colwin, unsigned char* __restrict__ hit, int ncb) {
  // A column m can hold a non-zero for some row of this 128-row tile only if z_m is within sqrt(1491) lengthscales of the
  // tile's bounding box (per-dimension [min, max] of its inputs): a conservative test costing O(M) per tile.  Sorted
  // 1-D inputs give tight boxes (narrow windows); unsorted inputs give boxes spanning the domain (full windows).
  __shared__ double bmin[P], bmax[P];
  __shared__ double red[2][4][P];
  __shared__ int s_lo, s_hi;
  __shared__ int s_hit[64];
  const int t = threadIdx.x, T = blockIdx.x, lane = t & 63, w = t >> 6;
  const long long r0 = (long long)T * 128;
  const int nr = (int)min(128LL, N - r0);
  if (t == 0) s_lo = 0x7fffffff, s_hi = 0;
  if (t < 64) s_hit[t] = 0;
  double lo[P], hi[P];
#pragma unroll
  for (int p = 0; p < P; ++p) lo[p] = INFINITY, hi[p] = -INFINITY;
  bool nan_in = false;
  if (t < nr) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const double x = X[(r0 + t) * P + p];
      lo[p] = hi[p] = x;
      nan_in |= (x != x);
    }
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      lo[p] = fmin(lo[p], __shfl_xor(lo[p], o, 64));
      hi[p] = fmax(hi[p], __shfl_xor(hi[p], o, 64));
    }
    if (lane == 0) red[0][w][p] = lo[p], red[1][w][p] = hi[p];
  }
  const bool any_nan = __syncthreads_or(nan_in ? 1 : 0) != 0;
  if (t == 0) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      bmin[p] = fmin(fmin(red[0][0][p], red[0][1][p]), fmin(red[0][2][p], red[0][3][p]));
      bmax[p] = fmax(fmax(red[1][0][p], red[1][1][p]), fmax(red[1][2][p], red[1][3][p]));
    }
  }
  __syncthreads();
  const double thr = WINDOW_R2_MAX * ell * ell * (1.0 + 1e-9);
  for (int m = t; m < M; m += 256) {
    double d2 = 0.0;
    bool zn = false;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      const double z = Z[(long long)m * ldz + p];
      zn |= (z != z);
      const double d = fmax(fmax(bmin[p] - z, z - bmax[p]), 0.0);  // distance from z to the box along dimension p
      d2 += d * d;
    }
    if (any_nan || zn || !(d2 > thr)) {  // NaNs count as "possibly non-zero"
      atomicMin(&s_lo, m);
      atomicMax(&s_hi, m + 1);
      s_hit[m >> 7] = 1;
    }
  }
  __syncthreads();
  if (t == 0) {
    const bool none = s_hi == 0;
    rowwin[2 * T] = none ? 0 : (s_lo & ~15);
    rowwin[2 * T + 1] = none ? 0 : min((s_hi + 15) & ~15, (M + 15) & ~15);
  }
  if (t < ncb) {
    hit[(long long)T * ncb + t] = (unsigned char)s_hit[t];
    if (s_hit[t]) {
      atomicMin(&colwin[2 * t], (int)r0);
      atomicMax(&colwin[2 * t + 1], (int)(r0 + nr));
    }
  }
}

__global__ __launch_bounds__(256) void window_fix_kernel(int* __restrict__ rowwin, int* __restrict__ colwin,
                                                         const unsigned char* __restrict__ hit, int tiles, int ncb, int M,
                                                         long long N) {
  __shared__ int viol;
  const int t = threadIdx.x;
  if (t == 0) viol = 0;
  __syncthreads();
  for (int cb = 0; cb < ncb; ++cb) {
    const int lo = colwin[2 * cb], hi = colwin[2 * cb + 1];
    if (lo == 0x7fffffff) continue;
    for (int T = (lo >> 7) + t; T < (hi + 127) >> 7; T += 256)
      if (!hit[(long long)T * ncb + cb]) viol = 1;
  }
  __syncthreads();
  if (viol) {  // not banded: dense ranges everywhere
    for (int T = t; T < tiles; T += 256) {
      rowwin[2 * T] = 0;
      rowwin[2 * T + 1] = (M + 15) & ~15;
    }
    for (int cb = t; cb < ncb; cb += 256) {
      colwin[2 * cb] = 0;
      colwin[2 * cb + 1] = (int)N;
    }
  } else {
    for (int cb = t; cb < ncb; cb += 256)
      if (colwin[2 * cb] == 0x7fffffff) colwin[2 * cb] = 0, colwin[2 * cb + 1] = 0;
  }
}

}  // namespace

void launch_windows(const double* X, long long N, int P, const double* Z, int ldz, int M, double ell, int* rowwin, int* colwin,
                    unsigned char* hit, hipStream_t s) {
  if (N <= 0) return;
  const int tiles = (int)((N + 127) / 128), ncb = (M + 127) / 128;
  if (ncb > 64) throw HipError{hipErrorInvalidValue, "exact-zero windows support M <= 8192", __FILE__, __LINE__};
  hipLaunchKernelGGL(window_init_kernel, dim3(1), dim3(64), 0, s, colwin, ncb);
  DISPATCH_P(P, hipLaunchKernelGGL((window_kernel<PP>), dim3(tiles), dim3(256), 0, s, X, N, Z, ldz, M, ell, rowwin, colwin, hit,
                                   ncb));
  hipLaunchKernelGGL(window_fix_kernel, dim3(1), dim3(256), 0, s, rowwin, colwin, hit, tiles, ncb, M, N);
}

void launch_rbf(const double* X, int ldx, long long N, int P, const double* Z, int ldz, int M, double var, double ell,
                double* K, bool same, hipStream_t s, const int* rowwin, bool exact, const RbfBatch* batch) {
  if (N <= 0 || M <= 0) return;
  RbfBatch bt = batch ? *batch : RbfBatch{};
  dim3 grid((unsigned)((N + RBF_ROWS - 1) / RBF_ROWS), (M + 511) / 512, batch ? batch->nq : 1);
  if (exact) {
    DISPATCH_P(P, hipLaunchKernelGGL((rbf_kernel<PP, true>), grid, dim3(256), 0, s, X, ldx, N, Z, ldz, M, var, ell, K,
                                     same ? 1 : 0, rowwin, bt));
  } else {
    DISPATCH_P(P, hipLaunchKernelGGL((rbf_kernel<PP, false>), grid, dim3(256), 0, s, X, ldx, N, Z, ldz, M, var, ell, K,
                                     same ? 1 : 0, rowwin, bt));
  }
}
