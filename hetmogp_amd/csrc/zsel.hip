// zsel.hip -- inducing inputs chosen from the data by greedy conditional variance, i.e. pivoted incomplete Cholesky of K_ff under the
// sum kernel k = sum_q s2_q exp(-r_q^2 / 2) (gfx950; Burt, Rasmussen & van der Wilk 2020).  hmogp_select_inducing's body.
//
//   zsel_init_kernel   d_i = k0 for every row, and the per-block partials of (max d, smallest index attaining it) and of sum d
//   zsel_step_kernel   pick j: c_i = (k(x_i, x_p) - sum_{l<j} L_il L_pl) / sqrt(d_p) for every row, one accumulation chain over l per row;
//                      writes plane j of the factor, d_i = max(d_i - c_i^2, 0), d_p = 0, and the per-block partials.  HBM-bound reader:
//                      8 N j bytes of planes per pick, 16 B per lane and plane (a lane owns two neighbouring rows), eight plane loads in
//                      flight per lane; the multipliers L_pl are uniform across the grid and come from the compact vector lp.
//   zsel_pick_kernel   ONE block: folds the partials (trees, ties to the smallest index), writes trace, tests the stop rule, writes the
//                      next pivot and its d, and gathers lp for it.  Raises the device-side stop flag; launches after that return at once.
//
// Two launches per pick on one stream; no cooperative launch, no grid-wide barrier, no cross-block atomics, no host synchronisation in
// the pick loop.  Every loop is bounded by Mmax, by the row count of the launch, or by a compile-time constant.
//
// Sum d is a tree everywhere: the lane's two rows (1 addition), the wave's butterfly (6), the block's four waves (2), then the one
// block's halving tree over the nb = ceil(N / 512) partials (ceil(log2 nb)).  Longest addition path: 9 + ceil(log2 nb).
#include <algorithm>
#include <cmath>
#include <vector>

#include "engine_impl.h"
#include "rbf_device.h"
#include "zsel.h"

namespace {

constexpr int ZB = 256;             // threads per block of the row kernels
constexpr int ZROWS = 2 * ZB;       // rows per block: a lane owns rows 2 t, 2 t + 1
constexpr int ZU = 8;               // plane loads in flight per lane
constexpr int ZPB = 1024;           // threads of the one-block kernel
constexpr int ZCAP = 2048;          // partials folded in LDS; beyond that the first levels of the tree run in place in global memory

struct ZselKern {
  int Q;
  double var[HMOGP_MAXQ], ell[HMOGP_MAXQ];
};

struct ZselState {     // device-resident, written by the one-block kernel only
  int stop;            // raised once: every later launch returns at once
  int mout;
  long long p;         // pivot of the pick about to run
  double dp;           // d_p at the time of the pick
};

// k(x, z) = sum_q s2_q exp(-r_q^2 / 2), q from left to right, r_q^2 in GPy's rounding order; nothing contracted
template <int P>
__device__ __forceinline__ double zsel_k(const ZselKern& kn, const double* x, double xsq, const double* z, double zsq) {
#pragma clang fp contract(off)
  double k = kn.var[0] * exp(-0.5 * rbf_r2<P>(x, xsq, z, zsq, kn.ell[0]));
  for (int q = 1; q < kn.Q; ++q) k = k + kn.var[q] * exp(-0.5 * rbf_r2<P>(x, xsq, z, zsq, kn.ell[q]));
  return k;
}

__device__ __forceinline__ double zsel_downdate(double d, double c) {
#pragma clang fp contract(off)
  return fmax(d - c * c, 0.0);
}

// (m, ix) <- the larger d of the two, ties to the smaller index
__device__ __forceinline__ void zsel_best(double& m, long long& ix, double m2, long long ix2) {
  if (m2 > m || (m2 == m && ix2 < ix)) m = m2, ix = ix2;
}

// The block's partials from every lane's (max d, index, sum d): wave butterfly, then the four waves as (w0 + w1) + (w2 + w3).
__device__ __forceinline__ void zsel_block_partials(double m, long long ix, double s, double* __restrict__ pmax,
                                                    long long* __restrict__ pidx, double* __restrict__ psum) {
  __shared__ double wm[ZB / 64], ws[ZB / 64];
  __shared__ long long wi[ZB / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o, 64);
    const double m2 = __shfl_xor(m, o, 64);
    const long long i2 = __shfl_xor(ix, o, 64);
    zsel_best(m, ix, m2, i2);
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wm[w] = m, wi[w] = ix, ws[w] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double bm = wm[0];
    long long bi = wi[0];
#pragma unroll
    for (int k = 1; k < ZB / 64; ++k) zsel_best(bm, bi, wm[k], wi[k]);
    pmax[blockIdx.x] = bm, pidx[blockIdx.x] = bi, psum[blockIdx.x] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
  }
}

__global__ __launch_bounds__(ZB) void zsel_init_kernel(long long N, double k0, double* __restrict__ d, double* __restrict__ pmax,
                                                       long long* __restrict__ pidx, double* __restrict__ psum) {
  const long long i0 = ((long long)blockIdx.x * ZB + threadIdx.x) * 2;
  double m = -1.0, s = 0.0;
  long long ix = 0x7fffffffffffffffLL;
  if (i0 < N) {                                          // (N is rounded up to even in the row arrays: the pair is always in bounds)
    const double d1 = i0 + 1 < N ? k0 : 0.0;
    *reinterpret_cast<f64x2*>(d + i0) = f64x2{k0, d1};
    m = k0, ix = i0, s = k0 + d1;
  }
  zsel_block_partials(m, ix, s, pmax, pidx, psum);
}

template <int P>
__global__ __launch_bounds__(ZB) void zsel_step_kernel(const double* __restrict__ X, long long N, long long ldn, ZselKern kn, int j,
                                                       const ZselState* __restrict__ st, const double* __restrict__ lp,
                                                       const double* __restrict__ Lt, double* __restrict__ Lj, double* __restrict__ d,
                                                       double* __restrict__ pmax, long long* __restrict__ pidx,
                                                       double* __restrict__ psum) {
  if (st->stop) return;                                  // (grid-uniform)
  const long long p = st->p;
  const long long i0 = ((long long)blockIdx.x * ZB + threadIdx.x) * 2;
  double m = -1.0, s = 0.0;
  long long ix = 0x7fffffffffffffffLL;
  if (i0 < N) {
    const bool two = i0 + 1 < N;
    const long long i1 = two ? i0 + 1 : i0;
    double xp[P], x0[P], x1[P];
#pragma unroll
    for (int c = 0; c < P; ++c) xp[c] = X[p * P + c], x0[c] = X[i0 * P + c], x1[c] = X[i1 * P + c];
    const double xpsq = sumsq<P>(xp);
    const double k0v = zsel_k<P>(kn, x0, sumsq<P>(x0), xp, xpsq), k1v = zsel_k<P>(kn, x1, sumsq<P>(x1), xp, xpsq);
    // ---- the chain over l = 0 .. j-1, one per row; ZU planes in flight
    double s0 = 0.0, s1 = 0.0;
    const double* Lrow = Lt + i0;
    int l = 0;
    for (; l + ZU <= j; l += ZU) {
      f64x2 v[ZU];
#pragma unroll
      for (int u = 0; u < ZU; ++u) v[u] = *reinterpret_cast<const f64x2*>(Lrow + (long long)(l + u) * ldn);
#pragma unroll
      for (int u = 0; u < ZU; ++u) {
        const double mu = lp[l + u];
        s0 = fma(v[u][0], mu, s0), s1 = fma(v[u][1], mu, s1);
      }
    }
    for (; l < j; ++l) {
      const f64x2 v = *reinterpret_cast<const f64x2*>(Lrow + (long long)l * ldn);
      const double mu = lp[l];
      s0 = fma(v[0], mu, s0), s1 = fma(v[1], mu, s1);
    }
    const double rs = sqrt(st->dp);
    const double c0 = (k0v - s0) / rs, c1 = two ? (k1v - s1) / rs : 0.0;
    const f64x2 dd = *reinterpret_cast<const f64x2*>(d + i0);
    double d0 = zsel_downdate(dd[0], c0), d1 = two ? zsel_downdate(dd[1], c1) : 0.0;
    if (i0 == p) d0 = 0.0;
    if (i0 + 1 == p) d1 = 0.0;
    *reinterpret_cast<f64x2*>(Lj + i0) = f64x2{c0, c1};
    *reinterpret_cast<f64x2*>(d + i0) = f64x2{d0, d1};
    s = d0 + d1;
    m = d0, ix = i0;
    if (two && d1 > d0) m = d1, ix = i0 + 1;
  }
  zsel_block_partials(m, ix, s, pmax, pidx, psum);
}

// One level after the other of the halving tree: entry t takes entry t + h, h = ceil(n / 2).  Reads touch [h, n), writes [0, n - h).
__device__ __forceinline__ int zsel_fold_level(double* m, long long* ix, double* s, int n) {
  const int h = (n + 1) >> 1;
  for (int t = threadIdx.x; t + h < n; t += ZPB) {
    s[t] += s[t + h];
    zsel_best(m[t], ix[t], m[t + h], ix[t + h]);
  }
  __syncthreads();
  return h;
}

// After pick j (j = -1: after zsel_init_kernel): trace[j + 1], then pick j + 1 -- its pivot, the stop rule, dpiv, lp.
__global__ __launch_bounds__(ZPB) void zsel_pick_kernel(int j, int nb, int Mcap, int n_forced, const long long* __restrict__ forced,
                                                        double thr, long long ldn, const double* __restrict__ Lt,
                                                        const double* __restrict__ d, double* pmax, long long* pidx, double* psum,
                                                        ZselState* st, long long* __restrict__ pivots, double* __restrict__ dpiv,
                                                        double* __restrict__ trace, double* __restrict__ lp) {
  if (st->stop) return;
  __shared__ double sm[ZCAP], ss[ZCAP];
  __shared__ long long si[ZCAP];
  __shared__ long long next_p;
  int n = nb;
  for (int lvl = 0; lvl < 32 && n > ZCAP; ++lvl) n = zsel_fold_level(pmax, pidx, psum, n);
  for (int t = threadIdx.x; t < n; t += ZPB) sm[t] = pmax[t], si[t] = pidx[t], ss[t] = psum[t];
  __syncthreads();
  for (int lvl = 0; lvl < 32 && n > 1; ++lvl) n = zsel_fold_level(sm, si, ss, n);
  if (threadIdx.x == 0) {
    const int jn = j + 1;
    trace[jn] = ss[0];
    long long np = -1;
    if (jn >= Mcap) {
      st->mout = jn, st->stop = 1;
    } else {
      const long long p = jn < n_forced ? forced[jn] : si[0];
      const double dp = d[p];
      if (!(dp > thr)) {
        st->mout = jn, st->stop = 1;
      } else {
        pivots[jn] = p, dpiv[jn] = dp;
        st->p = p, st->dp = dp;
        np = p;
      }
    }
    next_p = np;
  }
  __syncthreads();
  const long long p = next_p;
  if (p < 0) return;
  for (int l = threadIdx.x; l <= j; l += ZPB) lp[l] = Lt[(long long)l * ldn + p];
}

[[noreturn]] void refuse(const std::string& msg) { throw EngineError{HMOGP_E_INVALID, "hmogp_select_inducing: " + msg}; }

}  // namespace

namespace hmogp_detail {

void select_inducing_check(int64_t N, int P, const double* X, int Q, const double* variance, const double* lengthscale, int Mmax, double tol,
                            int n_forced, const int64_t* forced, const int64_t* pivots, const double* Z, const double* dpiv,
                            const double* trace, const int32_t* Mout) {
  if (N < 1) refuse("N must be >= 1");
  if (P < 1 || P > 4) refuse("P must be 1..4");
  if (Q < 1 || Q > HMOGP_MAXQ) refuse("Q must be 1..8");
  if (Mmax < 1) refuse("Mmax must be >= 1");
  if (!X) refuse("X is NULL");
  if (!variance) refuse("variance is NULL");
  if (!lengthscale) refuse("lengthscale is NULL");
  if (!pivots) refuse("pivots is NULL");
  if (!Z) refuse("Z is NULL");
  if (!dpiv) refuse("dpiv is NULL");
  if (!trace) refuse("trace is NULL");
  if (!Mout) refuse("Mout is NULL");
  if (!(tol >= 0.0)) refuse("tol must be >= 0 (and not NaN)");
  if (n_forced < 0 || n_forced > Mmax) refuse("n_forced must be 0..Mmax");
  if (n_forced > 0 && !forced) refuse("forced is NULL with n_forced > 0");
  for (int q = 0; q < Q; ++q) {
    if (!(std::isfinite(variance[q]) && variance[q] > 0.0)) refuse("variance must be finite and > 0");
    if (!(std::isfinite(lengthscale[q]) && lengthscale[q] > 0.0)) refuse("lengthscale must be finite and > 0");
  }
  for (int64_t e = 0; e < N * P; ++e)
    if (!std::isfinite(X[e])) refuse("X has a non-finite entry");
  {
    std::vector<int64_t> f(forced, forced + n_forced);
    for (int64_t v : f)
      if (v < 0 || v >= N) refuse("forced index out of range");
    std::sort(f.begin(), f.end());
    if (std::adjacent_find(f.begin(), f.end()) != f.end()) refuse("forced index repeated");
  }
  if ((N + (N & 1) + ZROWS - 1) / ZROWS > 0x7fffffffLL) refuse("N is too large for one launch");
}

void select_inducing_run(int64_t N, int P, const double* X, int Q, const double* variance, const double* lengthscale, int Mmax, double tol,
                         int n_forced, const int64_t* forced, int64_t* pivots, double* Z, double* dpiv, double* trace, double* L, double* d,
                         int32_t* Mout) {
  const long long ldn = N + (N & 1);                     // leading dimension of the planes: N rounded up to even (16-byte pairs)
  const int nb = (int)((ldn + ZROWS - 1) / ZROWS);
  const int Mcap = (int)std::min<int64_t>(Mmax, N);      // no more picks than rows: pick N would find every d at 0
  ZselKern kn;
  kn.Q = Q;
  double k0 = variance[0];
  for (int q = 0; q < HMOGP_MAXQ; ++q) kn.var[q] = q < Q ? variance[q] : 0.0, kn.ell[q] = q < Q ? lengthscale[q] : 1.0;
  for (int q = 1; q < Q; ++q) k0 = k0 + variance[q];
  const double thr = std::max(tol, HMOGP_ZSEL_FLOOR) * k0;

  // ---- the memory question: before any allocation
  const double need = 8.0 * (double)ldn * Mcap + 8.0 * (double)N * P + 8.0 * (double)ldn + 24.0 * nb + 8.0 * (3.0 * Mcap + 1.0 + n_forced) + 64.0;
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > (double)free_b) {
    char buf[256];
    std::snprintf(buf, sizeof buf, "the factor (8 N Mmax bytes) and the row arrays need %.0f bytes, the device has %.0f free", need,
                  (double)free_b);
    refuse(buf);
  }
  DevBuf dX, dLt, dd, dpm, dpi, dps, dst, dpv, ddp, dtr, dlp, dfo;
  dX.ensure(sizeof(double) * N * P), dLt.ensure(sizeof(double) * ldn * Mcap), dd.ensure(sizeof(double) * ldn);
  dpm.ensure(sizeof(double) * nb), dpi.ensure(sizeof(long long) * nb), dps.ensure(sizeof(double) * nb);
  dst.ensure(sizeof(ZselState), true), dpv.ensure(sizeof(long long) * Mcap), ddp.ensure(sizeof(double) * Mcap);
  dtr.ensure(sizeof(double) * (Mcap + 1)), dlp.ensure(sizeof(double) * Mcap), dfo.ensure(sizeof(long long) * std::max(n_forced, 1));
  HIP_TRY(hipMemcpy(dX.p, X, sizeof(double) * N * P, hipMemcpyHostToDevice));
  if (n_forced > 0) HIP_TRY(hipMemcpy(dfo.p, forced, sizeof(long long) * n_forced, hipMemcpyHostToDevice));
  static_assert(sizeof(long long) == sizeof(int64_t), "pivots are int64");

  // ---- init, then two launches per pick; nothing on the host waits inside the loop
  hipStream_t s = nullptr;
  ZselState* st = dst.as<ZselState>();
  hipLaunchKernelGGL(zsel_init_kernel, dim3(nb), dim3(ZB), 0, s, (long long)N, k0, dd.d(), dpm.d(), dpi.as<long long>(), dps.d());
  for (int j = -1; j < Mcap; ++j) {
    if (j >= 0) {
      DISPATCH_P(P, hipLaunchKernelGGL((zsel_step_kernel<PP>), dim3(nb), dim3(ZB), 0, s, dX.d(), (long long)N, ldn, kn, j, st, dlp.d(),
                                       dLt.d(), dLt.d() + (long long)j * ldn, dd.d(), dpm.d(), dpi.as<long long>(), dps.d()));
    }
    hipLaunchKernelGGL(zsel_pick_kernel, dim3(1), dim3(ZPB), 0, s, j, nb, Mcap, n_forced, dfo.as<long long>(), thr, ldn, dLt.d(), dd.d(),
                       dpm.d(), dpi.as<long long>(), dps.d(), st, dpv.as<long long>(), ddp.d(), dtr.d(), dlp.d());
  }
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());

  // ---- results
  ZselState hs;
  HIP_TRY(hipMemcpy(&hs, dst.p, sizeof hs, hipMemcpyDeviceToHost));
  const int M = hs.mout;
  if (!hs.stop || M < 0 || M > Mcap) throw EngineError{HMOGP_E_STATE, "hmogp_select_inducing: the pick loop did not finish"};
  *Mout = M;
  std::fill(pivots, pivots + Mmax, (int64_t)-1);
  std::fill(dpiv, dpiv + Mmax, 0.0);
  std::fill(trace, trace + Mmax + 1, 0.0);
  std::fill(Z, Z + (long long)Mmax * P, 0.0);
  if (M > 0) {
    HIP_TRY(hipMemcpy(pivots, dpv.p, sizeof(int64_t) * M, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(dpiv, ddp.p, sizeof(double) * M, hipMemcpyDeviceToHost));
  }
  HIP_TRY(hipMemcpy(trace, dtr.p, sizeof(double) * (M + 1), hipMemcpyDeviceToHost));
  for (int jj = 0; jj < M; ++jj) std::copy(X + pivots[jj] * P, X + (pivots[jj] + 1) * P, Z + (long long)jj * P);
  if (d) {
    std::vector<double> hd(ldn);
    HIP_TRY(hipMemcpy(hd.data(), dd.p, sizeof(double) * ldn, hipMemcpyDeviceToHost));
    std::copy(hd.begin(), hd.begin() + N, d);
  }
  if (L) {                                               // planes -> rows; columns at Mout and beyond are zero
    std::fill(L, L + (long long)N * Mmax, 0.0);
    std::vector<double> plane(ldn);
    for (int l = 0; l < M; ++l) {
      HIP_TRY(hipMemcpy(plane.data(), dLt.d() + (long long)l * ldn, sizeof(double) * ldn, hipMemcpyDeviceToHost));
      for (long long i = 0; i < N; ++i) L[i * Mmax + l] = plane[i];
    }
  }
}

}  // namespace hmogp_detail
