// rowpass.hip -- what streams the row pass's N x M data besides K_uf (kuf.hip), the quadrature (quad.hip) and the two FP64-MFMA
// contractions (gemm_f64.hip):
//
//   colstats        r = K^T alpha, dZ numerators = colsum(E^ .* (x - z))                     (reads K^, P~ once)
//   reducers        deterministic two-level sums (block partials -> bundle), no floating-point atomics
//   mirror / wire   the statistic bundle's symmetric halves and its wire format; the raw-gradient debug export
// (row statistics p = K^ a, c = rowsum(P~ .* K^) ... are fused into the forward contraction's epilogue, gemm_f64.hip)
#include <algorithm>

#include "rowpass.h"
#include "rbf_device.h"

namespace {

// ---- colstats: thread = 2 columns, block = 512 columns x `rows` rows ----------------------------------------
// STRICT (HMOGP_CFG_STRICT_QF only): r = A^T alpha from a second matrix and quirk Q10's r == 0 gating -- kept out of the hot-path
// instantiation, which has to fit 64 registers to run beside the Gram.
// [r6] WIN = false (no exact-zero windows: the default): the row loop's bounds are the same for every lane, so what a row contributes
// besides its K^ / P~ entries -- alpha, alpha0, beta0 and the input x_n -- is WAVE-UNIFORM.  Read through the constant address
// space at uniform addresses those values arrive in SGPRs (s_load; v_fma_f64 takes an SGPR pair as a source) instead of being
// broadcast into 6 + 2 P vector registers per lane: P = 2 ... 4 fit their 64 registers without a spill (2 - 64 spilled before; P = 2
// is BASELINE config 5's path: column statistics 7.6 -> 4.6 ms per step there).  WIN = true keeps the per-lane bounds and vector
// loads: the windows mode, and P = 1, which never spilled and is 10 % faster with them (launch_colstats).
#define HM_CONST(p) ((const __attribute__((address_space(4))) double*)(uintptr_t)(p))
template <int P, bool STRICT, bool SL, bool WIN>
__global__ __launch_bounds__(256, 8) void colstats_kernel(const double* __restrict__ Kh, const double* __restrict__ Pt,
                                                       const double* __restrict__ a, const double* __restrict__ alpha,
                                                       const double* __restrict__ alpha0, const double* __restrict__ beta0,
                                                       const double* __restrict__ X, const double* __restrict__ Z, int ldz,
                                                       long long N, int M, int rows, int want_z,
                                                       double* __restrict__ partials, const int* __restrict__ colwin,
                                                       ColBatch bt, const double* __restrict__ Ar, const double* __restrict__ ell) {
  {  // batched over the latents (grid.z)
    const long long q = blockIdx.z;
    if (STRICT) Ar += q * bt.sK;
    Kh += q * bt.sK, Pt += q * bt.sK, a += q * bt.sA, alpha += q * bt.sV, alpha0 += q * bt.sV, beta0 += q * bt.sV;
    Z += q * bt.sZ, partials += q * bt.sPart;
    if (colwin) colwin += q * bt.sWin;
  }
  const int t = threadIdx.x, c = blockIdx.x * 512 + 2 * t;
  if (c >= M) return;
  const bool two = (c + 1) < M;
  const bool vec = two && ((M & 1) == 0);
  double z0[P], z1[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    z0[p] = Z[(long long)c * ldz + p];
    z1[p] = two ? Z[(long long)(c + 1) * ldz + p] : 0.0;
  }
  const double a0 = a[c], a1 = two ? a[c + 1] : 0.0;
  const double zs0 = STRICT ? sumsq<P>(z0) : 0.0, zs1 = STRICT ? sumsq<P>(z1) : 0.0;
  // [r5] ell != nullptr: also  s2[m] = sum_n E_nm |x_n - z_m|^2 / l^2  -- the r2-weighted statistic behind the lengthscale gradient
  // (sl = sum_m s2[m]; svmogp.py:140 -> GPy update_gradients_full).  It used to be carried by the forward contraction's epilogue
  // as two more row statistics (p~, c~) with the distances recomputed per element there; E_nm and x_n - z_m are in hand here.
  const bool want_e = want_z || SL;
  // A block takes the row splits blockIdx.y, blockIdx.y + gridDim.y, ...: the grid may be CAPPED (launch_colstats) so that
  // this HBM-bound pass occupies only a few CU slots at a time beside the FP64-MFMA Gram it runs next to -- a block that
  // holds half a CU while it waits for HBM keeps a Gram block (whose registers fill the other half) from being scheduled.
  const long long nsplit = (N + rows - 1) / rows;
  for (long long sp = blockIdx.y; sp < nsplit; sp += gridDim.y) {
    long long n0 = sp * rows, n1 = min(N, n0 + rows);
    if (WIN && colwin) {  // rows outside the exact-zero window of this 128-column block contribute exact zeros
      n0 = max(n0, (long long)colwin[2 * (c >> 7)]);
      n1 = min(n1, (long long)colwin[2 * (c >> 7) + 1]);
    }
    double r0 = 0.0, r1 = 0.0, d0[P], d1[P], s20 = 0.0, s21 = 0.0;
#pragma unroll
    for (int p = 0; p < P; ++p) d0[p] = d1[p] = 0.0;
    for (long long n = n0; n < n1; ++n) {
      double k0, k1, q0 = 0.0, q1 = 0.0;
      if (vec) {
        const f64x2 kv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(Kh + n * M + c));
        k0 = kv.x, k1 = kv.y;
        if (want_e) {
          const f64x2 qv = __builtin_nontemporal_load(reinterpret_cast<const f64x2*>(Pt + n * M + c));
          q0 = qv.x, q1 = qv.y;
        }
      } else {
        k0 = Kh[n * M + c];
        k1 = two ? Kh[n * M + c + 1] : 0.0;
        if (want_e) {
          q0 = Pt[n * M + c];
          q1 = two ? Pt[n * M + c + 1] : 0.0;
        }
      }
      const double al = WIN ? alpha[n] : HM_CONST(alpha)[n];
      if (STRICT) {   // strict q(f): r = A^T alpha with A = K^ Kuu^-1 (dVE_dmu of svmogp_inf.py:144 as the reference forms it)
        r0 += Ar[n * M + c] * al;
        r1 += (two ? Ar[n * M + c + 1] : 0.0) * al;
      } else {
        r0 += k0 * al;
        r1 += k1 * al;
      }
      if (want_e) {
        const double al0 = WIN ? alpha0[n] : HM_CONST(alpha0)[n], be0 = 2.0 * (WIN ? beta0[n] : HM_CONST(beta0)[n]);
        double e0 = (al0 * a0 + be0 * q0) * k0, e1 = (al0 * a1 + be0 * q1) * k1;
        // Quirk Q10 (STRICT only): GPy's gradients_X drops the entries whose COMPUTED distance -- the expanded form |x|^2 + |z|^2 -
        // 2 x.z, clipped -- is exactly 0.  That needs |x - z|^2 below a few ulp of |z|^2: un-centred inputs, or, at 1e6 rows per
        // task, the odd row within 1.5e-8 |z| of an inducing point (one such row in the full-size C4 test: 4e-8 of one g_Z entry).
        // The default path keeps those terms (they are the mathematically correct ones): an in-loop test, even behind a cheap
        // pre-test, costs this kernel 16 spilled registers -- and it has to fit 64 to run beside the Gram.
        double g20 = 0.0, g21 = 0.0;     // STRICT: GPy's clipped expanded-form squared distances (unscaled)
        if (STRICT) {
          double xv[P];
#pragma unroll
          for (int p = 0; p < P; ++p) xv[p] = WIN ? X[n * P + p] : HM_CONST(X)[n * P + p];
          const double xsq = sumsq<P>(xv);
          g20 = rbf_r2_fast<P>(xv, xsq, z0, zs0, 1.0), g21 = rbf_r2_fast<P>(xv, xsq, z1, zs1, 1.0);
          if (g20 == 0.0) e0 = 0.0;
          if (g21 == 0.0) e1 = 0.0;
        }
        double q20 = 0.0, q21 = 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) {
          const double x = WIN ? X[n * P + p] : HM_CONST(X)[n * P + p];
          const double dx0 = x - z0[p], dx1 = x - z1[p];
          d0[p] += e0 * dx0;
          d1[p] += e1 * dx1;
          if (SL) q20 += dx0 * dx0, q21 += dx1 * dx1;
        }
        // [r6] strict q(f): the r2 weight of the lengthscale statistic in GPy's OWN form -- |x|^2 + |z|^2 - 2 x.z, clipped
        // (stationary.py `_unscaled_dist`): with un-centred inputs that form loses digits the reference's gradient carries
        // (lad_c1_offset_rung1) -- instead of sum_p (x_p - z_p)^2.  Replaces the r2-weighted twins of strict_rowstats_kernel.
        if (SL) s20 += e0 * (STRICT ? g20 : q20), s21 += e1 * (STRICT ? g21 : q21);
      }
    }
    // partial layout per row-split: [ r (M) | dZ (M*P) | s2 (M) ]
    double* out = partials + sp * ((long long)M * (2 + P));
    const double il2 = ell ? 1.0 / (ell[blockIdx.z] * ell[blockIdx.z]) : 0.0;   // (scaled once per split, not per element)
    out[(long long)M * (1 + P) + c] = s20 * il2;
    if (two) out[(long long)M * (1 + P) + c + 1] = s21 * il2;
    out[c] = r0;
    if (two) out[c + 1] = r1;
#pragma unroll
    for (int p = 0; p < P; ++p) {
      out[M + (long long)c * P + p] = d0[p];
      if (two) out[M + (long long)(c + 1) * P + p] = d1[p];
    }
  }
}

// ---- reducers ---------------------------------------------------------------------------------------------
// dst[off[k]] += sum_b partials[b*len + k]   (off == nullptr: dst[k])
__global__ __launch_bounds__(256) void reduce_rows_kernel(const double* __restrict__ partials, long long nrows, int len,
                                                          const long long* __restrict__ off, double* __restrict__ dst,
                                                          int accumulate) {
  __shared__ double scratch[16];
  const int k = blockIdx.x;
  double s = 0.0;
  for (long long b = threadIdx.x; b < nrows; b += blockDim.x) s += partials[b * len + k];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) {
    double* d = dst + (off ? off[k] : k);
    *d = accumulate ? (*d + s) : s;
  }
}
// dst[i] (+)= sum_s slabs[s*stride + i], i < len.  Block = 16 columns x 16 slab lanes: thread (c, g) sums the slabs
// g, g+16, ... of column c (independent loads, 128-byte segments), the 16 partial sums are added in a fixed order.
__global__ __launch_bounds__(256) void reduce_slabs_kernel(const double* __restrict__ slabs, int nslabs, long long stride,
                                                           long long len, double* __restrict__ dst, int accumulate,
                                                           long long sSlabs, long long sDst) {
  __shared__ double part[16][17];
  const int c = threadIdx.x & 15, g = threadIdx.x >> 4;
  const long long i = (long long)blockIdx.x * 16 + c;
  slabs += (long long)blockIdx.y * sSlabs;
  dst += (long long)blockIdx.y * sDst;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (i < len) {
    int b = g;
    for (; b + 48 < nslabs; b += 64) {
      s0 += slabs[b * stride + i];
      s1 += slabs[(b + 16) * stride + i];
      s2 += slabs[(b + 32) * stride + i];
      s3 += slabs[(b + 48) * stride + i];
    }
    for (; b < nslabs; b += 16) s0 += slabs[b * stride + i];
  }
  part[g][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && i < len) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += part[k][c];
    dst[i] = accumulate ? dst[i] + s : s;
  }
}
// dst[i][j] (+)= sum_s slabs[s][i][j] over the LOWER 128 x 128 tiles only (the Gram product never writes the others)
__global__ __launch_bounds__(256) void reduce_slabs_lower_kernel(const double* __restrict__ slabs, int nslabs, int M,
                                                                 double* __restrict__ dst, int accumulate, long long sSlabs,
                                                                 long long sDst) {
  slabs += (long long)blockIdx.z * sSlabs;
  dst += (long long)blockIdx.z * sDst;
  int v = blockIdx.x, ti = (int)((sqrt(8.0 * (double)v + 1.0) - 1.0) * 0.5);
  while ((ti + 1) * (ti + 2) / 2 <= v) ++ti;
  while (ti * (ti + 1) / 2 > v) --ti;
  const int tj = v - ti * (ti + 1) / 2;
  const long long MM = (long long)M * M;
  const int c2 = (threadIdx.x & 63) * 2, r4 = threadIdx.x >> 6;  // 64 lanes x 2 columns; block = 4 rows (blockIdx.y)
  const int col = tj * 128 + c2;
  if (col >= M) return;
  const bool two = col + 1 < M, vec = two && ((M & 1) == 0);
  {
    const int row = ti * 128 + blockIdx.y * 4 + r4;
    if (row >= M) return;
    const long long off = (long long)row * M + col;
    double s0 = 0.0, s1 = 0.0;
    for (int b = 0; b < nslabs; ++b) {
      if (vec) {
        const f64x2 x = *reinterpret_cast<const f64x2*>(slabs + b * MM + off);
        s0 += x.x, s1 += x.y;
      } else {
        s0 += slabs[b * MM + off];
        if (two) s1 += slabs[b * MM + off + 1];
      }
    }
    dst[off] = accumulate ? dst[off] + s0 : s0;
    if (two) dst[off + 1] = accumulate ? dst[off + 1] + s1 : s1;
  }
}
// lower tiles of H were computed: mirror to the upper triangle
__global__ void mirror_lower_kernel(double* __restrict__ A, int M, long long stride) {
  double* a = A + (long long)blockIdx.z * stride;
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c < M && c > r) a[(long long)r * M + c] = a[(long long)c * M + r];
}

// Wire format of the statistic bundle (what a multi-GPU run all-reduces): H_q is symmetric and the row pass only fills its
// lower triangle, so only that triangle travels -- [head NG | per q: tril(H_q) row-major packed (M(M+1)/2) | tail (per_q - M*M)].
// dir 0: bundle -> wire, dir 1: wire -> bundle (lower triangle; hmogp_step_finish mirrors it).
__global__ void wire_tri_kernel(double* __restrict__ bundle_q0, double* __restrict__ wire_q0, int M, long long per_q,
                                long long wire_per_q, int dir) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
  if (c > r) return;
  double* h = bundle_q0 + (long long)blockIdx.z * per_q + (long long)r * M + c;
  double* w = wire_q0 + (long long)blockIdx.z * wire_per_q + (long long)r * (r + 1) / 2 + c;
  if (dir == 0) *w = *h;
  else *h = *w;
}
// head (q == gridDim.y - 1 ... see launcher) and per-latent tails
__global__ void wire_rest_kernel(double* __restrict__ bundle, double* __restrict__ wire, long long NG, long long MM,
                                 long long Mtri, long long per_q, long long wire_per_q, int Q, int dir) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long tail = per_q - MM;
  if (i < NG) {
    if (dir == 0) wire[i] = bundle[i];
    else bundle[i] = wire[i];
    return;
  }
  const long long k = i - NG;
  if (k >= tail * Q) return;
  const long long q = k / tail, e = k - q * tail;
  double* b = bundle + NG + q * per_q + MM + e;
  double* w = wire + NG + q * wire_per_q + Mtri + e;
  if (dir == 0) *w = *b;
  else *b = *w;
}

__global__ void raw_kmn_kernel(const double* __restrict__ a, const double* __restrict__ gm, const double* __restrict__ gv,
                               int J, int j, double w, const double* __restrict__ Pt, int M, long long N,
                               double* __restrict__ out) {
  const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int m = blockIdx.y;
  if (n >= N) return;
  out[(long long)m * N + n] = a[m] * gm[n * J + j] + 2.0 * w * (gv[n * J + j] * Pt[n * M + m]);
}

}  // namespace

void launch_colstats(const double* Kh, const double* Pt, const double* a, const double* alpha, const double* alpha0,
                     const double* beta0, const double* X, int P, const double* Z, int ldz, long long N, int M, int rows,
                     bool want_z, double* partials, hipStream_t s, const int* colwin, const ColBatch* batch, int max_blocks,
                     const double* Ar, const double* ell) {
  if (N <= 0) return;
  ColBatch bt = batch ? *batch : ColBatch{};
  dim3 grid((M + 511) / 512, (unsigned)((N + rows - 1) / rows), batch ? batch->nq : 1);
  if (max_blocks > 0) {   // cap the blocks in flight: each takes several row splits in turn
    const long long per_y = (long long)grid.x * grid.z;
    grid.y = (unsigned)std::max<long long>(1, std::min<long long>(grid.y, max_blocks / per_y));
  }
#define HM_COLSTATS(ST, SLV)                                                                                                        \
  do {                                                                                                                            \
    if (colwin || P == 1) {                  /* (P = 1 never spilled, and its vector loads are faster: C2's column statistics 10.8 vs 11.9 ms) */ \
      DISPATCH_P(P, hipLaunchKernelGGL((colstats_kernel<PP, ST, SLV, true>), grid, dim3(256), 0, s, Kh, Pt, a, alpha, alpha0, beta0, X, \
                                       Z, ldz, N, M, rows, want_z ? 1 : 0, partials, colwin, bt, Ar, ell));                     \
    } else {                                                                                                                      \
      DISPATCH_P(P, hipLaunchKernelGGL((colstats_kernel<PP, ST, SLV, false>), grid, dim3(256), 0, s, Kh, Pt, a, alpha, alpha0, beta0, X, \
                                       Z, ldz, N, M, rows, want_z ? 1 : 0, partials, colwin, bt, Ar, ell));                     \
    }                                                                                                                             \
  } while (0)
  if (Ar && ell) { HM_COLSTATS(true, true); }
  else if (Ar) { HM_COLSTATS(true, false); }
  else if (ell) { HM_COLSTATS(false, true); }
  else { HM_COLSTATS(false, false); }
#undef HM_COLSTATS
}

// dst[q * sDst] += sum_m v[q][m]   (the per-column s2 of the column statistics -> the bundle's sl_q; fixed order)
__global__ __launch_bounds__(256) void sum_cols_kernel(const double* __restrict__ v, int M, double* __restrict__ dst, long long sDst) {
  __shared__ double scratch[16];
  const double* x = v + (long long)blockIdx.x * M;
  double s = 0.0;
  for (int m = threadIdx.x; m < M; m += 256) s += x[m];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) dst[(long long)blockIdx.x * sDst] += s;
}
void launch_sum_cols(const double* v, int Q, int M, double* dst, long long sDst, hipStream_t s) {
  hipLaunchKernelGGL(sum_cols_kernel, dim3(Q), dim3(256), 0, s, v, M, dst, sDst);
}

void launch_reduce_rows(const double* partials, long long nrows, int len, const long long* off, double* dst, bool accumulate,
                        hipStream_t s) {
  if (len <= 0) return;
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(len), dim3(256), 0, s, partials, nrows, len, off, dst, accumulate ? 1 : 0);
}

void launch_reduce_slabs(const double* slabs, int nslabs, long long stride, long long len, double* dst, bool accumulate,
                         hipStream_t s, int nb, long long sSlabs, long long sDst) {
  if (len <= 0) return;
  hipLaunchKernelGGL(reduce_slabs_kernel, dim3((unsigned)((len + 15) / 16), nb), dim3(256), 0, s, slabs, nslabs, stride, len,
                     dst, accumulate ? 1 : 0, sSlabs, sDst);
}

void launch_reduce_slabs_lower(const double* slabs, int nslabs, int M, double* dst, bool accumulate, hipStream_t s, int nb,
                               long long sSlabs, long long sDst) {
  const int tiles = (M + 127) / 128;
  hipLaunchKernelGGL(reduce_slabs_lower_kernel, dim3(tiles * (tiles + 1) / 2, 32, nb), dim3(256), 0, s, slabs, nslabs, M, dst,
                     accumulate ? 1 : 0, sSlabs, sDst);
}

void launch_mirror_lower(double* A, int Q, int M, long long stride, hipStream_t s) {
  hipLaunchKernelGGL(mirror_lower_kernel, dim3((M + 255) / 256, M, Q), dim3(256), 0, s, A, M, stride);
}

void launch_wire_copy(double* bundle, double* wire, long long NG, int Q, int M, long long per_q, int dir, hipStream_t s) {
  const long long MM = (long long)M * M, Mtri = (long long)M * (M + 1) / 2, wire_per_q = Mtri + (per_q - MM);
  hipLaunchKernelGGL(wire_tri_kernel, dim3((M + 255) / 256, M, Q), dim3(256), 0, s, bundle + NG, wire + NG, M, per_q, wire_per_q,
                     dir);
  const long long rest = NG + (per_q - MM) * Q;
  hipLaunchKernelGGL(wire_rest_kernel, dim3((unsigned)((rest + 255) / 256)), dim3(256), 0, s, bundle, wire, NG, MM, Mtri, per_q,
                     wire_per_q, Q, dir);
}

void launch_raw_kmn(const double* a, const double* gm, const double* gv, int J, int j, double w, const double* Pt, int M,
                    long long N, double* out, hipStream_t s) {
  if (N <= 0) return;
  hipLaunchKernelGGL(raw_kmn_kernel, dim3((unsigned)((N + 255) / 256), M), dim3(256), 0, s, a, gm, gv, J, j, w, Pt, M, N, out);
}
