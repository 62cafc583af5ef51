// strict_rows.hip -- the strict q(f) mode's (HMOGP_CFG_STRICT_QF) own row kernels beside trsm_panel.hip: the row statistics of the
// solve-based forms and the diagonal-block step of the blocked triangular solves.  Declarations: rowpass.h.
#include "rowpass.h"
#include "rbf_device.h"

// ---- strict q(f) (HMOGP_CFG_STRICT_QF): row statistics of the solve-based forms of svmogp_inf.py:212-218 ------------------------
// One wave per row.  phase 0:  p = A m_q,  c = rowsum(T .* T) - rowsum(A .* K^)    with A = K^ Kuu^-1, T = A L_q  ==  the reference's
// sum(square(dtrmm(L_q^T, R)), 0) - sum(R * Kfu^T, 0)  with R = dpotrs(Luu, Kfu^T) -- [r6] through X = K^ Luu^-T alone:
// p = X (Luu^-1 m), rowsum(A .* K^) = rowsum(X .* X), T = X (Luu^-1 L_q)  (the fallback of trsm_panel.hip's fused statistics).
// phase 1:  pg = K^ a,  cg = rowsum(P~ .* K^)  and their r2-weighted twins pt, ct, with P~ = A (S Kuu^-1 - I): what the reference's
// dL_dKmn (svmogp_inf.py:157-161) reduces to against K^ in svmogp.py:116-156.
template <int P>
__global__ __launch_bounds__(256) void strict_rowstats_kernel(StrictRows a) {
  const int q = blockIdx.y, lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= a.n) return;
  const int M = a.M;
  const double* kh = a.Kh + q * a.sK + n * M;
  if (a.phase == 0) {
    const double* ah = a.Ah + q * a.sK + n * M;
    double sp = 0.0, st = 0.0, sk = 0.0;
    // [r6] one-solve form: `Ah` holds X = K^ Luu^-T;  A m = X (Luu^-1 m) = X w3,  rowsum(A .* K^) = rowsum(X .* X)
    // (two-solve form, a.w3 == nullptr: `Ah` holds A itself -- p = A m, rowsum(A .* K^))
    const double* w3 = a.w3 ? a.w3 + (long long)q * M : nullptr;
    if (a.t2) {        // rowsum(T .* T) came out of the product's epilogue (gemm_rowpass.hip, fs_sq): T was never stored
      for (int m = lane; m < M; m += 64) {
        const double av = ah[m];
        sp += av * (w3 ? w3[m] : a.mu[(long long)m * a.Q + q]);
        sk += av * (w3 ? av : kh[m]);
      }
      sp = wave_sum(sp), sk = wave_sum(sk);
      if (lane == 0) a.p[q * a.ldn + n] = sp, a.c[q * a.ldn + n] = a.t2[q * a.ldn + n] - sk;
      return;
    }
    const double* tt = a.Tt + q * a.sK + n * M;
    for (int m = lane; m < M; m += 64) {
      const double av = ah[m], tv = tt[m];
      sp += av * (w3 ? w3[m] : a.mu[(long long)m * a.Q + q]);
      st += tv * tv;
      sk += av * (w3 ? av : kh[m]);
    }
    sp = wave_sum(sp), st = wave_sum(st), sk = wave_sum(sk);
    if (lane == 0) a.p[q * a.ldn + n] = sp, a.c[q * a.ldn + n] = st - sk;
    return;
  }
  const double* pt = a.Pt + q * a.sK + n * M;
  const double* av = a.a + (long long)q * M;
  const double* Z = a.Z + (long long)q * a.sZ;
  const double ell = a.ell[q];
  double xv[P];
#pragma unroll
  for (int p = 0; p < P; ++p) xv[p] = a.X[n * P + p];
  const double xsq = sumsq<P>(xv);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  for (int m = lane; m < M; m += 64) {
    double zv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) zv[p] = Z[(long long)m * a.ldz + p];
    const double r2 = rbf_r2<P>(xv, xsq, zv, sumsq<P>(zv), ell);
    const double k = kh[m], ka = k * av[m], pk = pt[m] * k;
    s0 += ka, s1 += pk, s2 += ka * r2, s3 += pk * r2;
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2), s3 = wave_sum(s3);
  if (lane == 0) {
    a.pg[q * a.ldn + n] = s0, a.cg[q * a.ldn + n] = s1;
    if (a.pt) a.pt[q * a.ldn + n] = s2, a.ct[q * a.ldn + n] = s3;
  }
}
// strict q(f): the diagonal-block step of the blocked triangular solves  V Luu^T = K^  (DIR 0, forward over the block's columns)
// and  A Luu = V  (DIR 1, backward) that make up the reference's dpotrs (svmogp_inf.py:214).  One thread = one row of the n x M
// right-hand side with its <= 32 unknowns in registers, the 32 x 32 diagonal block of Luu in LDS (broadcast reads); TRUE
// substitution, every unknown divided by its pivot as in LAPACK's dtrsm.  (A product with an explicit inverse of the block -- of
// any width down to 8 -- loses cond(block) more digits: 5e-8 instead of 3e-10 in m_fd at cond(K_uu) = 1e7, measured.)  The
// off-diagonal updates between two such steps are plain GEMMs (launch_gemm_f64, alpha = -1, beta = 1).
template <int DIR>
__global__ __launch_bounds__(256) void trsm_diag_kernel(double* __restrict__ V, long long sV, const double* __restrict__ L,
                                                        long long sL, int M, int j0, int nb, long long n, int wide, int u0, int u1,
                                                        const double* __restrict__ Vsrc) {
  // (the unknowns live in LDS, one column of 256 lanes per unknown -- conflict-free -- and the loops run at run time: with
  //  x[32] in registers and both loops unrolled the compiler hoists all 528 broadcast reads and spills ~1 KB per lane)
  __shared__ double Ls[32][33];
  __shared__ double xs[32][258];
  V += (long long)blockIdx.y * sV, L += (long long)blockIdx.y * sL;
  // Vsrc (wide launches only): this launch is the FIRST touch of its columns -- x and the updated columns are read from the matrix
  // the solve started from (same layout as V) and written to V: no copy of that matrix beforehand
  const double* Vin = Vsrc ? Vsrc + (long long)blockIdx.y * sV : V;
  const int t = threadIdx.x;
  for (int e = t; e < 32 * 32; e += 256) {
    const int r = e >> 5, c = e & 31;
    Ls[r][c] = (r < nb && c < nb) ? L[(long long)(j0 + r) * M + j0 + c] : (r == c ? 1.0 : 0.0);
  }
  const long long row0 = (long long)blockIdx.x * 256, row = row0 + t;
  const bool valid = row < n;
  double* v = V + (valid ? row : 0) * M + j0;
  // [r5] the block's 256 x 32 right-hand sides enter (and leave) through 16-byte accesses in which 16 consecutive lanes cover one
  // row's 256 bytes: one row per lane (32 loads of 8 bytes, lanes 8 KB apart) touched 64 cache lines per instruction
  // (substitution launches 47 -> 30 ms per strict step at the headline size: DESIGN 12g)
  // (`wide` is decided by the launcher: nb == 32, even M / j0 / batch stride, 16-byte aligned V)
  if (wide) {
#pragma unroll 4
    for (int e = t; e < 256 * 16; e += 256) {
      const int r = e >> 4, ch = e & 15;
      f64x2 v2 = f64x2{0.0, 0.0};
      if (row0 + r < n) v2 = *reinterpret_cast<const f64x2*>(Vin + (row0 + r) * M + j0 + 2 * ch);
      xs[2 * ch][r] = v2.x, xs[2 * ch + 1][r] = v2.y;
    }
  } else {
    for (int c = 0; c < 32; ++c) xs[c][t] = (valid && c < nb) ? v[c] : 0.0;
  }
  __syncthreads();
  // Chunks of 8 unknowns: their right-hand sides sit in 8 registers while the contributions of the unknowns solved before are
  // subtracted (one LDS read of the unknown + 8 broadcast reads of L feed 8 INDEPENDENT fused multiply-adds: the first version
  // ran one dependent chain per unknown, 25 ms per step at 200 000 rows), then the 8 x 8 triangle is solved in registers.
  // Padded rows / columns of the last block are identity: harmless.
  if (DIR == 0) {
    for (int c0 = 0; c0 < 32; c0 += 8) {
      if (c0 >= nb) break;
      double acc[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = xs[c0 + r][t];
      for (int i = 0; i < c0; ++i) {
        const double xi = xs[i][t];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] -= xi * Ls[c0 + r][i];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int q = 0; q < r; ++q) acc[r] -= acc[q] * Ls[c0 + r][c0 + q];
        acc[r] = acc[r] / Ls[c0 + r][c0 + r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) xs[c0 + r][t] = acc[r];
    }
  } else {
    for (int c0 = 24; c0 >= 0; c0 -= 8) {
      if (c0 >= nb) continue;
      double acc[8];
#pragma unroll
      for (int r = 0; r < 8; ++r) acc[r] = xs[c0 + r][t];
      for (int i = 31; i >= c0 + 8; --i) {
        const double xi = xs[i][t];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] -= xi * Ls[i][c0 + r];
      }
#pragma unroll
      for (int r = 7; r >= 0; --r) {
#pragma unroll
        for (int q = 7; q > r; --q) acc[r] -= acc[q] * Ls[c0 + q][c0 + r];
        acc[r] = acc[r] / Ls[c0 + r][c0 + r];
      }
#pragma unroll
      for (int r = 0; r < 8; ++r) xs[c0 + r][t] = acc[r];
    }
  }
  if (wide) {
    __syncthreads();
#pragma unroll 4
    for (int e = t; e < 256 * 16; e += 256) {
      const int r = e >> 4, ch = e & 15;
      if (row0 + r < n) *reinterpret_cast<f64x2*>(V + (row0 + r) * M + j0 + 2 * ch) = f64x2{xs[2 * ch][r], xs[2 * ch + 1][r]};
    }
    // [r5] The RIGHT-LOOKING update of the columns [u0, u1) that this block's unknowns still feed inside the current 128-column
    // block of the two-level scheme -- V[:, c] -= sum_k x[:, j0 + k] L[c][j0 + k] (DIR 0) / L[j0 + k][c] (DIR 1) -- on the
    // matrix cores, 32 columns at a time, with the freshly solved x read from LDS where it already sits: the separate
    // 32-column GEMM updates (one quarter of a 128-wide tile used, A and C streamed from HBM again) cost as much as the
    // 128-column updates that carry 12 x their flops.  A wave owns 64 rows; D fragment: col = lane & 15, row = (lane >> 4) + 4 reg.
    const int lane = t & 63, w = t >> 6, lr = lane & 15, lk = lane >> 4;
    for (int g0 = u0; g0 < u1; g0 += 32) {
      __syncthreads();                      // Ls: the substitution / the previous group's products are done with it
      for (int e = t; e < 32 * 32; e += 256) {
        if (DIR == 0) {
          const int c = e >> 5, k = e & 31;
          Ls[k][c] = L[(long long)(g0 + c) * M + j0 + k];
        } else {
          const int k = e >> 5, c = e & 31;
          Ls[k][c] = L[(long long)(j0 + k) * M + g0 + c];
        }
      }
      f64x4 acc[4][2];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long rr = row0 + w * 64 + a * 16 + 4 * r + lk;
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b][r] = rr < n ? Vin[rr * M + g0 + b * 16 + lr] : 0.0;
        }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        double fa[4], fb[2];
#pragma unroll
        for (int a = 0; a < 4; ++a) fa[a] = -xs[kk * 4 + lk][w * 64 + a * 16 + lr];
#pragma unroll
        for (int b = 0; b < 2; ++b) fb[b] = Ls[kk * 4 + lk][b * 16 + lr];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
      }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long long rr = row0 + w * 64 + a * 16 + 4 * r + lk;
          if (rr >= n) continue;
#pragma unroll
          for (int b = 0; b < 2; ++b) V[rr * M + g0 + b * 16 + lr] = acc[a][b][r];
        }
    }
    return;
  }
  if (valid)
    for (int c = 0; c < nb; ++c) v[c] = xs[c][t];
}
bool trsm_diag_can_fuse(const double* V, long long sV, int M) {
  return (M % 32) == 0 && (sV & 1) == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0;
}
void launch_trsm_diag(int dir, double* V, long long sV, const double* L, long long sL, int M, int j0, int nb, long long n, int Q,
                      hipStream_t s, int u0, int u1, const double* Vsrc) {
  if (n <= 0 || nb <= 0) return;
  dim3 grid((unsigned)((n + 255) / 256), Q);
  const int wide = (nb == 32 && (M & 1) == 0 && (j0 & 1) == 0 && (sV & 1) == 0 && (reinterpret_cast<uintptr_t>(V) & 15) == 0) ? 1 : 0;
  if (u1 > u0 && (!wide || ((u1 - u0) & 31) || (u0 & 31)))
    throw HipError{hipErrorInvalidValue, "trsm_diag: fused update needs full 32-column blocks and aligned rows", __FILE__, __LINE__};
  if (Vsrc && (!wide || (reinterpret_cast<uintptr_t>(Vsrc) & 15)))
    throw HipError{hipErrorInvalidValue, "trsm_diag: a first-touch source needs the row-coalesced path", __FILE__, __LINE__};
  if (dir == 0) hipLaunchKernelGGL((trsm_diag_kernel<0>), grid, dim3(256), 0, s, V, sV, L, sL, M, j0, nb, n, wide, u0, u1, Vsrc);
  else hipLaunchKernelGGL((trsm_diag_kernel<1>), grid, dim3(256), 0, s, V, sV, L, sL, M, j0, nb, n, wide, u0, u1, Vsrc);
}
void launch_strict_rowstats(const StrictRows& a, hipStream_t s) {
  if (a.n <= 0) return;
  dim3 grid((unsigned)((a.n + 3) / 4), a.Q);
  DISPATCH_P(a.P, hipLaunchKernelGGL((strict_rowstats_kernel<PP>), grid, dim3(256), 0, s, a));
}
