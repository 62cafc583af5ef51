// probe_gram_direct.hip -- the weighted Gram's main loop (gemm_rowpass.hip, ROLE 2, full-tile form) with ONE operand's MFMA
// fragments loaded STRAIGHT FROM GLOBAL MEMORY into registers and the LDS that frees spent on a k-major image of the other operand
// at BK = 32 (2 x 32 x 144 doubles: today's footprint): one block barrier per 64 MFMAs per wave instead of one per 32.
// Diagnostic only (not part of the .so).  H_split = K^T diag(beta) K^ over row ranges of 8192 rows, M = 1024, n = 2 097 152 rows:
// the operand is 16 GiB, far beyond the 256 MiB Infinity Cache, so the first tile of a range to touch a panel pulls it from HBM and
// the other tiles of the range (same XCD) find it in L2 -- as in the step.  Every variant is timed in every pass and pass 0 (clock
// ramp) is not printed; passes 1 and 2 are, so that the spread between repeated passes of one variant can be read off the output.
//   variant 0   today's round-3 loop: both operands staged at BK = 16, fragments read inside the step
//   variant 1   i-side direct (unscaled, 4 loads per k4-step), wave tile 64 x 32, scaled j-side image at BK = 32, ring D = 2
//   variant 2   i-side direct (2 loads per k4-step), wave tile 32 x 64 (4 ds_read per k4-step), ring D = 2
//   variant 3   the same, D = 4
//   variant 4   j-side direct (2 loads per k4-step, beta of the lane's own k applied in registers: 2 v_mul_f64 per 8 MFMAs),
//               wave tile 64 x 32, unscaled i-side image at BK = 32, ring D = 2
//   variants 5, 6   i-side direct, wave tile 16 x 128: the eight waves load disjoint 16-column bands (ONE load per k4-step, no panel
//               byte fetched twice by a block), 8 ds_read per k4-step in two groups of 4 in front of their 4 MFMAs; D = 2 and 4
// All direct loads are buffer_load_dwordx2: the lane part of the address in a VGPR, the k part in an SGPR; the resource is based at
// the block's first row of its range and its column panel (a range of 8192 rows x 8 KB = 64 MiB of 32-bit byte offsets).
// The image is staged in two halves of 16 rows, each loaded four k4-steps ahead of its ds_write into ONE set of staging registers
// (4 doubles + the k-scale): the lead of today's loop at about half its staging registers.
// Every accumulator sees the same products a_ki (beta_k a_kj) in the same order: all slabs of variants 1..6 are compared bit by
// bit with those of variant 0 ("differing" must print 0).
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int BM = 128, BN = 128, NT = 512, KM_LD = 144;
#define SB __builtin_amdgcn_sched_barrier(0)

struct Where {
  int ti, tj, split, kbeg, kend;
};
// block -> (tile, range): all tiles of one range on ONE XCD (block b runs on XCD b % 8), as launch_gemm_rowpass orders role 6
__device__ __forceinline__ bool where(int M, int K, int ksplit, Where& q) {
  const int T = M / BM, ntiles = T * T, v = blockIdx.x, xcd = v & 7, idx = v >> 3;
  q.split = (idx / ntiles) * 8 + xcd;
  if (q.split >= ksplit) return false;
  const int u = idx % ntiles;
  q.ti = u / T, q.tj = u - q.ti * T;
  const int ksteps = (K + 15) / 16, per = (ksteps + ksplit - 1) / ksplit;
  q.kbeg = q.split * per * 16;
  q.kend = min(K, q.kbeg + per * 16);
  return true;
}

// ---- variant 0: the product loop as it is ---------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 4) void gram_lds(const double* __restrict__ A, const double* __restrict__ S, double* __restrict__ C,
                                                  int M, int K, int ksplit) {
  constexpr int BK = 16, TILE = BK * KM_LD;
  __shared__ __attribute__((aligned(16))) double la[2][TILE];
  __shared__ __attribute__((aligned(16))) double lb[2][TILE];
  Where q;
  if (!where(M, K, ksplit, q)) return;
  const int i0 = q.ti * BM, j0 = q.tj * BN, kbeg = q.kbeg, kend = q.kend, lda = M;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  const int wm = w >> 2, wn = w & 3;
  f64x4 acc[4][2];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0, 0, 0, 0};
  const int bk = t >> 5, bc = (t & 31) * 2;
  const double* pa = A + i0 + bc;
  const double* pb = A + j0 + bc;
  double ra[4], rb[4], ks = 1.0;
  auto load = [&](int k0) {
    const int row = k0 + bk;
    const long long off = (long long)min(row, K - 1) * lda;
    const f64x2 x0 = *reinterpret_cast<const f64x2*>(pa + off), x1 = *reinterpret_cast<const f64x2*>(pa + off + 64);
    ra[0] = x0.x, ra[1] = x0.y, ra[2] = x1.x, ra[3] = x1.y;
    const f64x2 y0 = *reinterpret_cast<const f64x2*>(pb + off), y1 = *reinterpret_cast<const f64x2*>(pb + off + 64);
    rb[0] = y0.x, rb[1] = y0.y, rb[2] = y1.x, rb[3] = y1.y;
    ks = (row < kend) ? S[row] : 0.0;
  };
  auto stage = [&](int buf) {
    double* sa = &la[buf][bk * KM_LD + bc];
    *reinterpret_cast<f64x2*>(sa) = f64x2{ra[0], ra[1]};
    *reinterpret_cast<f64x2*>(sa + 64) = f64x2{ra[2], ra[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) rb[i] *= ks;
    double* sb = &lb[buf][bk * KM_LD + bc];
    *reinterpret_cast<f64x2*>(sb) = f64x2{rb[0], rb[1]};
    *reinterpret_cast<f64x2*>(sb + 64) = f64x2{rb[2], rb[3]};
  };
  int cur = 0;
  if (kbeg < kend) {
    load(kbeg);
    stage(0);
    if (kbeg + BK < kend) load(kbeg + BK);
  }
  __syncthreads();
  for (int k0 = kbeg; k0 < kend; k0 += BK) {
    if (k0 + BK < kend) stage(cur ^ 1);
    if (k0 + 2 * BK < kend) load(k0 + 2 * BK);
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      double fa[4], fb[2];
      const double* fpa = &la[cur][(kk * 4 + lk) * KM_LD + wm * 64 + lr];
      const double* fpb = &lb[cur][(kk * 4 + lk) * KM_LD + wn * 32 + lr];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = fpa[i * 16];
#pragma unroll
      for (int i = 0; i < 2; ++i) fb[i] = fpb[i * 16];
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][b], 0, 0, 0);
    }
    __syncthreads();
    cur ^= 1;
  }
  double* Cs = C + (size_t)q.split * M * M;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double* crow = Cs + (size_t)(i0 + wm * 64 + a * 16 + 4 * r + lk) * M + j0 + wn * 32 + lr;
#pragma unroll
      for (int b = 0; b < 2; ++b) crow[b * 16] = acc[a][b][r];
    }
}

// ---- variants 1..6: one operand's fragments global -> registers, the other as a k-major image at BK = 32 --------------------
// JD = false: the i-side (MFMA operand A, NA sub-tiles of 16 columns per wave) is direct, the image holds beta_k a_kj;
// JD = true:  the j-side (NB sub-tiles) is direct and multiplied by beta_k in registers, the image holds a_ki unscaled and the
//             32 k-scales of the step sit beside it.
// Ring: D slots of the direct operand's fragment; the loads of k4-step s + D are issued right BEHIND the 8 MFMAs of step s, into the
// slot those have read.  Loads beyond the range's last k4-step re-read it (clamped; consumed against a zero scale or not at all), and
// the image loads beyond the range read row min(row, K - 1) with scale 0: no conditional load in the loop.  A range that ends in
// the matrix's last, ragged k4-step (K % 4 != 0) takes the lane offset with the rows clamped to K - 1 for that step: one
// v_cndmask per k4-step on a scalar condition.
template <bool JD, int NA, int NB, int D>
__global__ __launch_bounds__(NT, 4) void gram_direct(const double* __restrict__ A, const double* __restrict__ S, double* __restrict__ C,
                                                     int M, int K, int ksplit) {
  constexpr int BK = 32, KS = BK / 4, IMG = BK * KM_LD, ND = JD ? NB : NA, NWJ = BN / (16 * NB);
  static_assert(NA * NB == 8 && KS % D == 0, "8 accumulators per wave; static ring slots");
  __shared__ __attribute__((aligned(16))) double img[2][IMG];
  __shared__ double kscl[JD ? 2 * BK + 2 * BK + 64 : 1];   // [2][BK] k-scales + a sink for the lanes that have none to write
  Where q;
  if (!where(M, K, ksplit, q)) return;
  const int i0 = q.ti * BM, j0 = q.tj * BN, kbeg = q.kbeg, kend = q.kend, lda = M;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  const int wm = w / NWJ, wn = w % NWJ;
  f64x4 acc[NA][NB];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = f64x4{0, 0, 0, 0};
  double* Cs = C + (size_t)q.split * M * M;
  if (kbeg < kend) {
    // image operand: thread = k row t/32 (+ 16 for the second half), column pairs (t%32)*2 and + 64
    const int bk = t >> 5, bc = (t & 31) * 2;
    const double* pst = A + (JD ? i0 : j0) + bc;
    double rs[4], ks;
    double* const ksdst = !JD ? kscl : (t & 31) == 0 ? &kscl[bk] : &kscl[2 * BK + lane];
    auto loadh = [&](int k0, int h) {
      const int row = min(k0 + 16 * h + bk, K - 1);
      const long long off = (long long)row * lda;
      const f64x2 x0 = *reinterpret_cast<const f64x2*>(pst + off), x1 = *reinterpret_cast<const f64x2*>(pst + off + 64);
      rs[0] = x0.x, rs[1] = x0.y, rs[2] = x1.x, rs[3] = x1.y;
      ks = S[row];
    };
    auto stageh = [&](int buf, int k0, int h) {
      const double sc = (k0 + 16 * h + bk < kend) ? ks : 0.0;
      if (JD) {
        ksdst[buf * BK + 16 * h] = sc;               // (every lane writes: a branch here costs a vmcnt(0) in the loop)
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) rs[i] *= sc;
      }
      double* s = &img[buf][(16 * h + bk) * KM_LD + bc];
      *reinterpret_cast<f64x2*>(s) = f64x2{rs[0], rs[1]};
      *reinterpret_cast<f64x2*>(s + 64) = f64x2{rs[2], rs[3]};
    };
    // direct operand
    const int dcol = JD ? j0 : i0;
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(A + (size_t)kbeg * lda + dcol), 0, (int)(sizeof(double) * ((size_t)(kend - 1 - kbeg) * lda + 128)), 0x00020000);
    const int klim = kbeg + 4 * ((kend - kbeg - 1) / 4);        // the range's last k4-step
    const int wcol = (JD ? wn * 16 * NB : wm * 16 * NA) + lr;
    const int voff = (int)sizeof(double) * (lk * lda + wcol);
    const int voff_last = (int)sizeof(double) * (min(lk, K - 1 - klim) * lda + wcol);
    double dr[D][ND];
    auto dload = [&](int k, int slot) {
      const int so = __builtin_amdgcn_readfirstlane((min(k, klim) - kbeg) * lda * (int)sizeof(double));
      const int vo = (k >= klim) ? voff_last : voff;
#pragma unroll
      for (int i = 0; i < ND; ++i)
        dr[slot][i] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(brs, vo + i * 16 * (int)sizeof(double), so, 0));
    };
    int cur = 0;
    loadh(kbeg, 0);
    stageh(0, kbeg, 0);
    loadh(kbeg, 1);
    stageh(0, kbeg, 1);
    loadh(kbeg + BK, 0);
#pragma unroll
    for (int d = 0; d < D; ++d) dload(kbeg + 4 * d, d);
    __syncthreads();
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        constexpr int NS = JD ? NA : NB, NG = (!JD && NB > 4) ? 2 : 1, NBG = NB / NG;   // (16 x 128: the image fragments in two groups of 4)
#pragma unroll
        for (int gq = 0; gq < NG; ++gq) {
          double fs[NS / NG], fa[NA], fb[NBG];
          const double* fp = &img[cur][(kk * 4 + lk) * KM_LD + (JD ? wm * 16 * NA : wn * 16 * NB + gq * 16 * NBG) + lr];
#pragma unroll
          for (int i = 0; i < NS / NG; ++i) fs[i] = fp[i * 16];
          if (JD) {
            const double bs = kscl[cur * BK + kk * 4 + lk];
#pragma unroll
            for (int i = 0; i < NA; ++i) fa[i] = fs[i];
#pragma unroll
            for (int i = 0; i < NB; ++i) fb[i] = dr[kk % D][i] * bs;
          } else {
#pragma unroll
            for (int i = 0; i < NA; ++i) fa[i] = dr[kk % D][i];
#pragma unroll
            for (int i = 0; i < NBG; ++i) fb[i] = fs[i];
          }
          SB;
#pragma unroll
          for (int a = 0; a < NA; ++a)
#pragma unroll
            for (int b = 0; b < NBG; ++b)
              acc[a][gq * NBG + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a], fb[b], acc[a][gq * NBG + b], 0, 0, 0);
          SB;
        }
        dload(k0 + 4 * (kk + D), kk % D);
        if (kk == 0) {
          stageh(cur ^ 1, k0 + BK, 0);
          loadh(k0 + BK, 1);
        }
        if (kk == KS / 2) {
          stageh(cur ^ 1, k0 + BK, 1);
          loadh(k0 + 2 * BK, 0);
        }
        SB;
      }
      __syncthreads();
      cur ^= 1;
    }
  }
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double* crow = Cs + (size_t)(i0 + wm * 16 * NA + a * 16 + 4 * r + lk) * M + j0 + wn * 16 * NB + lr;
#pragma unroll
      for (int b = 0; b < NB; ++b) crow[b * 16] = acc[a][b][r];
    }
}

__global__ void fill(double* __restrict__ x, size_t n, unsigned long long seed, double lo, double hi) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long z = (i + seed) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL, z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL, z ^= z >> 31;
    x[i] = lo + (hi - lo) * ((double)(z >> 11) / 9007199254740992.0);
  }
}
__global__ void count_diff(const unsigned long long* __restrict__ x, const unsigned long long* __restrict__ y, size_t n,
                           unsigned long long* __restrict__ out) {
  unsigned long long c = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) c += x[i] != y[i];
  if (c) atomicAdd(out, c);
}

#define CK(x)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (x);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      printf("%s: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);                   \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

int main(int argc, char** argv) {
  const int M = 1024, per_rows = 8192;
  const int n = argc > 1 ? atoi(argv[1]) : 2097152;          // rows (argument: a smaller run, e.g. a ragged one for the compare)
  const int ksteps = (n + 15) / 16, ksplit = (n + per_rows - 1) / per_rows, per = (ksteps + ksplit - 1) / ksplit;
  const size_t slab = (size_t)ksplit * M * M;
  double *A, *S, *C, *C0;
  unsigned long long* nd;
  CK(hipMalloc(&A, sizeof(double) * (size_t)n * M));
  CK(hipMalloc(&S, sizeof(double) * (size_t)n));
  CK(hipMalloc(&C, sizeof(double) * slab));
  CK(hipMalloc(&C0, sizeof(double) * slab));
  CK(hipMalloc(&nd, sizeof(*nd)));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, A, (size_t)n * M, 1ULL, -1.0, 1.0);
  hipLaunchKernelGGL(fill, dim3(1024), dim3(256), 0, 0, S, (size_t)n, 77ULL, 0.0625, 1.0);
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const int T = M / BM, blocks = T * T * ((ksplit + 7) / 8) * 8;
  const char* names[] = {"today's loop (both images, BK = 16)", "i direct, 64 x 32, D = 2, j image BK = 32", "i direct, 32 x 64, D = 2, j image BK = 32",
                         "i direct, 32 x 64, D = 4, j image BK = 32", "j direct, 64 x 32, D = 2, i image BK = 32",
                         "i direct, 16 x 128, D = 2, j image BK = 32", "i direct, 16 x 128, D = 4, j image BK = 32"};
  printf("n = %d rows, M = %d, %d ranges of %d k-steps of 16, %d blocks, operand %.1f GiB\n", n, M, ksplit, per, blocks,
         (double)n * M * 8 / (1 << 30));
  const int reps = 3;
  for (int pass = 0; pass < 3; ++pass)     // pass 0 warms the device up (clocks): only passes 1 and 2 are printed
    for (int variant = 0; variant < 7; ++variant) {
      auto run = [&] {
        switch (variant) {
          case 0: hipLaunchKernelGGL(gram_lds, dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 1: hipLaunchKernelGGL((gram_direct<false, 4, 2, 2>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 2: hipLaunchKernelGGL((gram_direct<false, 2, 4, 2>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 3: hipLaunchKernelGGL((gram_direct<false, 2, 4, 4>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 4: hipLaunchKernelGGL((gram_direct<true, 4, 2, 2>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 5: hipLaunchKernelGGL((gram_direct<false, 1, 8, 2>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
          case 6: hipLaunchKernelGGL((gram_direct<false, 1, 8, 4>), dim3(blocks), dim3(NT), 0, 0, A, S, C, M, n, ksplit); break;
        }
      };
      CK(hipMemset(C, 0xFF, sizeof(double) * slab));
      run();
      CK(hipDeviceSynchronize());
      CK(hipEventRecord(e0));
      for (int i = 0; i < reps; ++i) run();
      CK(hipEventRecord(e1));
      CK(hipEventSynchronize(e1));
      CK(hipGetLastError());
      float ms;
      CK(hipEventElapsedTime(&ms, e0, e1));
      ms /= reps;
      unsigned long long diff = 0;
      if (variant == 0) {
        CK(hipMemcpy(C0, C, sizeof(double) * slab, hipMemcpyDeviceToDevice));
      } else {
        CK(hipMemset(nd, 0, sizeof(*nd)));
        hipLaunchKernelGGL(count_diff, dim3(4096), dim3(256), 0, 0, (const unsigned long long*)C, (const unsigned long long*)C0, slab, nd);
        CK(hipMemcpy(&diff, nd, sizeof(diff), hipMemcpyDeviceToHost));
      }
      double c0;
      CK(hipMemcpy(&c0, C + (size_t)(ksplit - 1) * M * M + 777 * (size_t)M + 100, sizeof(double), hipMemcpyDeviceToHost));
      if (pass) printf("pass %d  %-44s %8.3f ms  %6.2f TFLOP/s   H_last[777][100] = %.17g   differing from variant 0: %llu\n", pass,
                       names[variant], ms, 2.0 * n * M * (double)M / ms / 1e9, c0, diff);
      fflush(stdout);
    }
  return 0;
}
