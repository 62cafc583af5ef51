// probe_gemm_bdirect.hip -- the forward's main loop (gemm_rowpass.hip, ROLE 1) with the B operand's MFMA fragments loaded
// STRAIGHT FROM GLOBAL MEMORY (L2-resident C_q) into registers instead of through an LDS image, and the LDS that frees spent on
// an A image of BK = 32: one block barrier per 64 MFMAs per wave instead of one per 32.  Diagnostic only (not part of the .so).
// Same conventions as probe_gemm_abl.hip: n = 131072, M = 1024, every variant is timed in every pass and pass 0 (clock ramp)
// is not printed; passes 1 and 2 are, so that the spread between repeated passes of one variant can be read off the output.
//   variant 0        today's loop: A and B images at BK = 16, fragments one k4-step ahead and carried across the barrier
//   variant 1        B direct (D = 2), A image at BK = 16
//   variants 2..4    B direct, A image at BK = 32, B fragments D = 2, 3, 4 k4-steps ahead of the MFMAs that consume them
//   variant 5        variant 4 with global_load_dwordx2 (64-bit lane addresses) instead of buffer_load_dwordx2
//   variants 6, 7    ablations of variant 4 (timing only): every B load reads k rows 0..3 (L1-resident) / no B loads in the loop
// Template flags F of gemm_bd: 1 = no B loads in the loop, 2 = B rows 0..3 only, 4 = buffer loads (lane offset in a VGPR, the
// k part of the address in an SGPR).
// All variants accumulate the transposed sub-tiles (operands swapped, B columns permuted) like the product kernel, and every
// accumulator sees the same products in the same order: the check column must print the SAME value for variants 0..5.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
constexpr int BM = 128, BN = 128, W = 8, NT = 512;
#define SB __builtin_amdgcn_sched_barrier(0)

__device__ __forceinline__ void store_tile(double* __restrict__ C, int N, int i0, int j0, int wm, int wn, int lr, int lk,
                                           const f64x4 (&acc)[4][2]) {
#pragma unroll
  for (int a = 0; a < 4; ++a) {   // lane (lr, lk): row wm*64 + a*16 + lr, columns wn*32 + b*16 + 4*lk + (0..3)
    double* crow = C + (long long)(i0 + wm * 64 + a * 16 + lr) * N + j0 + wn * 32 + 4 * lk;
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      *reinterpret_cast<f64x2*>(crow + b * 16) = f64x2{acc[a][b][0], acc[a][b][1]};
      *reinterpret_cast<f64x2*>(crow + b * 16 + 2) = f64x2{acc[a][b][2], acc[a][b][3]};
    }
  }
}

// ---- variant 0: the product loop as it is ------------------------------------------------------------------------------
__global__ __launch_bounds__(NT, 4) void gemm_lds(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                  int n, int N, int K) {
  constexpr int BK = 16, KM_LD = 144, RM_LD = 18, TILE = BK * KM_LD;
  __shared__ __attribute__((aligned(16))) double la[2][TILE];
  __shared__ __attribute__((aligned(16))) double lb[2][TILE];
  const int tiles_n = N / BN;
  int v = blockIdx.x;
  const int ntiles = (n / BM) * tiles_n;
  if ((ntiles & 7) == 0) { const int cpx = ntiles >> 3; v = (v & 7) * cpx + (v >> 3); }
  const int ti = v / tiles_n, tj = v - ti * tiles_n, i0 = ti * BM, j0 = tj * BN;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  const int wm = w >> 2, wn = w & 3, blr = 4 * (lr & 3) + (lr >> 2);
  f64x4 acc[4][2];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0, 0, 0, 0};
  double ra[4], rb[4];
  const int ar = t >> 2, ak = (t & 3) * 4, bk = t >> 5, bc = (t & 31) * 2;
  const double* pa = A + (long long)(i0 + ar) * K + ak;
  const double* pb = B + (long long)bk * N + j0 + bc;
  auto load = [&](int k0) {
    const f64x2 x0 = *reinterpret_cast<const f64x2*>(pa + k0), x1 = *reinterpret_cast<const f64x2*>(pa + k0 + 2);
    ra[0] = x0.x, ra[1] = x0.y, ra[2] = x1.x, ra[3] = x1.y;
    const double* q = pb + (long long)k0 * N;
    const f64x2 y0 = *reinterpret_cast<const f64x2*>(q), y1 = *reinterpret_cast<const f64x2*>(q + 64);
    rb[0] = y0.x, rb[1] = y0.y, rb[2] = y1.x, rb[3] = y1.y;
  };
  auto stage = [&](int buf) {
    double* sa = &la[buf][ar * RM_LD + ak];
    *reinterpret_cast<f64x2*>(sa) = f64x2{ra[0], ra[1]};
    *reinterpret_cast<f64x2*>(sa + 2) = f64x2{ra[2], ra[3]};
    double* sb = &lb[buf][bk * KM_LD + bc];
    *reinterpret_cast<f64x2*>(sb) = f64x2{rb[0], rb[1]};
    *reinterpret_cast<f64x2*>(sb + 64) = f64x2{rb[2], rb[3]};
  };
  double ga[2][4], gb[2][2];
  auto frag = [&](int buf, int kk, int s) {
    const double* fpa = &la[buf][(wm * 64 + lr) * RM_LD + kk * 4 + lk];
    const double* fpb = &lb[buf][(kk * 4 + lk) * KM_LD + wn * 32 + blr];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[s][i] = fpa[i * 16 * RM_LD];
#pragma unroll
    for (int i = 0; i < 2; ++i) gb[s][i] = fpb[i * 16];
  };
  auto mm8 = [&](int s) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(gb[s][b], ga[s][a], acc[a][b], 0, 0, 0);
  };
  int cur = 0;
  load(0);
  stage(0);
  load(BK);
  __syncthreads();
  frag(0, 0, 0);
  for (int k0 = 0; k0 < K; k0 += BK) {
    const bool more = k0 + BK < K;
    frag(cur, 1, 1);
    SB;
    mm8(0);
    SB;
    if (more) stage(cur ^ 1);
    if (k0 + 2 * BK < K) load(k0 + 2 * BK);
    SB;
    frag(cur, 2, 0);
    SB;
    mm8(1);
    SB;
    frag(cur, 3, 1);
    SB;
    mm8(0);
    SB;
    __syncthreads();
    if (more) frag(cur ^ 1, 0, 0);
    SB;
    mm8(1);
    SB;
    cur ^= 1;
  }
  store_tile(C, N, i0, j0, wm, wn, lr, lk, acc);
}

// ---- variants 1..4: B fragments global -> registers, A image of BKT columns ----------------------------------------------
// Row padding of the A image: LD = BKT + 2 doubles.  A fragment read is one ds_read_b64 per lane at dword address
// 2 LD lr + 2 lk (+ const); LD / 2 odd (9, 17) makes 2 LD lr mod 64 run through the 16 multiples of 4, so the 32 lanes of
// a half wave (lk in {0, 1} or {2, 3}) hit 64 distinct banks.  The stage writes are ds_write_b128 (groups of 8 lanes, banks
// mod 32): a thread writes the k's (t%4)*4..+3 and, at BKT = 32, 16 + the same, so a group is 2 rows x 4 threads at dwords
// 0, 8, 16, 24 and 2 LD mod 32 = 4 + the same: conflict-free (8 contiguous k's per thread would be 2-way).
// B ring: R register slots of 2 doubles.  The fragment of k4-step s is loaded D steps ahead into slot s % R.  R == D: the load
// of step s + D is issued right BEHIND the 8 MFMAs of step s, into the slot they read (they have issued, hence read it).
// D == 3: R = 4 (R must divide the k4-steps of a k-step for static register indices), the load goes in FRONT of the MFMAs.
// Loads beyond the last k4-step re-read the last one (clamped, never consumed): every step issues the same two loads, so the
// waits stay counted: the B fragment of step s is followed in issue order by the 2 (D - 1) (R == D) or 2 D (R != D) loads of
// the later steps, plus the NA / 2 A loads of the k-step when they went out in between -- in-order return makes
// s_waitcnt vmcnt(that count) wait for exactly step s.  (The compiler derives these counts itself: see the ISA.)
template <int BKT, int D, int F = 0>
__global__ __launch_bounds__(NT, 4) void gemm_bd(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C,
                                                 int n, int N, int K) {
  constexpr int LD = BKT + 2, IMG = BM * LD, KS = BKT / 4, R = (D == 3) ? 4 : D, NA = BKT / 4;
  static_assert(KS % R == 0, "static ring slots");
  __shared__ __attribute__((aligned(16))) double la[2][IMG];
  const int tiles_n = N / BN;
  int v = blockIdx.x;
  const int ntiles = (n / BM) * tiles_n;
  if ((ntiles & 7) == 0) { const int cpx = ntiles >> 3; v = (v & 7) * cpx + (v >> 3); }
  const int ti = v / tiles_n, tj = v - ti * tiles_n, i0 = ti * BM, j0 = tj * BN;
  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6), lr = lane & 15, lk = lane >> 4;
  const int wm = w >> 2, wn = w & 3, blr = 4 * (lr & 3) + (lr >> 2);
  f64x4 acc[4][2];
  for (int a = 0; a < 4; ++a)
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0, 0, 0, 0};
  double ra[NA];
  const int ar = t >> 2, ak = (t & 3) * 4;   // thread: row t/4, k's (t%4)*4..+3 (and 16 + the same at BKT = 32)
  const double* pa = A + (long long)(i0 + ar) * K + ak;
  auto load = [&](int k0) {   // (beyond the last k-step: the last one again, never staged -- unconditional, so the waits stay counted)
    k0 = min(k0, K - BKT);
#pragma unroll
    for (int i = 0; i < NA / 2; ++i) {
      const f64x2 x = *reinterpret_cast<const f64x2*>(pa + k0 + (i >> 1) * 16 + (i & 1) * 2);
      ra[2 * i] = x.x, ra[2 * i + 1] = x.y;
    }
  };
  auto stage = [&](int buf) {
    double* sa = &la[buf][ar * LD + ak];
#pragma unroll
    for (int i = 0; i < NA / 2; ++i) *reinterpret_cast<f64x2*>(sa + (i >> 1) * 16 + (i & 1) * 2) = f64x2{ra[2 * i], ra[2 * i + 1]};
  };
  const unsigned boff = (unsigned)(lk * N + j0 + wn * 32 + blr);   // the lane's part of the B address (the k part is uniform)
  double fb[R][2];
  const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(B), 0, (int)(sizeof(double) * K * N), 0x00020000);
  auto bload = [&](int k, int slot) {
    if (F & 2) k = 0;                                // ablation: the same 4 k rows every step (timing only)
    k = min(k, K - 4);
    if (F & 4) {                                     // buffer loads: lane offset in a VGPR, the k part in an SGPR, no address VALU
      const int so = __builtin_amdgcn_readfirstlane(k * N * (int)sizeof(double));
      fb[slot][0] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(brs, (int)(boff * sizeof(double)), so, 0));
      fb[slot][1] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(brs, (int)((boff + 16) * sizeof(double)), so, 0));
      return;
    }
    const double* q = B + (long long)k * N;
    fb[slot][0] = q[boff];
    fb[slot][1] = q[boff + 16];
  };
  double ga[2][4];
  auto frag = [&](int buf, int kk, int s) {
    const double* fpa = &la[buf][(wm * 64 + lr) * LD + kk * 4 + lk];
#pragma unroll
    for (int i = 0; i < 4; ++i) ga[s][i] = fpa[i * 16 * LD];
  };
  auto mm8 = [&](int s, int slot) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[slot][b], ga[s][a], acc[a][b], 0, 0, 0);
  };
  int cur = 0;
  load(0);
  stage(0);
  load(BKT);
#pragma unroll
  for (int d = 0; d < D; ++d) bload(4 * d, d % R);
  __syncthreads();
  frag(0, 0, 0);
  for (int k0 = 0; k0 < K; k0 += BKT) {
    const bool more = k0 + BKT < K;
#pragma unroll
    for (int kk = 0; kk < KS; ++kk) {
      if (kk < KS - 1) {
        frag(cur, kk + 1, (kk + 1) & 1);
      } else {
        __syncthreads();
        if (more) frag(cur ^ 1, 0, 0);
      }
      if (R != D && !(F & 1)) bload(k0 + 4 * (kk + D), (kk + D) % R);
      SB;
      mm8(kk & 1, kk % R);
      SB;
      if (R == D && !(F & 1)) bload(k0 + 4 * (kk + D), kk % R);   // (F & 1: ablation, fragments reused: timing only)
      if (kk == 0) {
        if (more) stage(cur ^ 1);
        load(k0 + 2 * BKT);
      }
      SB;
    }
    cur ^= 1;
  }
  store_tile(C, N, i0, j0, wm, wn, lr, lk, acc);
}

int main() {
  const int n = 131072, N = 1024, K = 1024;
  double *A, *B, *C;
  hipMalloc(&A, sizeof(double) * (size_t)n * K), hipMalloc(&B, sizeof(double) * (size_t)K * N), hipMalloc(&C, sizeof(double) * (size_t)n * N);
  std::vector<double> h((size_t)n * K);
  unsigned long long s = 88172645463325252ULL;
  for (auto& x : h) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; x = (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; }
  hipMemcpy(A, h.data(), sizeof(double) * (size_t)n * K, hipMemcpyHostToDevice);
  hipMemcpy(B, h.data(), sizeof(double) * (size_t)K * N, hipMemcpyHostToDevice);
  hipEvent_t e0, e1;
  hipEventCreate(&e0), hipEventCreate(&e1);
  const int blocks = (n / BM) * (N / BN);
  const char* names[] = {"today's loop (A, B images, BK = 16)", "B direct D = 2, A image BK = 16", "B direct D = 2, A image BK = 32",
                         "B direct D = 3, A image BK = 32", "B direct D = 4, A image BK = 32",
                         "  D = 4, BK = 32, global_load (64-bit lane addresses)", "  D = 4, BK = 32, B rows 0..3 only (timing only)",
                         "  D = 4, BK = 32, no B loads (timing only)"};
  const int rows[] = {12345, 131071, 0}, cols[] = {100, 1023, 77};
  for (int pass = 0; pass < 3; ++pass)     // pass 0 warms the device up (clocks): only passes 1 and 2 are printed
    for (int variant = 0; variant < 8; ++variant) {
      auto run = [&] {
        switch (variant) {
          case 0: hipLaunchKernelGGL(gemm_lds, dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 1: hipLaunchKernelGGL((gemm_bd<16, 2, 4>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 2: hipLaunchKernelGGL((gemm_bd<32, 2, 4>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 3: hipLaunchKernelGGL((gemm_bd<32, 3, 4>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 4: hipLaunchKernelGGL((gemm_bd<32, 4, 4>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 5: hipLaunchKernelGGL((gemm_bd<32, 4, 0>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 6: hipLaunchKernelGGL((gemm_bd<32, 4, 6>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
          case 7: hipLaunchKernelGGL((gemm_bd<32, 4, 5>), dim3(blocks), dim3(NT), 0, 0, A, B, C, n, N, K); break;
        }
      };
      hipMemset(C, 0, sizeof(double) * (size_t)n * N);
      run();
      if (hipDeviceSynchronize() != hipSuccess) { printf("variant %d: %s\n", variant, hipGetErrorString(hipGetLastError())); return 1; }
      hipEventRecord(e0);
      for (int i = 0; i < 10; ++i) run();
      hipEventRecord(e1);
      hipEventSynchronize(e1);
      float ms;
      hipEventElapsedTime(&ms, e0, e1);
      ms /= 10;
      double err = 0, c0 = 0;
      for (int q = 0; q < 3; ++q) {
        double c;
        hipMemcpy(&c, C + rows[q] * (size_t)N + cols[q], sizeof(double), hipMemcpyDeviceToHost);
        double ref = 0;
        for (int k = 0; k < K; ++k) ref += h[(size_t)rows[q] * K + k] * h[(size_t)k * N + cols[q]];
        err = fmax(err, fabs(c - ref));
        if (q == 0) c0 = c;
      }
      if (pass) printf("pass %d  %-40s %.3f ms  %.2f TFLOP/s   C[12345][100] = %.17g   max|err| %.2e\n", pass, names[variant], ms,
                       2.0 * n * N * K / ms / 1e9, c0, err);
      fflush(stdout);
    }
  return 0;
}
