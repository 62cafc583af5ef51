// gemm_rowpass.hip -- the two row-pass contractions of the svmogp_inf path as SPECIALISED FP64-MFMA kernels (gfx950):
//   forward   P~ = K^ C_q  (+ fused row statistics)      n x M x M, A row-major, B k-major        svmogp_inf.py:212-218
//   Gram      H_q += K^T diag(beta) K^ (lower tiles)     M x M x n, both operands k-major, split over n   :145-147
// Same block tile (128 x 128 x 16), LDS images, XCD-aware block order and fused epilogue as the general kernel
// (gemm_f64.hip), but
//   * EIGHT waves per block, wave tile 64 x 32 (8 accumulators, <= 128 VGPRs): two blocks per CU = FOUR waves per SIMD.
//     One wave per SIMD reaches half the FP64-MFMA rate, two reach all of it (tools/probes/probe_coissue.hip): with two
//     waves per SIMD every barrier / waitcnt stall of one idles half the pipe; four leave slack
//     (tools/probes/probe_gemm8.hip: 67.8 vs 64.0 TFLOP/s on the bare loop);
//   * a branch-free main loop: full 128-column tiles and a k-extent that is a multiple of 16 are REQUIRED of the
//     inducing dimension (gemm_rowpass_eligible; anything else takes the general kernel), ragged ROWS are handled by
//     clamping the row index once per thread (forward) or by a zero k-scale (Gram), so a k-step is: 2-4 vector loads,
//     32 MFMAs fed by 12 ds_read, 2-4 ds_write, one barrier -- no per-step bookkeeping;
//   * [r7] the plain forward (rowpass_gemm_kernel<1>) takes C_q's fragments straight from L2 into registers and spends the LDS on
//     an A image of BK = 32: 64 MFMAs fed by 32 ds_read + 16 buffer loads, 4 ds_write, one barrier (see "B DIRECT" below).
//   * [r8] the Gram (rowpass_gemm_kernel<2>, gram_tile) takes the fragments of its UNSCALED operand straight from global memory
//     and spends the LDS on a k-major image of the scaled one at BK = 32, wave tile 16 x 128: 64 MFMAs fed by 64 ds_read + 8
//     buffer loads, 4 ds_write, one barrier (see "I DIRECT" below).
#include <cstdlib>

#include "common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 16, W = 8, NT = W * 64;
constexpr int KM_LD = 144, RM_LD = 18, TILE_DOUBLES = BK * KM_LD;   // LDS images: see gemm_f64.hip
constexpr int NB = 2, WN = 32, NWN = 4;                              // wave tile 64 x 32 = 4 x 2 sub-tiles; 4 wave columns
constexpr int BK32 = 32, A32_LD = 34, BD_D = 2;                      // plain forward, B direct: A image at BK = 32, B ring depth
constexpr int GB = 8, GBG = 4, G_D = 2;                              // Gram: wave tile 16 x 128 = 1 x 8 sub-tiles, read in groups of 4; ring depth

struct Tile {
  double a[2][TILE_DOUBLES];
  double b[2][TILE_DOUBLES];
};

// Diagonal tiles of the lower-only Gram: wave w -> 16-row band wm of the tile, which needs the sub-tiles J <= wm, i.e. wm + 1 of 8.
// Bands 7, 6, 5, 4, 0, 1, 2, 3: the two waves of every SIMD (w and w + 4) carry 8 + 1, 7 + 2, 6 + 3, 5 + 4 = 9 of the 36 needed
// sub-tiles each, instead of 16.
__device__ __forceinline__ int diag_wm(int w) { return w < 4 ? 7 - w : w - 4; }

// One 128 x 128 tile of the forward contraction: main loop + epilogue (everything the kernel does once it knows its tile).
template <bool FOLD = false, bool BD = false>
__device__ __forceinline__ void rowpass_tile(const GemmArgs& g, int tiles_n, int ti, int tj, int split, Tile& lds, double* epi_a) {
  const int batch = blockIdx.z;
  const int M = g.M, N = g.N, K = g.K;
  const int i0 = ti * BM, j0 = tj * BN;
  if (i0 >= M || j0 >= N) return;
  int wlo = 0;
  if (g.b_tri > 0) wlo = j0;                                   // triangular fold of C: op(B)[k][j] == 0 for k < j
  const int ksteps = (K - wlo + BK - 1) / BK;
  const int per = (ksteps + g.ksplit - 1) / g.ksplit;
  const int kbeg = wlo + split * per * BK;
  const int kend = min(K, kbeg + per * BK);

  const double* __restrict__ A = g.A + (long long)batch * g.sA;
  const double* __restrict__ B = g.B + (long long)batch * g.sB;
  double* __restrict__ C = g.C + (long long)batch * g.sC + (long long)split * g.sSplit;
  double* fs_part = g.fs_part ? g.fs_part + (long long)batch * g.fs_sPart : nullptr;

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  const int wm = w >> 2;
  int wn = w & 3;
  // [r5] Triangular fold: inside the DIAGONAL 128-row block of C's fold (k in [j0, j0 + 128)) the wave column wn only meets
  // non-zero entries from k = j0 + 32 wn on (op(B)[k][j] == 0 for k < j), so its MFMAs of the earlier k-steps are skipped: 8, 6,
  // 4, 2 of the block's 8 k-steps for wn = 0 .. 3 (products with exact zeros: the accumulators keep their bits).  Waves w and
  // w + 4 share a SIMD, so the upper four take the wave columns in REVERSE order: every SIMD carries 10 of 16 wave-steps.
  // (FOLD: the paired kernel only -- the plain forward instantiation keeps its code)
  if (FOLD && w >= 4) wn = 3 - wn;
  const int klive = FOLD ? j0 + 32 * wn : 0;                    // first k-step whose MFMAs this wave issues
  // The forward contraction accumulates the TRANSPOSED sub-tiles (MFMA operands swapped, B fragment columns permuted): lane
  // (lr, lk) register r of acc[a][b] holds P~[wm*64 + a*16 + lr][wn*32 + b*16 + 4*lk + r] -- a lane owns 4 adjacent columns
  // of ONE row, so the fused row statistics are in-lane sums + two shuffles and P~ leaves as 16-byte stores.
  const int blr = 4 * (lr & 3) + (lr >> 2);

  f64x4 acc[4][NB];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};

  // ---- operand streams: 4 doubles per thread, operand and k-step ------------------------------------------------------
  // A row-major (thread: row t/4, k's (t%4)*4..+3; rows beyond the matrix read the last row, never stored),
  // B k-major   (thread: k row t/32, column pairs (t%32)*2 and +64)
  const int ar = t >> 2, ak = (t & 3) * 4, bk = t >> 5, bc = (t & 31) * 2;
  const double* pa = A + (long long)min(i0 + ar, M - 1) * g.lda + ak;
  const double* pb = B + (long long)bk * g.ldb + j0 + bc;
  double ra[4], rb[4];
  auto load = [&](int k0) {
    const f64x2 x0 = *reinterpret_cast<const f64x2*>(pa + k0), x1 = *reinterpret_cast<const f64x2*>(pa + k0 + 2);
    ra[0] = x0.x, ra[1] = x0.y, ra[2] = x1.x, ra[3] = x1.y;
    const double* q = pb + (long long)k0 * g.ldb;
    const f64x2 y0 = *reinterpret_cast<const f64x2*>(q), y1 = *reinterpret_cast<const f64x2*>(q + 64);
    rb[0] = y0.x, rb[1] = y0.y, rb[2] = y1.x, rb[3] = y1.y;
  };
  auto stage = [&](int buf) {
    double* sa = &lds.a[buf][ar * RM_LD + ak];
    *reinterpret_cast<f64x2*>(sa) = f64x2{ra[0], ra[1]};
    *reinterpret_cast<f64x2*>(sa + 2) = f64x2{ra[2], ra[3]};
    double* sb = &lds.b[buf][bk * KM_LD + bc];
    *reinterpret_cast<f64x2*>(sb) = f64x2{rb[0], rb[1]};
    *reinterpret_cast<f64x2*>(sb + 64) = f64x2{rb[2], rb[3]};
  };
  // MFMA operands ("fragments") of one k4-step: 4 A values + NB B values per lane, read from the LDS images into register set s
  double fa[2][4], fb[2][NB];
  auto frag = [&](int buf, int kk, int s) {
    const double* fpa = &lds.a[buf][(wm * 64 + lr) * RM_LD + kk * 4 + lk];
    const double* fpb = &lds.b[buf][(kk * 4 + lk) * KM_LD + wn * WN + blr];
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[s][i] = fpa[i * 16 * RM_LD];
#pragma unroll
    for (int i = 0; i < NB; ++i) fb[s][i] = fpb[i * 16];
  };
  auto mm8 = [&](int s) {
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fb[s][b], fa[s][a], acc[a][b], 0, 0, 0);
  };

  // ---- [r7] plain forward, B DIRECT (BD): C_q's fragments straight from L2 into registers, A image at BK = 32 ---------------
  // C_q is the one operand every block of the launch shares and its MFMA fragment is a coalesced access as it lies in memory
  // (for a fixed k the 16 lanes lr read 16 adjacent doubles): registers -> ds_write -> ds_read was a copy.  Without the B image
  // the LDS takes a double-buffered row-major A image of 128 x 32: ONE block barrier per 64 MFMAs per wave instead of one
  // per 32.  tools/probes/probe_gemm_bdirect.hip, profiles/r07_gemm_bdirect.txt: 69.5 -> 71.5 TFLOP/s on the bare loop.
  //   * A image: row stride A32_LD = 34 doubles.  A fragment read is one ds_read_b64 per lane at dword 68 lr + 2 lk (+ const):
  //     68 lr mod 64 runs through the 16 multiples of 4, so the 32 lanes of a half wave (lk in {0, 1} / {2, 3}) hit 64 distinct
  //     banks.  The stage writes are ds_write_b128: groups of 8 lanes, banks mod 32.  A thread writes the k's (t%4)*4..+3 and
  //     16 + the same of row t/4 (as the staged loop does within its 16): per group 2 rows x 4 threads at dwords 0, 8, 16, 24
  //     and 4 + the same (68 mod 32) -- conflict-free; 8 CONTIGUOUS k's per thread put threads 16 dwords apart: 2-way, measured
  //     as SQ_LDS_BANK_CONFLICT 0.235 of the LDS cycles.  2 x 128 x 34 = 8704 doubles of the tile buffers' 9216; the epilogue's
  //     staging needs 8192.
  //   * B fragments: lane (lr, lk) of wave column wn loads B[(k + lk) ldb + j0 + 32 wn + 16 b + blr], b < 2, for the k4-step at
  //     k, as two buffer_load_dwordx2 (lane part of the address in a VGPR that never changes, k ldb in an SGPR: no address
  //     arithmetic on the vector pipe; the same loads with 64-bit lane addresses measured 69.6).  They run BD_D = 2 k4-steps
  //     ahead of the MFMAs that consume them, in a ring of BD_D register slots: the loads of step s + BD_D are issued right
  //     BEHIND the 8 MFMAs of step s, into the slot those have read.  (D = 2, 3, 4 measured 71.5, 71.0, 71.5: the shallowest.)
  //   * waits: counted s_waitcnt vmcnt(n) on in-order return.  Every k4-step issues exactly its two B loads and every k-step
  //     exactly its four A loads (beyond the last step they re-read the last one: clamped, never consumed), so in front of the
  //     MFMAs of step s the loads issued AFTER B(s) are: B(s + 1) [2], and in the step behind the A loads those too [4]:
  //     vmcnt(2) / vmcnt(6) can only be satisfied once B(s) has landed (vmcnt(3) / (7) for its first half).  The A loads are
  //     older than every B fragment waited for from the third k4-step behind them on, so the stage of the next k-step needs
  //     no wait of its own.  The compiler derives exactly these counts from the straight-line code (there is no conditional
  //     load in the loop, which would make it fall back to the smaller count); they are not written by hand.
  //   * same products in the same order per accumulator (k ascending, k4 grouping 4 kk + lk, operands swapped): P~, p and c are
  //     bit-identical to the staged loop.
  if constexpr (BD) {
    static_assert(!FOLD, "B direct: the plain forward only");
    constexpr int KS = BK32 / 4, NA = BK32 / 4;
    static_assert(KS % BD_D == 0, "static ring slots");
    static_assert(2 * BM * A32_LD <= 4 * TILE_DOUBLES, "A image at BK = 32 fits the tile buffers");
    double* const img = &lds.a[0][0];                          // [2][BM * A32_LD]
    const int ar32 = t >> 2, ak32 = (t & 3) * 4;              // thread: row t/4, k's (t%4)*4..+3 and 16 + the same
    const double* pa32 = A + (long long)min(i0 + ar32, M - 1) * g.lda + ak32;
    double r32[NA];
    auto load32 = [&](int k0) {
      k0 = min(k0, kend - BK32);
#pragma unroll
      for (int i = 0; i < NA / 2; ++i) {
        const f64x2 x = *reinterpret_cast<const f64x2*>(pa32 + k0 + (i >> 1) * 16 + (i & 1) * 2);
        r32[2 * i] = x.x, r32[2 * i + 1] = x.y;
      }
    };
    auto stage32 = [&](int buf) {
      double* sa = img + buf * (BM * A32_LD) + ar32 * A32_LD + ak32;
#pragma unroll
      for (int i = 0; i < NA / 2; ++i) *reinterpret_cast<f64x2*>(sa + (i >> 1) * 16 + (i & 1) * 2) = f64x2{r32[2 * i], r32[2 * i + 1]};
    };
    // (launch_gemm_rowpass takes this loop only if the whole B panel is addressable with 32-bit byte offsets)
    const __amdgpu_buffer_rsrc_t brs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<double*>(B), 0, (int)(sizeof(double) * ((long long)(K - 1) * g.ldb + N)), 0x00020000);
    const int bvo = (int)sizeof(double) * (lk * g.ldb + j0 + wn * WN + blr);
    double gb[BD_D][NB];
    auto bload = [&](int k, int slot) {
      const int so = __builtin_amdgcn_readfirstlane(min(k, kend - 4) * g.ldb * (int)sizeof(double));
#pragma unroll
      for (int b = 0; b < NB; ++b)
        gb[slot][b] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(brs, bvo + b * 16 * (int)sizeof(double), so, 0));
    };
    double ga[2][4];
    auto frag32 = [&](int buf, int kk, int s) {
      const double* fpa = img + buf * (BM * A32_LD) + (wm * 64 + lr) * A32_LD + kk * 4 + lk;
#pragma unroll
      for (int i = 0; i < 4; ++i) ga[s][i] = fpa[i * 16 * A32_LD];
    };
    auto mm32 = [&](int s, int slot) {
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(gb[slot][b], ga[s][a], acc[a][b], 0, 0, 0);
    };
    int cur = 0;
    if (kbeg < kend) {
      load32(kbeg);
      stage32(0);
      load32(kbeg + BK32);
#pragma unroll
      for (int d = 0; d < BD_D; ++d) bload(kbeg + 4 * d, d);
    }
    __syncthreads();
    if (kbeg < kend) frag32(0, 0, 0);
    for (int k0 = kbeg; k0 < kend; k0 += BK32) {
      const bool more = k0 + BK32 < kend;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
        if (kk < KS - 1) {
          frag32(cur, kk + 1, (kk + 1) & 1);
        } else {                                               // (behind the last barrier of the tile no wave reads LDS any more)
          __syncthreads();
          if (more) frag32(cur ^ 1, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        mm32(kk & 1, kk % BD_D);
        __builtin_amdgcn_sched_barrier(0);
        bload(k0 + 4 * (kk + BD_D), kk % BD_D);
        if (kk == 0) {
          if (more) stage32(cur ^ 1);
          load32(k0 + 2 * BK32);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      cur ^= 1;
    }
  }

  // Software pipeline: the operands of step k + 1 are in registers when step k starts; they are staged into the other LDS
  // buffer BEFORE the MFMA block of step k (so the ds_write latency is covered by it and the barrier follows the last MFMA
  // directly) and the registers are refilled at once with step k + 2.
  int cur = 0;
  if (!BD && kbeg < kend) {
    load(kbeg);
    stage(0);
    if (kbeg + BK < kend) load(kbeg + BK);
  }
  if (!BD) __syncthreads();
  // [r4] Main loop with the fragments ONE k4-step AHEAD OF THE MFMAs AND CARRIED ACROSS THE BARRIER: the fragments of the next
  // tile's first k4-step are read right behind the barrier, in front of the last 8 MFMAs of the current tile, and the staging
  // of step k + 1 / the global loads of step k + 2 sit behind the first 8 MFMAs -- a wave never waits for LDS (or for the
  // ds_write -> ds_read turn-around at the top of a step) without 8 MFMAs of its own in flight.  Ablation of the bare loop
  // (tools/probes/probe_gemm_abl.hip, profiles/r04_gemm_ablation.txt): 66.3 -> 70.8 TFLOP/s; the same loop without any
  // barrier (racy) 72.5, MFMAs alone in this tile structure 73.6.  Same operations on the same values in the same order per
  // accumulator: results are bit-identical to the round-3 loop.
  if (!BD && kbeg < kend && (!FOLD || kbeg >= klive)) frag(0, 0, 0);
#define HM_SB __builtin_amdgcn_sched_barrier(0)
  for (int k0 = kbeg; !BD && k0 < kend; k0 += BK) {
    const bool more = k0 + BK < kend;
    const bool lv = !FOLD || k0 >= klive;                      // (wave-uniform; always true outside the fold's diagonal block)
    if (lv) {
      frag(cur, 1, 1);
      HM_SB;
      mm8(0);
      HM_SB;
    }
    if (more) stage(cur ^ 1);
    if (k0 + 2 * BK < kend) load(k0 + 2 * BK);
    HM_SB;
    if (lv) {
      frag(cur, 2, 0);
      HM_SB;
      mm8(1);
      HM_SB;
      frag(cur, 3, 1);
      HM_SB;
      mm8(0);
      HM_SB;
    }
    __syncthreads();
    if (more && (!FOLD || k0 + BK >= klive)) frag(cur ^ 1, 0, 0);
    if (lv) {
      HM_SB;
      mm8(1);
      HM_SB;
    }
    cur ^= 1;
  }
#undef HM_SB

  // ---- epilogue: D fragment of v_mfma_f64_16x16x4_f64: col = lane&15, row = (lane>>4) + 4*reg --------------------------
  if (fs_part && g.fs_sq) {
    // [r5] strict q(f): the only statistic is rowsum(T .* T) of the product itself -- in-lane squares of the lane's 8 values per
    // slice + the two shuffles over the four lanes of a row; same partial layout as `c` below (slot 1 of [stat][4 tiles_n][M])
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      double sq = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) sq = fma(acc[a][b][r], acc[a][b][r], sq);
      sq += __shfl_xor(sq, 16, 64);
      sq += __shfl_xor(sq, 32, 64);
      const int rl = wm * 64 + a * 16 + lr;
      if (lk == 0 && i0 + rl < M) fs_part[((long long)NWN * tiles_n + NWN * tj + wn) * M + (i0 + rl)] = sq;
    }
    if (!g.store_c) return;
  } else if (fs_part) {
    // Fused row statistics (GemmArgs::fs_*): lane (lr, lk) owns row rl = wm*64 + a*16 + lr and the column quads
    // wn*32 + b*16 + 4*lk + (0..3), b < 2, of slice a; it re-reads exactly its own 8 values of the K^ tile per slice
    // (L2/MALL-warm) with LDS-DMA loads (global_load_lds_dwordx4: lane l's 16 bytes land at base + 16*l) into a
    // wave-private double buffer -- no VGPRs, no block barriers.  Slices 0 and 1 are issued up front, slice a + 2 as soon as
    // slice a has been consumed (into the buffer it frees): every slice but the first has two consumption periods to land
    // in.  The waits count on loads returning in order: s_waitcnt vmcnt(4) with [slice a | stores | slice a + 1] outstanding
    // can only be satisfied once slice a has landed (were one of its 4 loads outstanding, so were all 4 of slice a + 1).
    // [r5] TWO statistics (p = K^ a, c = rowsum(P~ .* K^)).  Their r2-weighted twins (only ever consumed as the scalar sl of the
    // lengthscale gradient) moved to colstats_kernel, which forms E_nm and x_n - z_m anyway: no per-element distances, no
    // `hyper` branch and no inputs staged here any more.
    constexpr int NCH = 2 * NB, WSTAGE = 2 * NCH * 128;
    double* flat = &lds.a[0][0];                  // Tile = 4 * TILE_DOUBLES contiguous doubles
    double* stg = flat + w * WSTAGE;              // [2 buffers][NCH chunks][64 lanes][2]
    static_assert(W * WSTAGE <= 4 * TILE_DOUBLES, "epilogue scratch fits the tile buffers");
    const int colq = j0 + wn * WN + 4 * lk;       // + b*16 (+ 2h)
    const double* __restrict__ Ke = g.fs_k ? g.fs_k + (long long)batch * g.sA : A;   // (strict q(f): K^ is not this product's A operand)
    auto issue = [&](int a) {
      const int grow = min(i0 + wm * 64 + a * 16 + lr, M - 1);
      const double* src = Ke + (long long)grow * g.lda + colq;
      double* dst = stg + (a & 1) * (NCH * 128);
#pragma unroll
      for (int c = 0; c < NCH; ++c)               // chunk c = 2*b + h
        __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(src + (c >> 1) * 16 + (c & 1) * 2),
                                         (void __attribute__((address_space(3)))*)(dst + c * 128), 16, 0, 0);
    };
    issue(0);
    issue(1);
    if (t < 128) epi_a[t] = g.fs_a[(long long)batch * g.fs_sA + j0 + t];
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (a < 3) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");   // slice a has landed; slice a + 1 may still be in flight
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const int rl = wm * 64 + a * 16 + lr;
      double sp = 0.0, sc = 0.0;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const int cl = wn * WN + b * 16 + 4 * lk;  // this lane's 4 adjacent columns of sub-tile b (within the tile)
        const double* kp = stg + (a & 1) * (NCH * 128) + (2 * b) * 128 + 2 * lane;
        const f64x2 k01 = *reinterpret_cast<const f64x2*>(kp), k23 = *reinterpret_cast<const f64x2*>(kp + 128);
        const double kv[4] = {k01.x, k01.y, k23.x, k23.y};
        const f64x2 a01 = *reinterpret_cast<const f64x2*>(epi_a + cl), a23 = *reinterpret_cast<const f64x2*>(epi_a + cl + 2);
        const double av[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          sp += kv[r] * av[r];
          sc += acc[a][b][r] * kv[r];
        }
      }
#pragma unroll
      for (int o = 16; o <= 32; o <<= 1) {           // the four lanes (lk) that share this row
        sp += __shfl_xor(sp, o, 64);
        sc += __shfl_xor(sc, o, 64);
      }
      if (lk == 0 && i0 + rl < M) {                  // partial of (column tile, wave column): [stat][4 * tiles_n][M]
        double* o = fs_part + ((long long)(NWN * tj + wn)) * M + (i0 + rl);
        const long long ss = (long long)NWN * tiles_n * M;
        o[0] = sp, o[ss] = sc;
      }
      if (a < 2) {                                   // slice a is consumed: its buffer takes slice a + 2
        asm volatile("" ::: "memory");
        issue(a + 2);
      }
    }
    if (!g.store_c) return;
  }
  // lane (lr, lk): row wm*64 + a*16 + lr, columns wn*32 + b*16 + 4*lk + (0..3)
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int row = i0 + wm * 64 + a * 16 + lr;
    if (row >= M) continue;
    double* crow = C + (long long)row * g.ldc + j0 + wn * WN + 4 * lk;
    if (g.c_sub) {   // [r5] C -= op(A) op(B): the 128-column updates of the strict mode's blocked triangular solves
      // (c_src: the columns' FIRST touch reads them from the matrix the solve started from -- no copy of it beforehand)
      const double* srow = g.c_src ? g.c_src + (long long)batch * g.sC + (long long)row * g.ldc + j0 + wn * WN + 4 * lk : crow;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        const f64x2 c01 = *reinterpret_cast<const f64x2*>(srow + b * 16), c23 = *reinterpret_cast<const f64x2*>(srow + b * 16 + 2);
        *reinterpret_cast<f64x2*>(crow + b * 16) = f64x2{c01.x - acc[a][b][0], c01.y - acc[a][b][1]};
        *reinterpret_cast<f64x2*>(crow + b * 16 + 2) = f64x2{c23.x - acc[a][b][2], c23.y - acc[a][b][3]};
      }
      continue;
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      *reinterpret_cast<f64x2*>(crow + b * 16) = f64x2{acc[a][b][0], acc[a][b][1]};
      *reinterpret_cast<f64x2*>(crow + b * 16 + 2) = f64x2{acc[a][b][2], acc[a][b][3]};
    }
  }
}

// One 128 x 128 tile of one row range of the weighted Gram H += A^T diag(s) B (both operands k-major over the same rows): main
// loop + slab store.
// ---- [r8] I DIRECT: the unscaled operand's fragments straight from global memory, the scaled one as an image at BK = 32 --------
// For a fixed row k the 16 lanes lr of a fragment read 16 adjacent doubles of a k-major operand as they lie in memory: registers
// -> ds_write -> ds_read was a copy for either operand.  With the i-side (MFMA operand A, unscaled) direct, the tile buffers
// hold the j-side s_k b_kj as ONE double-buffered k-major image of 32 rows (2 x 32 x KM_LD doubles: the footprint of the two
// BK = 16 image pairs it replaces): one block barrier per 64 MFMAs per wave instead of one per 32.
// tools/probes/probe_gram_direct.hip, profiles/r08_gram_direct.txt (2 M rows streamed from HBM): 68.2 -> 70.5 TFLOP/s.
//   * wave tile 16 x 128 (one sub-tile of the i-side, GB = 8 of the j-side; 8 x 1 wave tiles): the eight waves load disjoint
//     16-column bands of the direct operand -- ONE load and a ring of G_D doubles per k4-step, no panel byte fetched twice by a
//     block.  The image costs eight ds_read_b64 per k4-step (dword 288 lk + 2 lr + const: the half waves lk in {0, 1} / {2, 3}
//     hit 64 distinct banks, as before), read in two groups of GBG = 4 in front of their 4 MFMAs (8 fragment registers, not 16).
//     In the step: 32 x 64 with two loads per k4-step -0.5 ms, 64 x 32 with four over the register cap.
//   * direct loads: lane (lr, lk) of band wm loads A[(k + lk) lda + i0 + 16 wm + lr] for the k4-step at k as one
//     buffer_load_dwordx2 -- the lane part of the address in a VGPR, (k - kbeg) lda in an SGPR.
//     The resource is based at the block's first row of its range and its column panel, so 32-bit byte offsets only have to span
//     ONE RANGE (gemm_rowpass_eligible checks that).  The loads run G_D = 2 k4-steps ahead of the MFMAs that consume them: the
//     load of step s + 2 is issued right behind the 8 MFMAs of step s into the slot those have read.
//   * image: a thread stages 4 doubles of k row t/32 of each 16-row HALF of the step; half h of step s + 1 is loaded four k4-steps
//     ahead of its ds_write into the ONE set of staging registers (4 doubles + the k-scale): h = 0 is written behind the first 8
//     MFMAs of step s and the registers refilled with h = 1, which is written behind the fifth 8 and the registers refilled with
//     h = 0 of step s + 2.  The lead of the BK = 16 loop at 10 staging registers instead of 18.  The k-scale is applied at stage
//     time (a multiply at load time makes the compiler wait for the loads in front of the MFMAs).
//   * no conditional load: image rows beyond the range read row min(row, K - 1) and get the k-scale 0 (so does the second half
//     of a step when the range ends on an odd multiple of 16: range boundaries are NOT moved); direct loads beyond the range's
//     last k4-step re-read it (consumed against the zero scale or not at all).  Where that last k4-step is the matrix's ragged
//     one (K % 4 != 0) the lane rows are clamped to K - 1: a second lane offset, selected on a scalar condition.  The compiler
//     derives counted s_waitcnt vmcnt(n) from the straight-line code: there is no vmcnt(0) in the loop (ISA checked).
//   * same products a_ki (s_k b_kj) in the same order per accumulator (k ascending from kbeg, k4 grouping 4 kk + lk; the added
//     half step contributes a * 0 to sums that start from + 0): H is bit-identical to the BK = 16 loop.
__device__ __forceinline__ void gram_tile(const GemmArgs& g, int ti, int tj, int split, Tile& lds) {
  const int batch = blockIdx.z;
  const int M = g.M, N = g.N, K = g.K;
  const int i0 = ti * BM, j0 = tj * BN;
  if (i0 >= M || j0 >= N) return;
  const int ksteps = (K + BK - 1) / BK;
  const int per = (ksteps + g.ksplit - 1) / g.ksplit;
  const int kbeg = split * per * BK;
  const int kend = min(K, kbeg + per * BK);

  const double* __restrict__ A = g.A + (long long)batch * g.sA;
  const double* __restrict__ B = g.B + (long long)batch * g.sB;
  const double* __restrict__ S = g.kscale + (long long)batch * g.sS;
  double* __restrict__ C = g.C + (long long)batch * g.sC + (long long)split * g.sSplit;

  const int t = threadIdx.x, lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  // (diagonal tiles: 9 needed sub-tiles per SIMD -- see diag_wm; only what lies on or below the diagonal is computed and stored)
  const bool diag = ti == tj && g.lower_only;
  const int wm = diag ? diag_wm(w) : w;                        // the wave's 16-row band of the tile
  const int nsub = diag ? wm + 1 : GB;                         // sub-tiles 0 .. nsub - 1 of the band are computed (wave-uniform)

  f64x4 acc[GB];
#pragma unroll
  for (int b = 0; b < GB; ++b) acc[b] = f64x4{0.0, 0.0, 0.0, 0.0};

  // image operand: thread = k row t/32 of each half, column pairs (t%32)*2 and + 64
  constexpr int KS = BK32 / 4, HALF = BK32 / 2;
  static_assert(KS % G_D == 0, "static ring slots");
  static_assert(2 * BK32 * KM_LD == 4 * TILE_DOUBLES, "the image at BK = 32 is the tile buffers");
  double* const img = &lds.a[0][0];                            // [2][BK32 * KM_LD]
  const int bk = t >> 5, bc = (t & 31) * 2;
  const double* pst = B + j0 + bc;
  double rs[4], ks;
  auto loadh = [&](int k0, int h) {
    const int row = min(k0 + HALF * h + bk, K - 1);
    const long long off = (long long)row * g.ldb;
    const f64x2 x0 = *reinterpret_cast<const f64x2*>(pst + off), x1 = *reinterpret_cast<const f64x2*>(pst + off + 64);
    rs[0] = x0.x, rs[1] = x0.y, rs[2] = x1.x, rs[3] = x1.y;
    ks = S[row];
  };
  auto stageh = [&](int buf, int k0, int h) {
    const double sc = (k0 + HALF * h + bk < kend) ? ks : 0.0;
    double* s = img + buf * (BK32 * KM_LD) + (HALF * h + bk) * KM_LD + bc;
    *reinterpret_cast<f64x2*>(s) = f64x2{rs[0] * sc, rs[1] * sc};
    *reinterpret_cast<f64x2*>(s + 64) = f64x2{rs[2] * sc, rs[3] * sc};
  };
  // direct operand (on diagonal tiles the same panel as the image's: no special case)
  const __amdgpu_buffer_rsrc_t ars = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<double*>(A + (long long)kbeg * g.lda + i0), 0, (int)sizeof(double) * ((kend - 1 - kbeg) * g.lda + BM), 0x00020000);
  const int klim = kbeg + 4 * ((kend - kbeg - 1) / 4);          // the range's last k4-step
  const int avo = (int)sizeof(double) * (lk * g.lda + wm * 16 + lr);
  const int avo_last = (int)sizeof(double) * (min(lk, K - 1 - klim) * g.lda + wm * 16 + lr);
  double ga[G_D];
  auto aload = [&](int k, int slot) {
    const int so = __builtin_amdgcn_readfirstlane((min(k, klim) - kbeg) * g.lda * (int)sizeof(double));
    ga[slot] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(ars, (k >= klim) ? avo_last : avo, so, 0));
  };
  if (kbeg < kend) {                                            // (an empty range loads nothing and still writes its zero slab tile)
    loadh(kbeg, 0);
    stageh(0, kbeg, 0);
    loadh(kbeg, 1);
    stageh(0, kbeg, 1);
    loadh(kbeg + BK32, 0);
#pragma unroll
    for (int d = 0; d < G_D; ++d) aload(kbeg + 4 * d, d);
  }
  __syncthreads();
  {
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BK32) {
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) {
#pragma unroll
        for (int gq = 0; gq < GB / GBG; ++gq) {
          if (gq * GBG >= nsub) continue;                      // (a band of a diagonal tile that ends in the first group)
          double fb[GBG];
          const double* fpb = img + cur * (BK32 * KM_LD) + (kk * 4 + lk) * KM_LD + gq * 16 * GBG + lr;
#pragma unroll
          for (int b = 0; b < GBG; ++b) fb[b] = fpb[b * 16];
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int b = 0; b < GBG; ++b) {
            if (gq * GBG + b >= nsub) continue;                // wave-uniform (scalar) guard; never taken off the diagonal
            acc[gq * GBG + b] = __builtin_amdgcn_mfma_f64_16x16x4f64(ga[kk % G_D], fb[b], acc[gq * GBG + b], 0, 0, 0);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        aload(k0 + 4 * (kk + G_D), kk % G_D);
        if (kk == 0) {
          stageh(cur ^ 1, k0 + BK32, 0);
          loadh(k0 + BK32, 1);
        }
        if (kk == KS / 2) {
          stageh(cur ^ 1, k0 + BK32, 1);
          loadh(k0 + 2 * BK32, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
      cur ^= 1;
    }
  }

  // ---- slab store: D fragment of v_mfma_f64_16x16x4_f64: col = lane&15, row = (lane>>4) + 4*reg ------------------------------
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    double* crow = C + (long long)(i0 + wm * 16 + 4 * r + lk) * g.ldc + j0 + lr;
#pragma unroll
    for (int b = 0; b < GB; ++b)
      if (b < nsub) crow[b * 16] = acc[b][r];
  }
}

template <int ROLE, bool PAIR, bool BD = false>
__device__ __forceinline__ void rowpass_block(const GemmArgs& g, int tiles_n, int ntiles, Tile& lds, double* epi_a) {

  // ---- which tile / batch / k-range (block b is observed to run on XCD b % 8: speed only) ----------------------------
  int v = blockIdx.x, split = 0;
  int ti, tj;
  if (ROLE == 2 && g.lower_only) {
    // Lower tiles of the Gram, in TWO phases of equal-duration blocks.  The tiles of one K range stream the same operand rows,
    // and they only share them through the XCD's L2 if they START together: blocks of unequal duration (a diagonal tile does
    // ~0.6 of the work) spread the start times of everything behind them and the sharing is lost (measured: 36 mixed tiles
    // per range run as slowly as 36 full ones).  So: first all strictly-lower tiles, range-major, all tiles of one K range on
    // ONE XCD (block b is observed to run on XCD b % 8: speed only); then the diagonal tiles, which share nothing (tile
    // (d, d) reads panel d only).
    const int T = tiles_n, noff = T * (T - 1) / 2, ks8 = (g.ksplit > 1) ? ((g.ksplit + 7) / 8) * 8 : 1, gx1 = noff * ks8;
    if (v < gx1) {
      int u = v;                                          // strictly-lower index: u = ti (ti - 1) / 2 + tj, tj < ti
      if (g.ksplit > 1) {
        const int xcd = v & 7, idx = v >> 3;
        split = (idx / noff) * 8 + xcd;
        u = idx % noff;
      }
      ti = (int)((sqrt(8.0 * (double)u + 1.0) + 1.0) * 0.5);
      while (ti * (ti + 1) / 2 <= u) ++ti;
      while (ti * (ti - 1) / 2 > u) --ti;
      tj = u - ti * (ti - 1) / 2;
    } else {
      const int u = v - gx1;
      split = u / T;
      ti = tj = u - split * T;
    }
    if (split >= g.ksplit) return;
  } else {
    if (g.ksplit > 1) {               // all tiles of one K range on ONE XCD: they stream the same operand rows concurrently
      const int xcd = v & 7, idx = v >> 3;
      split = (idx / ntiles) * 8 + xcd;
      v = idx % ntiles;
      if (split >= g.ksplit) return;
    } else if ((ntiles & 7) == 0) {   // a contiguous range of tiles per XCD: the column tiles of a row panel share its A panel
      const int cpx = ntiles >> 3;
      v = (v & 7) * cpx + (v >> 3);
    }
    const int tcols = PAIR ? tiles_n / 2 : tiles_n;
    ti = v / tcols;
    tj = v - ti * tcols;
  }
  if constexpr (ROLE == 2) {
    gram_tile(g, ti, tj, split, lds);
    return;
  } else {
    rowpass_tile<PAIR, BD>(g, tiles_n, ti, tj, split, lds, epi_a);
  }
  // Triangular fold (b_tri > 0, the E-step's / predict_f's forward): the k-loop of column tile j starts at j, so the tiles of
  // a row panel do 8, 7, ... 1 eighths of a full tile's work.  In paired mode a block takes column tiles j and
  // tiles_n - 1 - j one after the other: every block does (tiles_n + 1) / tiles_n of a full tile -- equal durations.
  if (PAIR) {
    __syncthreads();                 // the epilogue of the first tile used the tile buffers as scratch
    rowpass_tile<PAIR>(g, tiles_n, ti, tiles_n - 1 - tj, split, lds, epi_a);
  }
}

// ROLE 1 = forward, ROLE 2 = weighted Gram (names the instantiation in profiles, like gemm_f64_kernel's ROLE)
template <int ROLE>
__global__ __launch_bounds__(NT, 4) void rowpass_gemm_kernel(GemmArgs g, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) Tile lds;
  __shared__ __attribute__((aligned(16))) double epi_a[ROLE == 1 ? 128 : 2];
  rowpass_block<ROLE, false, ROLE == 1>(g, tiles_n, ntiles, lds, epi_a);   // (forward: B direct)
}
// the forward contraction with BOTH operands staged through LDS (BK = 16): the C -= A B updates of the strict solves (k-extents
// that are multiples of 16 only), the unpaired triangular fold, B panels beyond 32-bit byte offsets
__global__ __launch_bounds__(NT, 4) void rowpass_fwd_staged_kernel(GemmArgs g, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) Tile lds;
  __shared__ __attribute__((aligned(16))) double epi_a[128];
  rowpass_block<1, false>(g, tiles_n, ntiles, lds, epi_a);
}
// the forward contraction against the triangular fold of C, two column tiles per block (see rowpass_block)
__global__ __launch_bounds__(NT, 4) void rowpass_fold_pair_kernel(GemmArgs g, int tiles_n, int ntiles) {
  __shared__ __attribute__((aligned(16))) Tile lds;
  __shared__ __attribute__((aligned(16))) double epi_a[128];
  rowpass_block<1, true>(g, tiles_n, ntiles, lds, epi_a);
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

// Can this contraction take the specialised kernel?  (full 128-column tiles of the inducing dimension, k-extent a
// multiple of 16 for the forward, even leading dimensions and 16-byte aligned operands, none of the general kernel's extras)
bool gemm_rowpass_eligible(const GemmArgs& g) {
  // [r5] role 1 also as the in-place update C -= op(A) op(B) (alpha = -1, beta = 1, no statistics, any k-extent that is a
  // multiple of 16): launch_gemm_rowpass sets c_sub
  const bool sub = g.role == 1 && g.alpha == -1.0 && g.beta == 1.0 && !g.fs_part && g.b_tri == 0 && g.store_c;
  if (g.nouter != 1 || (!sub && (g.alpha != 1.0 || g.beta != 0.0)) || g.win || g.M_last || g.N_last || g.K_last || g.a_tri) return false;
  if ((g.lda & 1) || (g.ldb & 1) || (g.ldc & 1) || !aligned16(g.A) || !aligned16(g.B) || !aligned16(g.C)) return false;
  if (g.c_src && (!sub || !aligned16(g.c_src))) return false;
  if (g.fs_k && (g.role != 1 || !g.fs_part || g.fs_sq || !aligned16(g.fs_k))) return false;
  if ((g.sA & 1) || (g.sB & 1) || (g.sC & 1) || (g.sSplit & 1)) return false;
  if (g.role == 1)
    return !g.a_kmajor && g.b_kmajor && !g.lower_only && g.ksplit == 1 && !g.kscale && g.b_tri >= 0 && (g.N % BN) == 0 &&
           (g.K % BK) == 0 && (g.K == g.N || sub) && g.K >= BK && g.M >= 1;
  if (g.role == 2) {
    // (the direct operand is addressed with 32-bit byte offsets from the first row of a block's row range: see gram_tile)
    const long long per = (((long long)g.K + BK - 1) / BK + g.ksplit - 1) / g.ksplit;
    return g.a_kmajor && g.b_kmajor && g.kscale && g.b_tri == 0 && g.M == g.N && (g.N % BN) == 0 &&
           g.lda == g.ldb && g.K >= 1 && g.ksplit >= 1 && ((per * BK + 4) * g.lda + BM) * (long long)sizeof(double) <= 0x7FFFFFFFLL;
  }
  return false;
}

void launch_gemm_rowpass(const GemmArgs& g_in, hipStream_t stream) {
  GemmArgs g = g_in;
  g.c_sub = (g.role == 1 && g.alpha == -1.0 && g.beta == 1.0) ? 1 : 0;
  const int tiles_m = (g.M + BM - 1) / BM, tiles_n = (g.N + BN - 1) / BN;
  const int ntiles = g.lower_only ? tiles_m * (tiles_m + 1) / 2 : tiles_m * tiles_n;
  const int gx = (g.ksplit > 1) ? ntiles * ((g.ksplit + 7) / 8) * 8 : ntiles;
  dim3 grid(gx, 1, g.nbatch);
  if (g.role == 1) {
    // triangular fold: column tiles paired (j, tiles_n - 1 - j) per block (see the kernel)
    const int pair = (g.b_tri > 0 && g.ksplit == 1 && tiles_n >= 2 && (tiles_n & 1) == 0) ? 1 : 0;
    if (pair) {
      grid.x = tiles_m * (tiles_n / 2);
      hipLaunchKernelGGL(rowpass_fold_pair_kernel, grid, dim3(NT), 0, stream, g, tiles_n, (int)grid.x);
    } else if (!g.c_sub && g.b_tri == 0 && (g.K % BK32) == 0 && ((long long)(g.K - 1) * g.ldb + g.N) * (long long)sizeof(double) <= 0x7FFFFFFFLL) {
      // plain forward: C_q's fragments straight from L2, A image at BK = 32 (needs k-extent % 32 == 0: holds whenever K == N)
      hipLaunchKernelGGL((rowpass_gemm_kernel<1>), grid, dim3(NT), 0, stream, g, tiles_n, ntiles);
    } else {
      hipLaunchKernelGGL(rowpass_fwd_staged_kernel, grid, dim3(NT), 0, stream, g, tiles_n, ntiles);
    }
  } else {
    hipLaunchKernelGGL((rowpass_gemm_kernel<2>), grid, dim3(NT), 0, stream, g, tiles_n, ntiles);
  }
}

int launch_gemm_rowpass_or_general(const GemmArgs& g, hipStream_t stream) {
  const bool eligible = gemm_rowpass_eligible(g);
  if ((g.fs_sq || g.fs_k) && !eligible)
    throw HipError{hipErrorInvalidValue, "fs_sq / fs_k are features of the specialised forward kernel only", __FILE__, __LINE__};
  if (eligible) {
    launch_gemm_rowpass(g, stream);
    return NWN;
  }
  if (g.role == 1 && (g.alpha != 1.0 || g.beta != 0.0)) {   // the general kernel's role-1 epilogue stores op(A) op(B) as it is
    GemmArgs h = g;
    h.role = 0;
    launch_gemm_f64(h, stream);
    return 2;
  }
  launch_gemm_f64(g, stream);
  return 2;
}
