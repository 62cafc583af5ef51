// quad.hip -- the quadrature of the row pass (gfx950):
//   quad            q(f) mean/variance (svmogp_inf.py:212-218) -> variational expectations (het_likelihood.py:
//                   101-131) -> row weights alpha/beta for the backward pass + scalar statistics
// one launch per segment (quad_kernel) or one per pool (quad_multi_kernel), and the reduction of a pool's block partials.
// Declarations: rowpass.h.
#include <algorithm>

#include "rowpass.h"
#include "lik_device.h"
#include "lik_dispatch.h"

namespace {

// ---- quad -----------------------------------------------------------------------------------------------
// LDS of one quadrature block
struct QuadShared {
  double etab[4][HMOGP_ETAB];
  double red[4][HMOGP_MAXSCAL];
  // mixing weights of this task's functions: from the kernel arguments, or (captured-graph replays) from device memory
  double w[HMOGP_MAXQ][HMOGP_MAXJ], w0[HMOGP_MAXQ][HMOGP_MAXJ], kap[HMOGP_MAXQ][HMOGP_MAXJ], var[HMOGP_MAXQ];
  double scale;
};

// The quadrature of one block of rows (block `blk` of the segment `a` describes).  DEVONLY: the by-value weights of `a` do not
// exist (quad_multi_kernel).
template <int LIK, int CATD, bool DEVONLY>
__device__ __forceinline__ void quad_body(const QuadArgs& a, unsigned blk, QuadShared& sh) {
  constexpr int G = lik_lanes(LIK);
  auto& etab = sh.etab;
  auto& red = sh.red;
  auto& s_w = sh.w;
  auto& s_w0 = sh.w0;
  auto& s_kap = sh.kap;
  auto& s_var = sh.var;
  double& s_scale = sh.scale;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long n = ((long long)blk * 256 + t) / G;
  const bool valid = n < a.N;                       // uniform per wave when G == 64
  // (row of the pool-wide [Q][ldn] vectors: `a.off` is the segment's offset in the pool when the pointers are NOT pre-offset --
  //  quad_multi_kernel: eight derived pointers per segment would be 16 more live SGPRs, and the instantiations that carry four or
  //  five likelihood bodies spilled SGPRs to scratch memory, 68 bytes per lane)
  const long long nn = n + a.off;
  const bool lead = valid && (G == 1 || lane == 0);  // the lane that owns the row's outputs
  const int Q = a.Q, J = a.dimf;
  const int nscal = 2 + 2 * Q + J + Q * J;
  // the row's inputs are requested BEFORE the weights are staged: one memory round trip for both (small models: the kernel is
  // a chain of latencies)
  double mu[HMOGP_MAXJ], vv[HMOGP_MAXJ], pq[HMOGP_MAXQ], cq[HMOGP_MAXQ];
#pragma unroll
  for (int q = 0; q < HMOGP_MAXQ; ++q) {
    pq[q] = (valid && q < Q) ? a.p[q * a.ldn + nn] : 0.0;
    cq[q] = (valid && q < Q) ? a.c[q * a.ldn + nn] : 0.0;
  }
  // (Weibull: the row's second value, delta, is row 1 of the task's [2][ldy] image and travels where yaux does)
  const double yv = valid ? a.y[n] : 0.0,
               yauxv = (LIK == HMOGP_LIK_WEIBULL) ? (valid ? a.y[a.ldy + n] : 0.0) : ((valid && a.yaux) ? a.yaux[n] : 0.0);
  // (Binomial, Beta-Binomial: y is row 0 of the task's [2][ldy] image (k, n); the row's own n takes the place of lik_param, yaux is lc)
  double ntr = 1.0;
  if constexpr (lik_has_trials(LIK)) ntr = valid ? a.y[a.ldy + n] : 1.0;
  double lyv[LIK == HMOGP_LIK_DIRICHLET ? CATD : 1];   // Dirichlet: log y_k of the row, k = 0 .. K - 1 (CATD = K)
  if constexpr (LIK == HMOGP_LIK_DIRICHLET) {
#pragma unroll
    for (int k = 0; k < CATD; ++k) lyv[k] = valid ? a.y[k * a.ldy + n] : 0.0;
  }
  if (t < HMOGP_MAXQ * HMOGP_MAXJ) {
    const int q = t / HMOGP_MAXJ, j = t % HMOGP_MAXJ;
    const bool in = q < a.Q && j < a.dimf;
    if (DEVONLY || a.Wd) {
      const long long o = (long long)q * a.Df + a.d0 + j;
      s_w[q][j] = in ? a.Wd[o] : 0.0, s_w0[q][j] = in ? a.W0d[o] : 0.0, s_kap[q][j] = in ? a.kapd[o] : 0.0;
      if (j == 0) s_var[q] = q < a.Q ? a.vard[q] : 0.0;
      if (t == 0) s_scale = a.scaled[0];
    } else if (!DEVONLY) {
      s_w[q][j] = a.w[q][j], s_w0[q][j] = a.w0[q][j], s_kap[q][j] = a.kap[q][j];
      if (j == 0) s_var[q] = a.var[q];
      if (t == 0) s_scale = a.scale;
    }
  }
  __syncthreads();
  // contribution of this lane to block scalar `slot` (uniform slot; every lane of the wave calls)
  auto emit = [&](int slot, double val) {
    const double s = (G == 1) ? wave_sum(val) : val;
    if (lane == 0) red[w][slot] = s;
  };
  bool neg = false;
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) {
    double m = 0.0, v = 0.0;
    if (j < J) {
#pragma unroll
      for (int q = 0; q < HMOGP_MAXQ; ++q)
        if (q < Q) {
          const double wq = s_w[q][j];
          m += wq * pq[q];
          v += (wq * wq + s_kap[q][j]) * s_var[q] + wq * wq * cq[q];
        }
      neg |= (v < 0.0);
    }
    mu[j] = m;
    vv[j] = v;
  }
  LikOut o;
  o.ve = 0.0;
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) o.gm[j] = o.gv[j] = 0.0;
  if constexpr (LIK == HMOGP_LIK_DIRICHLET) {
    if (valid) lik_dirichlet_wave<CATD>(lyv, mu, vv, lane, etab[w], o);
  } else if constexpr (lik_has_trials(LIK)) {
    if (valid) lik_eval<LIK, CATD>(yv, yauxv, mu, vv, ntr, lane, etab[w], a.quirks, o);
  } else {
    if (valid) lik_eval<LIK, CATD>(yv, yauxv, mu, vv, a.lik_param, lane, etab[w], a.quirks, o);
  }
  if (G == 64 || a.pg) {  // wave-per-row likelihoods: p / c were only needed for q(f); re-read them instead of keeping 2 x MAXQ
                          // doubles alive across the node loop (register pressure = occupancy of the quadrature).
                          // Strict q(f) (a.pg != nullptr): the block scalars sa / swk take the explicit-inverse forms K^ a and
                          // rowsum(P~ .* K^) the reference's gradient code uses (svmogp_inf.py:157-161), q(f) took the solve-based ones
    const double* pp = a.pg ? a.pg : a.p;
    const double* cc = a.pg ? a.cg : a.c;
#pragma unroll
    for (int q = 0; q < HMOGP_MAXQ; ++q) {
      pq[q] = (valid && q < Q) ? pp[q * a.ldn + nn] : 0.0;
      cq[q] = (valid && q < Q) ? cc[q * a.ldn + nn] : 0.0;
    }
  }
  // (the loops over a row's functions are unrolled to HMOGP_MAXJ with a guard: a run-time trip count indexes mu / vv / the LikOut
  //  arrays dynamically and parks them in scratch -- 144 bytes per lane in EVERY quad_kernel / var_exp_kernel instantiation, r5)
  if (a.out_mu && lead) {
#pragma unroll
    for (int j = 0; j < HMOGP_MAXJ; ++j)
      if (j < J) {
        a.out_mu[n * J + j] = mu[j];
        a.out_v[n * J + j] = vv[j];
      }
  }
  const double s = lead ? s_scale : 0.0;  // non-owning lanes contribute zeros
  o.ve *= s;
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j) {
    o.gm[j] *= s;
    o.gv[j] *= s;
  }
  if (a.out_gm && lead) {
#pragma unroll
    for (int j = 0; j < HMOGP_MAXJ; ++j)
      if (j < J) {
        a.out_gm[n * J + j] = o.gm[j];
        a.out_gv[n * J + j] = o.gv[j];
      }
  }
  emit(0, o.ve);
  emit(1, (lead && neg) ? 1.0 : 0.0);
#pragma unroll
  for (int q = 0; q < HMOGP_MAXQ; ++q) {
    if (q < Q) {
      double al = 0.0, be = 0.0, al0 = 0.0, be0 = 0.0;
#pragma unroll
      for (int j = 0; j < HMOGP_MAXJ; ++j)
        if (j < J) {
          const double wq = s_w[q][j], w0 = s_w0[q][j];
          al += wq * o.gm[j];
          be += wq * wq * o.gv[j];
          al0 += w0 * o.gm[j];
          be0 += w0 * wq * o.gv[j];
          emit(2 + 2 * Q + J + q * J + j, o.gm[j] * pq[q] + 2.0 * wq * (o.gv[j] * cq[q]));  // swk[q][j]
        }
      if (lead) {
        a.alpha[q * a.ldn + nn] = al;
        a.beta[q * a.ldn + nn] = be;
        a.alpha0[q * a.ldn + nn] = al0;
        a.beta0[q * a.ldn + nn] = be0;
      }
      const double ptq = (lead && a.pt) ? a.pt[q * a.ldn + nn] : 0.0;
      const double ctq = (lead && a.ct) ? a.ct[q * a.ldn + nn] : 0.0;
      emit(2 + 2 * q, al0 * pq[q] + 2.0 * be0 * cq[q]);  // sa_q
      emit(3 + 2 * q, al0 * ptq + 2.0 * be0 * ctq);      // sl_q
    }
  }
#pragma unroll
  for (int j = 0; j < HMOGP_MAXJ; ++j)
    if (j < J) emit(2 + 2 * Q + j, o.gv[j]);  // sgv[j]
  __syncthreads();
  if (t < nscal) a.partials[(long long)blk * nscal + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

template <int LIK, int CATD = 0>
__global__ __launch_bounds__(256) void quad_kernel(QuadArgs a) {
  __shared__ QuadShared sh;
  quad_body<LIK, CATD, false>(a, blockIdx.x, sh);
}

// All segments of a pool in ONE launch (small models: three likelihood families of ~1000 rows each are three launches of a few
// blocks otherwise); block -> segment by the prefix of block counts, likelihood by a block-uniform branch.
// [r5] MASK = the likelihood families this instantiation carries (bit L for family L, bit 8 + d for Categorical with d latent
// functions).  One kernel with all fifteen bodies inlined is allocated for the worst of them (256 VGPRs + 32 AGPRs, 380 spilled
// SGPRs, one wave per SIMD); the sets of the BASELINE configurations get instantiations of their own (C1's
// {HetGaussian, Bernoulli, Categorical(3)}: see the register table in DESIGN 11e), any other set the all-inclusive one.
// Student (id 8) takes bit 17, above Categorical's 8 + d (d <= 8), and Ordinal (id 9) bit 18, so that no bit of an existing family moves.
// Dirichlet (id 10) takes bit 19 + (K - 2), K = 2 .. 4: one bit per K, like Categorical, so that each K is an instantiation of its own.
// Negative Binomial (id 11) takes bit 22 (bit 11 is Categorical with three functions), Weibull (id 12) bit 23 (bit 12 is Categorical
// with four), Binomial (id 13) bit 24, Beta-Binomial (id 14) bit 25 and the zero-inflated Poisson (id 15) bit 26 (bit 15 is Categorical
// with seven); the mask is an unsigned of 32 bits, so bits 27 .. 31 remain.
static_assert(sizeof(unsigned) * 8 >= 32, "quad_multi mask");
constexpr unsigned qm_bit(int lik, int dimf) {
  return lik == HMOGP_LIK_CATEGORICAL ? 1u << (8 + dimf)
         : lik == HMOGP_LIK_DIRICHLET ? 1u << (17 + dimf)
         : lik == HMOGP_LIK_NEGBINOMIAL ? 1u << 22
         : lik == HMOGP_LIK_WEIBULL ? 1u << 23
         : lik == HMOGP_LIK_BINOMIAL ? 1u << 24
         : lik == HMOGP_LIK_BETABINOMIAL ? 1u << 25
         : lik == HMOGP_LIK_ZIPOISSON ? 1u << 26
                                      : (lik == HMOGP_LIK_STUDENT ? 1u << 17 : (lik == HMOGP_LIK_ORDINAL ? 1u << 18 : 1u << lik));
}
constexpr unsigned QM_C1 = qm_bit(HMOGP_LIK_HETGAUSSIAN, 0) | qm_bit(HMOGP_LIK_BERNOULLI, 0) | qm_bit(HMOGP_LIK_CATEGORICAL, 2);
constexpr unsigned QM_H4 = qm_bit(HMOGP_LIK_GAUSSIAN, 0) | qm_bit(HMOGP_LIK_BERNOULLI, 0) | qm_bit(HMOGP_LIK_POISSON, 0) |
                           qm_bit(HMOGP_LIK_GAMMA, 0);
constexpr unsigned QM_C5 = qm_bit(HMOGP_LIK_GAUSSIAN, 0) | qm_bit(HMOGP_LIK_CATEGORICAL, 3);
constexpr unsigned QM_LIGHT = qm_bit(HMOGP_LIK_GAUSSIAN, 0) | qm_bit(HMOGP_LIK_BERNOULLI, 0) | qm_bit(HMOGP_LIK_HETGAUSSIAN, 0) |
                              qm_bit(HMOGP_LIK_POISSON, 0) | qm_bit(HMOGP_LIK_EXPONENTIAL, 0);

template <unsigned MASK>
__global__ __launch_bounds__(256) void quad_multi_kernel(QuadMulti m) {
  __shared__ QuadShared sh;
  int s = 0;
  while (s + 1 < m.nseg && blockIdx.x >= m.seg[s + 1].blk0) ++s;
  const QuadSeg& g = m.seg[s];
  QuadArgs a;
  a.lik = g.lik, a.lik_param = g.lik_param, a.dimf = g.dimf, a.Q = m.Q, a.N = g.N;
  a.y = g.y, a.yaux = g.yaux, a.ldy = g.ldy;
  a.p = m.p, a.c = m.c, a.pt = m.pt, a.ct = m.ct, a.off = g.off;
  a.ldn = m.ldn;
  a.Wd = m.Wd, a.W0d = m.W0d, a.kapd = m.kapd, a.vard = m.vard, a.scaled = m.scale_base + g.t;
  a.Df = m.Df, a.d0 = g.d0;
  a.pg = a.cg = nullptr;
  a.quirks = m.quirks;
  a.alpha = m.alpha, a.beta = m.beta, a.alpha0 = m.alpha0, a.beta0 = m.beta0;
  a.partials = m.partials + g.part0;
  a.out_mu = a.out_v = a.out_gm = a.out_gv = nullptr;
  const unsigned blk = blockIdx.x - g.blk0;
#define QB(L)                                                  \
  if constexpr ((MASK & qm_bit(L, 0)) != 0) {                  \
    if (g.lik == L) {                                          \
      quad_body<L, 0, true>(a, blk, sh);                       \
      return;                                                  \
    }                                                          \
  }
#define QBC(D)                                                 \
  if constexpr ((MASK & qm_bit(HMOGP_LIK_CATEGORICAL, D)) != 0) { \
    if (g.lik == HMOGP_LIK_CATEGORICAL && g.dimf == D) {       \
      quad_body<HMOGP_LIK_CATEGORICAL, D, true>(a, blk, sh);   \
      return;                                                  \
    }                                                          \
  }
  QB(HMOGP_LIK_GAUSSIAN) QB(HMOGP_LIK_BERNOULLI) QB(HMOGP_LIK_HETGAUSSIAN) QB(HMOGP_LIK_POISSON) QB(HMOGP_LIK_EXPONENTIAL)
  QB(HMOGP_LIK_GAMMA) QB(HMOGP_LIK_BETA) QB(HMOGP_LIK_STUDENT) QB(HMOGP_LIK_ORDINAL) QB(HMOGP_LIK_NEGBINOMIAL)
  QB(HMOGP_LIK_WEIBULL) QB(HMOGP_LIK_BINOMIAL) QB(HMOGP_LIK_BETABINOMIAL) QB(HMOGP_LIK_ZIPOISSON)
  QBC(1) QBC(2) QBC(3) QBC(4) QBC(5) QBC(6) QBC(7) QBC(8)
#define QBD(K)                                                 \
  if constexpr ((MASK & qm_bit(HMOGP_LIK_DIRICHLET, K)) != 0) { \
    if (g.lik == HMOGP_LIK_DIRICHLET && g.dimf == K) {         \
      quad_body<HMOGP_LIK_DIRICHLET, K, true>(a, blk, sh);     \
      return;                                                  \
    }                                                          \
  }
  QBD(2) QBD(3) QBD(4)
#undef QBD
#undef QB
#undef QBC
}

}  // namespace

long long quad_blocks(int lik, long long N) { return (N * lik_lanes(lik) + 255) / 256; }

void launch_quad(const QuadArgs& a, hipStream_t s) {
  if (a.N <= 0) return;
  dim3 grid((unsigned)quad_blocks(a.lik, a.N));
  visit_family(a.lik, a.dimf, [&](auto fam) {
    hipLaunchKernelGGL((quad_kernel<decltype(fam)::LIK, decltype(fam)::D>), grid, dim3(256), 0, s, a);
  });
}

bool quad_multi_specialised(const QuadMulti& m) {
  unsigned need = 0;
  for (int i = 0; i < m.nseg; ++i) need |= qm_bit(m.seg[i].lik, m.seg[i].dimf);
  for (unsigned mask : {QM_C1, QM_C5, QM_H4, QM_LIGHT})
    if ((need & ~mask) == 0) return true;
  return false;
}

void launch_quad_multi(const QuadMulti& m_in, hipStream_t s) {
  QuadMulti m = m_in;
  unsigned blocks = 0;
  long long part = 0;
  for (int i = 0; i < m.nseg; ++i) {
    QuadSeg& g = m.seg[i];
    if (g.lik == HMOGP_LIK_CATEGORICAL && (g.dimf < 1 || g.dimf > 8))
      throw HipError{hipErrorInvalidValue, "Categorical needs 2 <= K <= 9", __FILE__, __LINE__};
    if (g.lik == HMOGP_LIK_DIRICHLET && (g.dimf < 2 || g.dimf > HMOGP_DIRICHLET_MAXK))
      throw HipError{hipErrorInvalidValue, "Dirichlet needs 2 <= K <= HMOGP_DIRICHLET_MAXK", __FILE__, __LINE__};
    g.blk0 = blocks, g.part0 = part;
    const long long nb = quad_blocks(g.lik, g.N);
    blocks += (unsigned)nb;
    part += nb * (2 + 2 * m.Q + g.dimf + m.Q * g.dimf);
  }
  if (blocks == 0) return;
  unsigned need = 0;
  for (int i = 0; i < m.nseg; ++i) need |= qm_bit(m.seg[i].lik, m.seg[i].dimf);
#define QML(MASK)                                                                             \
  if ((need & ~(MASK)) == 0) {                                               \
    hipLaunchKernelGGL((quad_multi_kernel<MASK>), dim3(blocks), dim3(256), 0, s, m);          \
    return;                                                                                   \
  }
  QML(QM_C1) QML(QM_C5) QML(QM_H4) QML(QM_LIGHT)
#undef QML
  // [r6] any other likelihood set (BASELINE config 4's eight families ...): one launch for the five cheap families together and one
  // per expensive family present, each over the SAME block range and segment table -- a block whose segment the instantiation does
  // not carry returns at once.  The all-inclusive instantiation this replaces is allocated for the worst body it inlines (256 VGPRs +
  // 38 AGPRs, 321 spilled SGPRs, 144 bytes of scratch, one wave per SIMD) and ran every cheap segment at that occupancy.
#define QMS(MASK)                                                                             \
  if ((need & (MASK)) != 0) hipLaunchKernelGGL((quad_multi_kernel<MASK>), dim3(blocks), dim3(256), 0, s, m);
  QMS(QM_LIGHT)
  QMS(qm_bit(HMOGP_LIK_GAMMA, 0)) QMS(qm_bit(HMOGP_LIK_BETA, 0)) QMS(qm_bit(HMOGP_LIK_STUDENT, 0))
  QMS(qm_bit(HMOGP_LIK_ORDINAL, 0)) QMS(qm_bit(HMOGP_LIK_NEGBINOMIAL, 0)) QMS(qm_bit(HMOGP_LIK_WEIBULL, 0))
  QMS(qm_bit(HMOGP_LIK_BINOMIAL, 0)) QMS(qm_bit(HMOGP_LIK_BETABINOMIAL, 0)) QMS(qm_bit(HMOGP_LIK_ZIPOISSON, 0))
  QMS(qm_bit(HMOGP_LIK_DIRICHLET, 2)) QMS(qm_bit(HMOGP_LIK_DIRICHLET, 3)) QMS(qm_bit(HMOGP_LIK_DIRICHLET, 4))
  QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 1)) QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 2)) QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 3))
  QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 4)) QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 5)) QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 6))
  QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 7)) QMS(qm_bit(HMOGP_LIK_CATEGORICAL, 8))
#undef QMS
}

namespace {
__global__ __launch_bounds__(256) void reduce_rows_multi_kernel(SmallQuadRed qr, double* __restrict__ dst) {
  __shared__ double scratch[16];
  const int k = blockIdx.x;
  for (int sg = 0; sg < qr.nseg; ++sg) {
    const auto& g = qr.s[sg];
    if (k >= g.nscal) continue;              // (block-uniform)
    double s = 0.0;
    for (long long b = threadIdx.x; b < g.nrows; b += blockDim.x) s += g.part[b * g.nscal + k];
    s = block_sum(s, scratch);
    if (threadIdx.x == 0) dst[g.off[k]] += s;
    __syncthreads();
  }
}
}  // namespace
void launch_reduce_rows_multi(const SmallQuadRed& qr, double* dst, hipStream_t s) {
  int len = 0;
  for (int i = 0; i < qr.nseg; ++i) len = std::max(len, qr.s[i].nscal);
  if (len <= 0) return;
  hipLaunchKernelGGL(reduce_rows_multi_kernel, dim3(len), dim3(256), 0, s, qr, dst);
}
