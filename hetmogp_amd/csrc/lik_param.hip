// lik_param.hip -- the parameter group "likelihood parameters" (DESIGN 9e): Gaussian sigma, Student nu, Ordinal cut points + sigma.
//   * hmogp_var_exp_dparam: per-row derivatives of the variational expectation (building block of the row-by-row tests);
//   * hmogp_set_lik_params: a task's parameters become mutable; an Ordinal task keeps a PRIVATE table (the process-wide registry of
//     hmogp_ordinal_table is append-only and holds HMOGP_ORDINAL_MAXTABLES entries: training takes thousands of updates) and its rows'
//     cut points are rebuilt from the resident labels on the device;
//   * hmogp_lik_grad_enable / hmogp_lik_grad_read: d ELBO / d theta = batch_scale[t] sum_rows d ve / d theta of the last evaluation,
//     one row kernel per family behind the pool's quadrature, block partials in a slab, summed in a fixed order (no floating-point
//     atomics: two evaluations give the same bits).
// Declarations: engine_impl.h.
#include "engine_impl.h"
#include "lik_device.h"
#include "lik_dispatch.h"

namespace {

// ---- per-row building block ---------------------------------------------------------------------------------------------------
// out [N][C]: Gaussian C = 1 (d sigma), Student C = 1 (d nu), Ordinal C = 3 (d lo, d hi, d sigma; y is [2][N]: lower, upper cut points)
template <int LIK>
__global__ __launch_bounds__(256) void var_exp_dparam_kernel(double param, long long N, const double* __restrict__ y,
                                                             const double* __restrict__ m, const double* __restrict__ v,
                                                             double* __restrict__ out) {
  constexpr int G = lik_lanes(LIK);
  __shared__ double etab[4][60];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long n = ((long long)blockIdx.x * 256 + t) / G;
  if (n >= N) return;                                  // (uniform per wave when G == 64)
  if constexpr (LIK == HMOGP_LIK_GAUSSIAN) {
    out[n] = lik_gaussian_dsigma(y[n], m[n], v[n], param);
  } else if constexpr (LIK == HMOGP_LIK_STUDENT) {
    const double mu[2] = {m[2 * n], m[2 * n + 1]}, vv[2] = {v[2 * n], v[2 * n + 1]};
    const double d = lik_student_dnu_wave(y[n], mu, vv, param, lane, etab[w]);
    if (lane == 0) out[n] = d;
  } else {
    double dlo, dhi, dsig;
    lik_ordinal_dparam(y[n], y[N + n], m[n], v[n], param, dlo, dhi, dsig);
    out[3 * n] = dlo, out[3 * n + 1] = dhi, out[3 * n + 2] = dsig;
  }
}

// ---- Ordinal: the rows' own cut points from the resident labels, one lane per row, the table by value ----------------------------
__global__ __launch_bounds__(256) void ordinal_cuts_kernel(OrdinalTable tb, long long N, const double* __restrict__ label,
                                                           double* __restrict__ lo, double* __restrict__ hi) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int k = (int)label[n];                         // 1 .. K (checked when the data were set)
  lo[n] = (k >= 2 && k <= tb.K) ? tb.edge[k - 2] : -INFINITY;
  hi[n] = (k >= 1 && k <= tb.K - 1) ? tb.edge[k - 1] : INFINITY;
}

// ---- the gradient kernel of one segment ---------------------------------------------------------------------------------------
// q(f) of a row exactly as quad_body forms it (m += w p; v += (w^2 + kappa) var + w^2 c) from the pool's row statistics and the
// device-resident mixing weights, then the row's derivative; block partials [blocks][nout].
// nout: Gaussian 1, Student 1, Ordinal K (cut 1 .. K - 1, then sigma).  A row with label k adds d/d hi to cut k, d/d lo to cut k - 1.
template <int LIK>
__global__ __launch_bounds__(256) void lik_grad_kernel(LikGradArgs a) {
  constexpr int G = lik_lanes(LIK);
  constexpr int J = (LIK == HMOGP_LIK_STUDENT) ? 2 : 1;
  __shared__ double etab[4][60];
  __shared__ double red[4][HMOGP_ORDINAL_MAXK];
  __shared__ double s_w[HMOGP_MAXQ][J], s_kap[HMOGP_MAXQ][J], s_var[HMOGP_MAXQ];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long n = ((long long)blockIdx.x * 256 + t) / G;
  const bool valid = n < a.N;                          // uniform per wave when G == 64
  const long long nn = n + a.off;
  const int Q = a.Q;
  double pq[HMOGP_MAXQ], cq[HMOGP_MAXQ];
#pragma unroll
  for (int q = 0; q < HMOGP_MAXQ; ++q) {
    pq[q] = (valid && q < Q) ? a.p[q * a.ldn + nn] : 0.0;
    cq[q] = (valid && q < Q) ? a.c[q * a.ldn + nn] : 0.0;
  }
  if (t < HMOGP_MAXQ * J) {
    const int q = t / J, j = t % J;
    const bool in = q < Q;
    const long long o = (long long)q * a.Df + a.d0 + j;
    s_w[q][j] = in ? a.Wd[o] : 0.0, s_kap[q][j] = in ? a.kapd[o] : 0.0;
    if (j == 0) s_var[q] = in ? a.vard[q] : 0.0;
  }
  __syncthreads();
  double mu[J], vv[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    double m = 0.0, v = 0.0;
#pragma unroll
    for (int q = 0; q < HMOGP_MAXQ; ++q)
      if (q < Q) {
        const double wq = s_w[q][j];
        m += wq * pq[q];
        v += (wq * wq + s_kap[q][j]) * s_var[q] + wq * wq * cq[q];
      }
    mu[j] = m, vv[j] = v;
  }
  const int nout = a.nout;
  if constexpr (LIK == HMOGP_LIK_GAUSSIAN) {
    const double d = valid ? lik_gaussian_dsigma(a.y[n], mu[0], vv[0], a.lik_param) : 0.0;
    const double s = wave_sum(d);
    if (lane == 0) red[w][0] = s;
  } else if constexpr (LIK == HMOGP_LIK_STUDENT) {
    double d = 0.0;
    if (valid) d = lik_student_dnu_wave(a.y[n], mu, vv, a.lik_param, lane, etab[w]);   // (valid in every lane)
    if (lane == 0) red[w][0] = d;
  } else {
    double dlo = 0.0, dhi = 0.0, dsig = 0.0;
    int k = 0;
    if (valid) {
      lik_ordinal_dparam(a.y[n], a.yaux[n], mu[0], vv[0], a.lik_param, dlo, dhi, dsig);
      k = (int)a.label[n];
    }
    for (int c = 0; c < nout - 1; ++c) {               // cut c + 1: upper cut of label c + 1, lower cut of label c + 2
      const double s = wave_sum((k == c + 1 ? dhi : 0.0) + (k == c + 2 ? dlo : 0.0));
      if (lane == 0) red[w][c] = s;
    }
    const double s = wave_sum(dsig);
    if (lane == 0) red[w][nout - 1] = s;
  }
  __syncthreads();
  if (t < nout) a.partials[(long long)blockIdx.x * nout + t] = red[0][t] + red[1][t] + red[2][t] + red[3][t];
}

// block partials -> dst[slot] += scale * sum over the blocks, in a fixed order (one block per slot)
__global__ __launch_bounds__(256) void lik_grad_reduce_kernel(const double* __restrict__ part, long long nblocks, int nout,
                                                              double* __restrict__ dst, double scale,
                                                              const double* __restrict__ scaled) {
  __shared__ double scratch[16];
  const int k = blockIdx.x;
  double s = 0.0;
  for (long long b = threadIdx.x; b < nblocks; b += blockDim.x) s += part[b * nout + k];
  s = block_sum(s, scratch);
  if (threadIdx.x == 0) dst[k] += (scaled ? scaled[0] : scale) * s;
}

}  // namespace

namespace hmogp_detail {

// the three families with parameters of their own (lik_dparam_cols != 0), as a compile-time fact for the two launchers below
constexpr bool has_own_params(int lik) { return lik == HMOGP_LIK_GAUSSIAN || lik == HMOGP_LIK_STUDENT || lik == HMOGP_LIK_ORDINAL; }

void launch_var_exp_dparam(int lik, double param, long long N, const double* y, const double* m, const double* v, double* out,
                           hipStream_t s) {
  if (N <= 0) return;
  if (!has_own_params(lik)) throw EngineError{HMOGP_E_INVALID, "this likelihood has no parameters of its own"};
  const dim3 grid((unsigned)((N * lik_lanes(lik) + 255) / 256));
  visit_family(lik, 0, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK;
    if constexpr (has_own_params(L)) {
      if constexpr (L == HMOGP_LIK_ORDINAL) param = ordinal_table(param).sigma;
      hipLaunchKernelGGL((var_exp_dparam_kernel<L>), grid, dim3(256), 0, s, param, N, y, m, v, out);
    } else {
      throw EngineError{HMOGP_E_INVALID, "this likelihood has no parameters of its own"};
    }
  });
}

long long lik_grad_blocks(int lik, long long n) { return (n * lik_lanes(lik) + 255) / 256; }

void launch_lik_grad(const LikGradArgs& a, double* dst, double scale, const double* scaled, hipStream_t s) {
  if (a.N <= 0 || !has_own_params(a.lik)) return;   // (a family without parameters adds nothing)
  const long long nb = lik_grad_blocks(a.lik, a.N);
  const dim3 grid((unsigned)nb);
  visit_family(a.lik, 0, [&](auto fam) {
    constexpr int L = decltype(fam)::LIK;
    if constexpr (has_own_params(L)) hipLaunchKernelGGL((lik_grad_kernel<L>), grid, dim3(256), 0, s, a);
    else throw HipError{hipErrorInvalidValue, "lik_grad: this likelihood has no parameters of its own", __FILE__, __LINE__};
  });
  hipLaunchKernelGGL(lik_grad_reduce_kernel, dim3(a.nout), dim3(256), 0, s, a.partials, nb, a.nout, dst, scale, scaled);
}

}  // namespace hmogp_detail

// =================================================================================================== engine
int hmogp_engine::lik_param_count(int t) const {
  if (t < 0 || t >= T) throw EngineError{HMOGP_E_INVALID, "task index out of range"};
  const Task& k = tasks[t];
  if (k.lik == HMOGP_LIK_GAUSSIAN || k.lik == HMOGP_LIK_STUDENT) return 1;
  if (k.lik == HMOGP_LIK_ORDINAL) return task_table(k).K;
  return 0;
}

void hmogp_engine::set_lik_params(int t, const double* values, int n) {
  const int want = lik_param_count(t);
  if (want == 0) throw EngineError{HMOGP_E_INVALID, "this task's likelihood has no parameters of its own"};
  if (!values || n != want) throw EngineError{HMOGP_E_INVALID, "hmogp_set_lik_params: n does not match hmogp_lik_param_count"};
  Task& k = tasks[t];
  // validated like the constructors, before anything of the task changes
  if (k.lik == HMOGP_LIK_GAUSSIAN || k.lik == HMOGP_LIK_STUDENT) {
    if (!(std::isfinite(values[0]) && values[0] > 0.0))
      throw EngineError{HMOGP_E_INVALID, k.lik == HMOGP_LIK_GAUSSIAN ? "Gaussian: sigma must be finite and > 0" : "Student: deg_free must be finite and > 0"};
    HIP_TRY(hipSetDevice(device));
    k.param = k.qparam = values[0];
  } else {
    OrdinalTable tb;
    tb.K = want, tb.sigma = values[want - 1];
    if (!(std::isfinite(tb.sigma) && tb.sigma > 0.0)) throw EngineError{HMOGP_E_INVALID, "Ordinal: sigma must be finite and > 0"};
    for (int i = 0; i < want - 1; ++i) {
      if (!std::isfinite(values[i]) || (i > 0 && !(values[i] > values[i - 1])))
        throw EngineError{HMOGP_E_INVALID, "Ordinal: the cut points must be finite and strictly increasing"};
      tb.edge[i] = values[i];
    }
    for (int i = want - 1; i < HMOGP_ORDINAL_MAXK - 1; ++i) tb.edge[i] = 0.0;
    HIP_TRY(hipSetDevice(device));
    if (k.N > 0) {   // (stream-ordered in front of the next evaluation; no host pass over the rows, nothing uploaded)
      hipLaunchKernelGGL(ordinal_cuts_kernel, dim3((unsigned)((k.N + 255) / 256)), dim3(256), 0, st, tb, k.N, k.Y.d(), k.Ylo.d(), k.Yaux.d());
      HIP_TRY(hipGetLastError());   // a launch that did not happen leaves the rows' cuts AND the table below as they were
    }
    k.table = tb, k.own_table = true;
    k.qparam = tb.sigma;
  }
  began = false;
  drop_graphs();     // (captured small-model graphs hold the old value as a kernel argument)
}

void hmogp_engine::ensure_lik_grad_workspace() {
  if (!lik_grad_on) return;
  const long long rows = std::max<long long>(ws_rows, 1);
  // Student: one partial per 4 rows; Ordinal: K <= 32 partials per 256 rows; Gaussian: one per 256 rows
  likpart.ensure(sizeof(double) * ((rows + 3) / 4 + (rows + 255) / 256 * HMOGP_ORDINAL_MAXK + 2 * HMOGP_ORDINAL_MAXK));
  dlikgrad.ensure(sizeof(double) * (size_t)T * HMOGP_ORDINAL_MAXK, true);
}

void hmogp_engine::lik_grad_enable(bool on) {
  if (on == lik_grad_on) return;
  HIP_TRY(hipSetDevice(device));
  lik_grad_on = on;
  lik_grad_valid = false;
  began = false;
  drop_graphs();
  ensure_lik_grad_workspace();
}

void hmogp_engine::lik_grad_pool(const std::vector<Seg>& pl) {
  for (auto& sg : pl) {
    Task& k = tasks[sg.t];
    if (k.lik != HMOGP_LIK_GAUSSIAN && k.lik != HMOGP_LIK_STUDENT && k.lik != HMOGP_LIK_ORDINAL) continue;
    LikGradArgs a;
    a.lik = k.lik, a.lik_param = k.qparam, a.Q = Q, a.Df = Df, a.d0 = k.d0, a.N = sg.n, a.off = sg.off, a.ldn = ws_rows;
    a.nout = k.lik == HMOGP_LIK_ORDINAL ? task_table(k).K : 1;
    a.y = k.quad_y() + sg.r0;
    a.yaux = k.Yaux.p ? k.Yaux.d() + sg.r0 : nullptr;
    a.label = k.Y.d() + sg.r0;
    a.p = vp.d(), a.c = vc.d();
    a.Wd = dW.d(), a.kapd = dkap.d(), a.vard = dvar.d();
    a.partials = likpart.d();
    Scope sc(this, CAT_QUAD, 2);
    // (small path: the batch scale is read from the parameter block, so that a captured graph replays with a new one)
    launch_lik_grad(a, dlikgrad.d() + (size_t)sg.t * HMOGP_ORDINAL_MAXK, h_bs[sg.t], small_path ? dsmall.d() + oBs + sg.t : nullptr, st);
  }
}

void hmogp_engine::lik_grad_read(int t, double* g, int n) {
  const int want = lik_param_count(t);
  if (!g || n != want || want == 0) throw EngineError{HMOGP_E_INVALID, "hmogp_lik_grad_read: n does not match hmogp_lik_param_count"};
  std::fill(g, g + n, 0.0);
  if (!lik_grad_on || !lik_grad_valid || !(group_mask & HMOGP_GROUP_HYPER)) return;   // a gated group reads as zeros
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(g, dlikgrad.d() + (size_t)t * HMOGP_ORDINAL_MAXK, sizeof(double) * n, hipMemcpyDeviceToHost));
}
