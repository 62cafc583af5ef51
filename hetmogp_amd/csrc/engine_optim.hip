// engine_optim.hip -- device-resident q(u): Adadelta, the natural-gradient step; predict_f; the raw-gradient debug export.
// Split out of engine.hip in round 6 (no behaviour change); declarations: engine_impl.h.
#include "engine_impl.h"

void hmogp_engine::qu_load(const double* m_u, const double* L_flat) {
  if (!m_u || !L_flat) throw EngineError{HMOGP_E_INVALID, "null q(u) arrays"};
  HIP_TRY(hipSetDevice(device));
  const size_t nm = sizeof(double) * M * Q, nl = sizeof(double) * ((long long)M * (M + 1) / 2) * Q;
  HIP_TRY(hipMemcpyAsync(dmu.p, m_u, nm, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dLflat.p, L_flat, nl, hipMemcpyHostToDevice, st));
  for (DevBuf* b : {&ad_gms_m, &ad_sms_m, &ad_step_m, &ad_pend_m}) {
    b->ensure(nm);
    HIP_TRY(hipMemsetAsync(b->p, 0, nm, st));
  }
  for (DevBuf* b : {&ad_gms_L, &ad_sms_L, &ad_step_L, &ad_pend_L}) {
    b->ensure(nl);
    HIP_TRY(hipMemsetAsync(b->p, 0, nl, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  qu_resident = true;
}

void hmogp_engine::qu_read(double* m_u, double* L_flat) {
  if (!qu_resident) throw EngineError{HMOGP_E_STATE, "no resident q(u)"};
  HIP_TRY(hipSetDevice(device));
  if (m_u) HIP_TRY(hipMemcpyAsync(m_u, dmu.p, sizeof(double) * M * Q, hipMemcpyDeviceToHost, st));
  if (L_flat) HIP_TRY(hipMemcpyAsync(L_flat, dLflat.p, sizeof(double) * ((long long)M * (M + 1) / 2) * Q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
}

void hmogp_engine::qu_adadelta(int phase, double rate, double m, double d, double omd, double o) {
  if (!qu_resident) throw EngineError{HMOGP_E_STATE, "no resident q(u)"};
  if (phase == 1 && !evaluated) throw EngineError{HMOGP_E_STATE, "Adadelta update without a finished evaluation"};
  if (phase == 1 && skip_g_L && !small_path && (group_mask & HMOGP_GROUP_QU) != 0)
    throw EngineError{HMOGP_E_STATE, "the last evaluation ran with HMOGP_EVAL_NO_G_L: it left no gradient of q(u)'s factor"};
  HIP_TRY(hipSetDevice(device));
  const long long nm = (long long)M * Q, nl = ((long long)M * (M + 1) / 2) * Q;
  const bool has = phase == 1 && (group_mask & HMOGP_GROUP_QU) != 0;
  launch_adadelta(dmu.d(), ad_gms_m.d(), ad_sms_m.d(), ad_step_m.d(), ad_pend_m.d(), has ? gmu.d() : nullptr, -1.0, nm, phase, rate, m, d, omd, o, st);
  launch_adadelta(dLflat.d(), ad_gms_L.d(), ad_sms_L.d(), ad_step_L.d(), ad_pend_L.d(), has ? gL.d() : nullptr, -1.0, nl, phase, rate, m, d, omd, o, st);
  // (no host synchronisation: every consumer of the resident q(u) is ordered behind this stream -- the next evaluation's q(u)
  //  chain on the third stream waits for ev_qu, hmogp_qu_read / hmogp_qu_natgrad run on this stream)
  HIP_TRY(hipEventRecord(ev_qu, st));
}

void hmogp_engine::debug_raw(double* o_kmm, double* o_kmn, double* o_kdiag) {
  if (!evaluated) throw EngineError{HMOGP_E_STATE, "no finished evaluation"};
  if ((group_mask & HMOGP_GROUP_ALL) != HMOGP_GROUP_ALL) throw EngineError{HMOGP_E_STATE, "debug export needs group_mask = HMOGP_GROUP_ALL"};
  if (pools.size() != 1) throw EngineError{HMOGP_E_STATE, "debug export needs all rows in one pool (small N)"};
  HIP_TRY(hipSetDevice(device));
  const long long MM = (long long)M * M, ldn = ws_rows;
  if (o_kmm) HIP_TRY(hipMemcpyAsync(o_kmm, dKmm.p, sizeof(double) * MM * Q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (!o_kmn && !o_kdiag) return;
  const auto& pl = pools[0];
  std::vector<long long> nt(T, 0), off(T, 0);
  for (auto& sg : pl) {
    if (nt[sg.t] == 0) off[sg.t] = sg.off;
    nt[sg.t] += sg.n;   // a task's segments are contiguous inside the pool
  }
  long long nmax = 1;
  for (int t = 0; t < T; ++t) nmax = std::max(nmax, nt[t]);
  DevBuf gm, gv, tile;
  std::vector<DevBuf> gmt(T), gvt(T);
  for (auto& sg : pl) {
    Task& k = tasks[sg.t];
    gmt[sg.t].ensure(sizeof(double) * nt[sg.t] * k.dimf), gvt[sg.t].ensure(sizeof(double) * nt[sg.t] * k.dimf);
    QuadArgs qa;
    qa.lik = k.lik, qa.lik_param = k.qparam, qa.dimf = k.dimf, qa.Q = Q, qa.N = sg.n;
    qa.y = k.quad_y() + sg.r0;
    qa.yaux = k.Yaux.p ? k.Yaux.d() + sg.r0 : nullptr;
    qa.ldy = k.quad_ldy();
    qa.p = vp.d() + sg.off, qa.c = vc.d() + sg.off, qa.pt = vpt.d() + sg.off, qa.ct = vct.d() + sg.off;
    qa.ldn = ldn;
    std::memset(qa.w, 0, sizeof(qa.w)), std::memset(qa.w0, 0, sizeof(qa.w0)), std::memset(qa.kap, 0, sizeof(qa.kap));
    std::memset(qa.var, 0, sizeof(qa.var));
    for (int q = 0; q < Q; ++q) {
      qa.var[q] = h_var[q];
      for (int j = 0; j < k.dimf; ++j) {
        qa.w[q][j] = h_W[q * Df + k.d0 + j];
        qa.w0[q][j] = h_W0[q * Df + k.d0 + j];
        qa.kap[q][j] = h_kap[q * Df + k.d0 + j];
      }
    }
    qa.scale = h_bs[sg.t];
    qa.quirks = quirks;
    if (strict) qa.pg = vpg.d() + sg.off, qa.cg = vcg.d() + sg.off;
    qa.alpha = valpha.d() + sg.off, qa.beta = vbeta.d() + sg.off;      // rewritten with identical values
    qa.alpha0 = valpha0.d() + sg.off, qa.beta0 = vbeta0.d() + sg.off;
    qa.partials = quadpart.d();
    const long long within = sg.off - off[sg.t];
    qa.out_gm = gmt[sg.t].d() + within * k.dimf, qa.out_gv = gvt[sg.t].d() + within * k.dimf;
    launch_quad(qa, st);
  }
  tile.ensure(sizeof(double) * nmax * M);
  std::vector<double> hgv;
  size_t o1 = 0, o2 = 0;
  for (int q = 0; q < Q; ++q)
    for (int d = 0; d < Df; ++d) {
      const int t = f_index[d], j = d_index[d], J = tasks[t].dimf;
      const long long n = nt[t];
      if (o_kmn && n > 0) {
        launch_raw_kmn(a.d() + (long long)q * M, gmt[t].d(), gvt[t].d(), J, j, h_W[q * Df + d],
                       Pt.d() + (long long)q * ldn * M + off[t] * M, M, n, tile.d(), st);
        HIP_TRY(hipMemcpyAsync(o_kmn + o1, tile.p, sizeof(double) * n * M, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
      }
      o1 += (size_t)n * M;
      if (o_kdiag && n > 0) {
        hgv.resize((size_t)n * J);
        HIP_TRY(hipMemcpy(hgv.data(), gvt[t].p, sizeof(double) * n * J, hipMemcpyDeviceToHost));
        for (long long i = 0; i < n; ++i) o_kdiag[o2 + i] = hgv[(size_t)i * J + j];
      }
      o2 += (size_t)n;
    }
}

void hmogp_engine::natgrad_core(double gamma, bool sync) {
  if (!evaluated || !have_qu_grads) throw EngineError{HMOGP_E_STATE, "natural-gradient step needs a finished evaluation with the q(u) group"};
  if (!(gamma > 0.0)) throw EngineError{HMOGP_E_INVALID, "bad natural-gradient arguments"};
  HIP_TRY(hipSetDevice(device));
  const long long Mtri = (long long)M * (M + 1) / 2;
  for (DevBuf* b : {&ng_t1, &ng_t2, &ng_th, &ng_mnew}) b->ensure(sizeof(double) * Q * M);
  ng_mq.ensure(sizeof(double) * M * Q), ng_lflat.ensure(sizeof(double) * Mtri * Q);
  if (!h_info2) HIP_TRY(hipHostMalloc((void**)&h_info2, sizeof(int) * 2 * HMOGP_MAXQ, hipHostMallocDefault));
  if (ng_pending) (void)qu_natgrad_status();                                       // (its info words sit where this step's will land)
  HIP_TRY(hipStreamWaitEvent(st, ev_join, 0));                                     // the q(u) tail of the evaluation (third stream)
  // Lambda = S^-1 - 2 gamma dL/dS is the new precision.  It is factorised REVERSED (rows and columns): J Lambda J = R R^T
  // gives Lambda = U U^T with U = J R J upper triangular, hence S_new = Lambda^-1 = U^-T U^-1 and L_new = U^-T = the
  // anti-transpose of R^-1 is the lower Cholesky factor of S_new (unique: positive diagonal) -- one factorisation and one
  // triangular inverse, no product R^-T R^-1 and no second factorisation.
  launch_natgrad_prec(Sqi.d(), dLdS.d(), gamma, G.d(), Q, M, true, st);
  launch_gemv_batched(Sqi.d(), dmu.d(), ng_t1.d(), Q, M, 1, Q, st);                // S^-1 m
  launch_gemv_batched(dLdS.d(), dmu.d(), ng_t2.d(), Q, M, 1, Q, st);               // dL/dS m
  launch_natgrad_theta1(ng_t1.d(), ng_t2.d(), gmu.d(), gamma, ng_th.d(), Q, M, st);
  launch_potrf_batched(G.d(), Q, M, dinfo.as<int>(), dscr.d(), st);                // J Lambda J = R R^T
  HIP_TRY(hipMemcpyAsync(h_info2, dinfo.p, sizeof(int) * Q, hipMemcpyDeviceToHost, st));
  // (speculative, like the K_uu chain of an evaluation: a failed factorisation makes the launches below no-ops on garbage
  //  that is never committed)
  launch_trtri_batched(G.d(), tmpA.d(), tmpB.d(), Q, M, st);                       // R^-1
  launch_antitranspose(tmpA.d(), GSK.d(), Q, M, st);                               // L_new[i][j] = R^-1[M-1-j][M-1-i]
  launch_gemv_t_batched(GSK.d(), ng_th.d(), ng_t1.d(), Q, M, st);                  // L^T theta1
  launch_gemv_batched(GSK.d(), ng_t1.d(), ng_mnew.d(), Q, M, M, 1, st);            // m_new = S_new theta1 = L (L^T theta1)
  launch_pack_tril(GSK.d(), ng_lflat.d(), Q, M, 1.0, st);
  launch_scatter_mq(ng_mnew.d(), ng_mq.d(), Q, M, st);
  if (!sync) return;               // hmogp_qu_natgrad_async: the commit is decided on the device, the host looks later
  HIP_TRY(hipStreamSynchronize(st));
  // (a failed step has only written scratch -- G, GSK, tmpA, tmpB -- none of which is an input of the step: the caller
  //  may retry with a smaller gamma straight away, no new evaluation needed)
  for (int q = 0; q < Q; ++q)
    if (h_info2[q] != 0) throw EngineError{HMOGP_E_NOT_PD, "natural-gradient step leaves the positive-definite cone (reduce gamma)"};
  evaluated = false;  // q(u) moves on: posterior / predict / another step need a fresh evaluation
}

void hmogp_engine::natgrad_step(double gamma, double* m_out, double* L_flat_out) {
  if (!m_out || !L_flat_out) throw EngineError{HMOGP_E_INVALID, "bad natural-gradient arguments"};
  natgrad_core(gamma);
  const long long Mtri = (long long)M * (M + 1) / 2;
  HIP_TRY(hipMemcpyAsync(m_out, ng_mq.p, sizeof(double) * M * Q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(L_flat_out, ng_lflat.p, sizeof(double) * Mtri * Q, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
}

void hmogp_engine::qu_natgrad(double gamma) {
  if (!qu_resident) throw EngineError{HMOGP_E_STATE, "no resident q(u) (hmogp_qu_load)"};
  natgrad_core(gamma);
  const long long Mtri = (long long)M * (M + 1) / 2;
  HIP_TRY(hipMemcpyAsync(dmu.p, ng_mq.p, sizeof(double) * M * Q, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(dLflat.p, ng_lflat.p, sizeof(double) * Mtri * Q, hipMemcpyDeviceToDevice, st));
  // (no synchronisation: the next evaluation reads q(u) on streams ordered behind this one -- see upload_params)
  HIP_TRY(hipEventRecord(ev_qu, st));
}

void hmogp_engine::qu_natgrad_async(double gamma) {
  if (!qu_resident) throw EngineError{HMOGP_E_STATE, "no resident q(u) (hmogp_qu_load)"};
  if (ng_pending) throw EngineError{HMOGP_E_STATE, "a natural-gradient step is pending (hmogp_qu_natgrad_status)"};
  natgrad_core(gamma, false);
  const long long Mtri = (long long)M * (M + 1) / 2;
  launch_commit_if_ok(dinfo.as<int>(), Q, ng_mq.d(), dmu.d(), (long long)M * Q, ng_lflat.d(), dLflat.d(), Mtri * Q, st);
  HIP_TRY(hipEventRecord(ev_qu, st));
  if (!ev_ng) HIP_TRY(hipEventCreateWithFlags(&ev_ng, hipEventDisableTiming));
  HIP_TRY(hipEventRecord(ev_ng, st));
  ng_pending = true;
  evaluated = false;               // q(u) (probably) moves on: posterior / predict / another step need a fresh evaluation
}

int hmogp_engine::qu_natgrad_status() {
  if (ng_pending) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(hipEventSynchronize(ev_ng));
    ng_pending = false;
    ng_last_taken = true;
    for (int q = 0; q < Q; ++q) ng_last_taken = ng_last_taken && h_info2[q] == 0;
  }
  return ng_last_taken ? 1 : 0;
}

void hmogp_engine::qf_chunk(const double* Xchunk, long long n, DevBuf& dX, DevBuf& dm, DevBuf& dv) {
  const long long MM = (long long)M * M;
  const int ldz = Q * P;
  const long long ldn = ws_rows;
  HIP_TRY(hipMemcpyAsync(dX.p, Xchunk, sizeof(double) * n * P, hipMemcpyHostToDevice, st));
  if (strict) {
    RbfBatch rbt;
    rbt.nq = Q, rbt.var = dvar.d(), rbt.ell = dell.d(), rbt.sZ = P, rbt.sK = ldn * M;
    launch_rbf(dX.d(), P, n, P, dZ.d(), ldz, M, 0.0, 1.0, Kh.d(), false, st, nullptr, true, &rbt);
    strict_forward(n, dX.d(), false, false);   // (in the form of the evaluation the prediction is taken from)
  }
  for (int q = 0; q < Q && !strict; ++q) {
    double* kh = Kh.d() + (long long)q * ldn * M;
    double* pt = Pt.d() + (long long)q * ldn * M;
    launch_rbf(dX.d(), P, n, P, dZ.d() + q * P, ldz, M, h_var[q], h_ell[q], kh, false, st, nullptr, false);
    GemmArgs g;
    g.A = kh, g.lda = M, g.a_kmajor = 0;
    g.B = Ctri.d() + q * MM, g.ldb = M, g.b_kmajor = 1, g.b_tri = 1;  // variances only: triangular fold of C
    g.C = pt, g.ldc = M;
    g.M = (int)n, g.N = M, g.K = M;
    g.role = 1;
    g.fs_part = fwdpart.d(), g.fs_a = a.d() + (long long)q * M, g.fs_x = dX.d(), g.fs_z = dZ.d() + q * P;
    g.fs_ldz = ldz, g.fs_P = P, g.fs_hyper = 0, g.fs_ell = dell.d() + q;
    g.store_c = 0;
    const int nparts = launch_gemm_rowpass_or_general(g, st);
    launch_combine_parts(fwdpart.d(), nparts * ((M + 127) / 128), n, vp.d() + q * ldn, vc.d() + q * ldn, nullptr, nullptr, st);
  }
  launch_qf_combine(vp.d(), vc.d(), ldn, n, Q, Df, dW.d(), dkap.d(), dvar.d(), dm.d(), dv.d(), st);
}

void hmogp_engine::predict_f(const double* Xnew, long long Nnew, double* m, double* v) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to predict from"};
  if (Nnew < 0 || (Nnew > 0 && (!Xnew || !m || !v))) throw EngineError{HMOGP_E_INVALID, "bad predict arguments"};
  HIP_TRY(hipSetDevice(device));
  ensure_workspace(std::min(chunk, std::max<long long>(Nnew, 1)));
  ensure_strict_workspace();           // (predictions follow the mode of the evaluation they are taken from)
  const long long ldn = ws_rows;
  DevBuf dX, dm, dv;
  dX.ensure(sizeof(double) * ldn * P), dm.ensure(sizeof(double) * ldn * Df), dv.ensure(sizeof(double) * ldn * Df);
  for (long long r0 = 0; r0 < Nnew; r0 += ldn) {
    const long long n = std::min(ldn, Nnew - r0);
    qf_chunk(Xnew + r0 * P, n, dX, dm, dv);
    HIP_TRY(hipMemcpyAsync(m + r0 * Df, dm.p, sizeof(double) * n * Df, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(v + r0 * Df, dv.p, sizeof(double) * n * Df, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
}

// the same chunks as predict_f; the task's columns of q(f) and |v| go straight into the rule's kernel, with the task's CURRENT
// likelihood parameters (whatever hmogp_set_lik_params last wrote).  Ynew has the layout hmogp_set_task_data takes, and gets its checks.
void hmogp_engine::predict_log_density(int t, const double* Xnew, const double* Ynew, long long Nnew, int T_, double* lpd, double* ess) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to predict from"};
  if (t < 0 || t >= T) throw EngineError{HMOGP_E_INVALID, "task index out of range"};
  if (Nnew < 0 || (Nnew > 0 && (!Xnew || !Ynew || !lpd))) throw EngineError{HMOGP_E_INVALID, "bad predict arguments"};
  if (Nnew == 0) return;
  const Task& k = tasks[t];
  HIP_TRY(hipSetDevice(device));
  DevBuf dy, dl, de;
  const OrdinalTable* tb = k.lik == HMOGP_LIK_ORDINAL ? &task_table(k) : nullptr;
  upload_y_image(k.lik, k.param, tb, Ynew, Nnew, dy);      // (checks the rows; throws before anything is launched)
  dl.ensure(sizeof(double) * Nnew);
  if (ess) de.ensure(sizeof(double) * Nnew);
  ensure_workspace(std::min(chunk, std::max<long long>(Nnew, 1)));
  ensure_strict_workspace();
  const long long ldn = ws_rows;
  DevBuf dX, dm, dv;
  dX.ensure(sizeof(double) * ldn * P), dm.ensure(sizeof(double) * ldn * Df), dv.ensure(sizeof(double) * ldn * Df);
  for (long long r0 = 0; r0 < Nnew; r0 += ldn) {
    const long long n = std::min(ldn, Nnew - r0);
    qf_chunk(Xnew + r0 * P, n, dX, dm, dv);
    LpdArgs a;
    a.lik = k.lik, a.J = k.dimf, a.T = T_, a.param = k.qparam, a.N = n;
    a.y = dy.d() + r0, a.ldy = Nnew;
    a.m = dm.d() + k.d0, a.v = dv.d() + k.d0, a.ldf = Df, a.absv = true;
    a.lpd = dl.d() + r0, a.ess = ess ? de.d() + r0 : nullptr;
    launch_log_predictive_gh(a, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (dX is reused by the next chunk's upload)
  }
  HIP_TRY(hipMemcpy(lpd, dl.p, sizeof(double) * Nnew, hipMemcpyDeviceToHost));
  if (ess) HIP_TRY(hipMemcpy(ess, de.p, sizeof(double) * Nnew, hipMemcpyDeviceToHost));
}

// predict_log_density's loop with the cdf / quantile kernels behind q(f).  Every check comes before the first launch.
void hmogp_engine::predict_cdf_quantile(int t, const double* Xnew, const double* ynew, long long Nnew, int T_, double* cdf, double* sf,
                                        int nP, const double* p, double* q) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to predict from"};
  if (t < 0 || t >= T) throw EngineError{HMOGP_E_INVALID, "task index out of range"};
  const Task& k = tasks[t];
  if (const char* why = predq_refusal(k.lik)) throw EngineError{HMOGP_E_INVALID, why};
  const bool quant = q != nullptr;
  if (quant && (nP < 1 || nP > HMOGP_QUANT_MAXP || !p)) throw EngineError{HMOGP_E_INVALID, "nP must be in 1 .. HMOGP_QUANT_MAXP"};
  if (Nnew < 0 || (Nnew > 0 && (!Xnew || (!quant && !ynew)))) throw EngineError{HMOGP_E_INVALID, "bad predict arguments"};
  if (Nnew == 0) return;
  HIP_TRY(hipSetDevice(device));
  DevBuf dy, d1, d2;
  const OrdinalTable* tb = k.lik == HMOGP_LIK_ORDINAL ? &task_table(k) : nullptr;
  if (!quant) upload_y_cdf(k.lik, k.param, tb, ynew, Nnew, dy);   // (checks the labels; throws before anything is launched)
  if (quant) d1.ensure(sizeof(double) * Nnew * nP);
  if (!quant && cdf) d1.ensure(sizeof(double) * Nnew);
  if (!quant && sf) d2.ensure(sizeof(double) * Nnew);
  ensure_workspace(std::min(chunk, std::max<long long>(Nnew, 1)));
  ensure_strict_workspace();
  const long long ldn = ws_rows;
  DevBuf dX, dm, dv;
  dX.ensure(sizeof(double) * ldn * P), dm.ensure(sizeof(double) * ldn * Df), dv.ensure(sizeof(double) * ldn * Df);
  for (long long r0 = 0; r0 < Nnew; r0 += ldn) {
    const long long n = std::min(ldn, Nnew - r0);
    qf_chunk(Xnew + r0 * P, n, dX, dm, dv);
    PqArgs a;
    a.lik = k.lik, a.T = T_, a.param = k.qparam, a.table = tb, a.N = n;
    a.m = dm.d() + k.d0, a.v = dv.d() + k.d0, a.ldf = Df, a.absv = true;
    if (quant) {
      a.nP = nP, a.q = d1.d() + r0 * nP;
      for (int i = 0; i < nP; ++i) a.p[i] = p[i];
      launch_predictive_quantile(a, st);
    } else {
      a.y = dy.d() + r0, a.ldy = Nnew;
      a.cdf = cdf ? d1.d() + r0 : nullptr, a.sf = sf ? d2.d() + r0 : nullptr;
      launch_predictive_cdf(a, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (dX is reused by the next chunk's upload)
  }
  if (quant) HIP_TRY(hipMemcpy(q, d1.p, sizeof(double) * Nnew * nP, hipMemcpyDeviceToHost));
  if (!quant && cdf) HIP_TRY(hipMemcpy(cdf, d1.p, sizeof(double) * Nnew, hipMemcpyDeviceToHost));
  if (!quant && sf) HIP_TRY(hipMemcpy(sf, d2.p, sizeof(double) * Nnew, hipMemcpyDeviceToHost));
}

// the joint posterior of the functions d[0 .. nD) at Xnew, function-major (n = nD * Nnew).  The mean is q(f)'s own (qf_chunk:
// the same bits as hmogp_predict_f).  G_q = A_q C_q A_q^T follows the mode of the evaluation it is taken from, as qf_chunk does:
//   default  T = A_q C_q, G_q = T A_q^T                                              (the explicit C_q)
//   strict   R = A_q Kuu^-1 by the row solves against Luu, T = R L_q, G_q = T T^T - R A_q^T   (svmogp_inf.py:214-218, literally)
// Every product is the existing GEMM ACCUMULATING into a zeroed target (beta = 1): that pins the general FP64-MFMA kernel whatever the
// row count, so an entry's k-order -- and with it its bits -- does not depend on which other rows or functions the call has.  Only the
// lower tiles of G_q are formed; joint_assemble_kernel reads only them.  Every refusal comes before the first device call.
void hmogp_engine::joint(const double* Xnew, long long Nnew, int nD, const int* d, double* mean, double* cov, int S,
                         unsigned long long seed, double* F, double* Lout, double* jitter_out, int* rung_out) {
  const bool sample = S != 0 || F != nullptr;
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to predict from"};
  if (nD < 1 || !d) throw EngineError{HMOGP_E_INVALID, "joint: nD must be >= 1 and d_index given"};
  {
    std::vector<char> seen((size_t)Df, 0);
    for (int j = 0; j < nD; ++j) {
      if (d[j] < 0 || d[j] >= Df) throw EngineError{HMOGP_E_INVALID, "joint: a function index is out of range"};
      if (seen[d[j]]) throw EngineError{HMOGP_E_INVALID, "joint: a function index is repeated"};
      seen[d[j]] = 1;
    }
  }
  if (Nnew < 0) throw EngineError{HMOGP_E_INVALID, "bad predict arguments"};
  if (Nnew > HMOGP_JOINT_MAXDIM || (long long)nD * Nnew > HMOGP_JOINT_MAXDIM)
    throw EngineError{HMOGP_E_INVALID, "joint: nD * Nnew exceeds HMOGP_JOINT_MAXDIM"};
  if (sample && S < 1) throw EngineError{HMOGP_E_INVALID, "joint: S must be >= 1"};
  if (Nnew > 0 && (!Xnew || (sample ? !F : (!mean || !cov)))) throw EngineError{HMOGP_E_INVALID, "bad predict arguments"};
  if (jitter_out) *jitter_out = 0.0;
  if (rung_out) *rung_out = -1;
  if (Nnew == 0) return;

  HIP_TRY(hipSetDevice(device));
  const long long N = Nnew, n = (long long)nD * N, MM = (long long)M * M, sK = N * M, NN = N * N;
  ensure_workspace(std::min(chunk, N));
  ensure_strict_workspace();           // (the joint posterior follows the mode of the evaluation it is taken from)
  const long long ldn = ws_rows;
  DevBuf dd, dX, dm, dv, jmean, jX, jA, jT, jR, jG, jcov;
  dd.ensure(sizeof(int) * nD);
  HIP_TRY(hipMemcpyAsync(dd.p, d, sizeof(int) * nD, hipMemcpyHostToDevice, st));
  dX.ensure(sizeof(double) * ldn * P), dm.ensure(sizeof(double) * ldn * Df), dv.ensure(sizeof(double) * ldn * Df);
  jmean.ensure(sizeof(double) * n);
  for (long long r0 = 0; r0 < N; r0 += ldn) {
    const long long nn = std::min(ldn, N - r0);
    qf_chunk(Xnew + r0 * P, nn, dX, dm, dv);
    launch_joint_gather(dm.d(), Df, dd.as<int>(), nD, N, r0, nn, jmean.d(), st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (dX is reused by the next chunk's upload)
  }
  jX.ensure(sizeof(double) * N * P), jA.ensure(sizeof(double) * Q * sK), jT.ensure(sizeof(double) * Q * sK);
  jG.ensure(sizeof(double) * Q * NN), jcov.ensure(sizeof(double) * n * n);
  HIP_TRY(hipMemcpyAsync(jX.p, Xnew, sizeof(double) * N * P, hipMemcpyHostToDevice, st));
  RbfBatch rbt;
  rbt.nq = Q, rbt.var = dvar.d(), rbt.ell = dell.d(), rbt.sZ = P, rbt.sK = sK;
  launch_rbf(jX.d(), P, N, P, dZ.d(), Q * P, M, 0.0, 1.0, jA.d(), false, st, nullptr, strict, &rbt);   // A_q: K_uf as qf_chunk rounds it
  HIP_TRY(hipMemsetAsync(jT.p, 0, sizeof(double) * Q * sK, st));
  HIP_TRY(hipMemsetAsync(jG.p, 0, sizeof(double) * Q * NN, st));
  // C_[q] += alpha * A_[q] op(B_[q]), A_ the N x K rows (row-major, lda = M); batched over the latents
  auto acc = [&](const double* A_, const double* B_, long long sB, int b_kmajor, int b_tri, double* C_, int ldc, long long sC,
                 int ncols, double alpha, bool lower) {
    GemmArgs g;
    g.A = A_, g.lda = M, g.a_kmajor = 0, g.sA = sK;
    g.B = B_, g.ldb = M, g.b_kmajor = b_kmajor, g.sB = sB, g.b_tri = b_tri;
    g.C = C_, g.ldc = ldc, g.sC = sC;
    g.M = (int)N, g.N = ncols, g.K = M;
    g.nbatch = Q;
    g.alpha = alpha, g.beta = 1.0;
    g.lower_only = lower ? 1 : 0;
    launch_gemm_f64(g, st);
  };
  if (strict) {
    jR.ensure(sizeof(double) * Q * sK);
    potrs_rows_inplace(jR.d(), sK, Luu.d(), MM, M, N, Q, st, Lsy.d(), jA.d(), rdiag.d(), nullptr, 3, lsym_valid);   // R = A Kuu^-1
    acc(jR.d(), L.d(), MM, 1, +1, jT.d(), M, sK, M, 1.0, false);               // T = R L_q (L_q lower)
    acc(jT.d(), jT.d(), sK, 0, 0, jG.d(), (int)N, NN, (int)N, 1.0, true);      // G = T T^T
    acc(jR.d(), jA.d(), sK, 0, 0, jG.d(), (int)N, NN, (int)N, -1.0, true);     //     - R A^T
  } else {
    acc(jA.d(), C.d(), MM, 1, 0, jT.d(), M, sK, M, 1.0, false);                // T = A C_q
    acc(jT.d(), jA.d(), sK, 0, 0, jG.d(), (int)N, NN, (int)N, 1.0, true);      // G = T A^T
  }
  JointArgs ja;
  ja.P = P, ja.Q = Q, ja.Df = Df, ja.nD = nD, ja.N = N;
  ja.X = jX.d(), ja.G = jG.d(), ja.W = dW.d(), ja.kap = dkap.d(), ja.var = dvar.d(), ja.ell = dell.d();
  ja.d = dd.as<int>(), ja.cov = jcov.d();
  launch_joint_assemble(ja, st);
  HIP_TRY(hipGetLastError());
  if (mean) HIP_TRY(hipMemcpyAsync(mean, jmean.p, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  if (cov) HIP_TRY(hipMemcpyAsync(cov, jcov.p, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
  if (!sample) {
    HIP_TRY(hipStreamSynchronize(st));
    return;
  }
  // L = chol(cov + jitter I) on the ladder hmogp_jitchol_inv climbs (batch of one; the ladder's rung count is bounded), then
  // F = mean + Z L^T: the normal fill writes the mean into F, the GEMM accumulates onto it (L dense, zeros above the diagonal)
  std::vector<double> hdiag((size_t)n);
  HIP_TRY(hipMemcpy2DAsync(hdiag.data(), sizeof(double), jcov.p, sizeof(double) * (n + 1), sizeof(double), (size_t)n,
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  double dmean = 0.0;
  for (long long i = 0; i < n; ++i) dmean += hdiag[i];
  dmean /= (double)n;
  DevBuf jL, jscr, jinfo, jjit, jZ, jF;
  jL.ensure(sizeof(double) * n * n), jscr.ensure(sizeof(double) * n * n), jinfo.ensure(sizeof(int)), jjit.ensure(sizeof(double));
  int r = -2;
  jitchol_batched(jcov.d(), jL.d(), 1, (int)n, &dmean, &r, jinfo.as<int>(), jjit.d(), jscr.d(), st);
  if (rung_out) *rung_out = r;
  if (jitter_out) *jitter_out = r < 0 ? 0.0 : dmean * 1e-6 * std::pow(10.0, r);
  jZ.ensure(sizeof(double) * S * n), jF.ensure(sizeof(double) * S * n);
  launch_joint_normal(seed, S, n, jZ.d(), jmean.d(), jF.d(), st);
  GemmArgs g;
  g.A = jZ.d(), g.lda = (int)n, g.a_kmajor = 0;
  g.B = jL.d(), g.ldb = (int)n, g.b_kmajor = 0, g.b_tri = -1;      // op(B)[k][j] = L[j][k]: zero for k > j
  g.C = jF.d(), g.ldc = (int)n;
  g.M = S, g.N = (int)n, g.K = (int)n;
  g.beta = 1.0;
  launch_gemm_f64(g, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(F, jF.p, sizeof(double) * S * n, hipMemcpyDeviceToHost, st));
  if (Lout) HIP_TRY(hipMemcpyAsync(Lout, jL.p, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
}

// gradients of q(f) with respect to the new inputs, dm / dv [Nnew][Df][P] (v the SIGNED value predict_f returns).  The same
// chunks as predict_f; m and v are qf_chunk's own (the bits of hmogp_predict_f).  A_q is the image the mean was formed with, read back from
// memory by qf_xgrad_kernel: in the default mode qf_chunk's own K_uf, still in Kh (the forward contraction only reads it); in the strict
// mode, whose solves overwrite theirs, the same launch_rbf once more, as joint does.  T_q = A_q C_q follows the mode of the evaluation it is taken from, as joint does:
//   default  T = A C_q                                                                 (the explicit C_q)
//   strict   R = A Kuu^-1 (row solves against Luu), T1 = R L_q, U = T1 L_q^T - A, T = U Kuu^-1   (C_q is never read)
// Every product is the existing GEMM ACCUMULATING into a zeroed target (beta = 1): the general FP64-MFMA kernel whatever the row count,
// so a row's bits do not depend on the chunk.  The mean's coefficients are the engine's `a` in both modes.  Every refusal comes before
// the first device call.
void hmogp_engine::predict_f_grad(const double* Xnew, long long Nnew, double* m, double* v, double* dm_out, double* dv_out) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to predict from"};
  if (Nnew < 0) throw EngineError{HMOGP_E_INVALID, "predict_f_grad: Nnew must be >= 0"};
  if (Nnew > 0 && !Xnew) throw EngineError{HMOGP_E_INVALID, "predict_f_grad: Xnew is NULL"};
  if (Nnew > 0 && (!dm_out || !dv_out)) throw EngineError{HMOGP_E_INVALID, "predict_f_grad: dm and dv must be given"};
  if (Nnew == 0) return;

  HIP_TRY(hipSetDevice(device));
  ensure_workspace(std::min(chunk, std::max<long long>(Nnew, 1)));
  ensure_strict_workspace();           // (the gradients follow the mode of the evaluation they are taken from)
  const long long ldn = ws_rows, MM = (long long)M * M;
  DevBuf dX, dm, dv, gA, gT, gR, gU, ggp, ggc, gdm, gdv;
  dX.ensure(sizeof(double) * ldn * P), dm.ensure(sizeof(double) * ldn * Df), dv.ensure(sizeof(double) * ldn * Df);
  const long long nmax = std::min(ldn, Nnew);
  gT.ensure(sizeof(double) * Q * (strict ? nmax : ldn) * M);
  if (strict) gA.ensure(sizeof(double) * Q * nmax * M), gR.ensure(sizeof(double) * Q * nmax * M), gU.ensure(sizeof(double) * Q * nmax * M);
  ggp.ensure(sizeof(double) * Q * nmax * P), ggc.ensure(sizeof(double) * Q * nmax * P);
  gdm.ensure(sizeof(double) * nmax * Df * P), gdv.ensure(sizeof(double) * nmax * Df * P);
  for (long long r0 = 0; r0 < Nnew; r0 += ldn) {
    const long long n = std::min(ldn, Nnew - r0), sK = (strict ? n : ldn) * M;   // (default mode: Kh's own stride, for A and T alike)
    qf_chunk(Xnew + r0 * P, n, dX, dm, dv);
    const double* A_q = Kh.d();                        // default mode: [Q][ldn * M], the rows qf_chunk's mean was formed with
    if (strict) {
      RbfBatch rbt;
      rbt.nq = Q, rbt.var = dvar.d(), rbt.ell = dell.d(), rbt.sZ = P, rbt.sK = sK;
      launch_rbf(dX.d(), P, n, P, dZ.d(), Q * P, M, 0.0, 1.0, gA.d(), false, st, nullptr, true, &rbt);   // K_uf as qf_chunk rounds it
      A_q = gA.d();
    }
    // C_[q] += A_[q] op(B_[q]), A_ the n x M rows (row-major, lda = M); batched over the latents
    auto acc = [&](const double* A_, const double* B_, int b_kmajor, int b_tri, double* C_) {
      GemmArgs g;
      g.A = A_, g.lda = M, g.a_kmajor = 0, g.sA = sK;
      g.B = B_, g.ldb = M, g.b_kmajor = b_kmajor, g.sB = MM, g.b_tri = b_tri;
      g.C = C_, g.ldc = M, g.sC = sK;
      g.M = (int)n, g.N = M, g.K = M;
      g.nbatch = Q;
      g.alpha = 1.0, g.beta = 1.0;
      launch_gemm_f64(g, st);
    };
    if (strict) {
      potrs_rows_inplace(gR.d(), sK, Luu.d(), MM, M, n, Q, st, Lsy.d(), gA.d(), rdiag.d(), nullptr, 3, lsym_valid);   // R = A Kuu^-1
      HIP_TRY(hipMemsetAsync(gU.p, 0, sizeof(double) * Q * sK, st));
      acc(gR.d(), L.d(), 1, +1, gU.d());                                       // T1 = R L_q   (L_q lower)
      HIP_TRY(hipMemsetAsync(gR.p, 0, sizeof(double) * Q * sK, st));
      acc(gU.d(), L.d(), 0, -1, gR.d());                                       // T1 L_q^T     (op(B)[k][j] = L_q[j][k]: zero for k > j)
      launch_sub(gR.d(), gA.d(), gU.d(), Q * sK, st);                          // U = T1 L_q^T - A
      potrs_rows_inplace(gT.d(), sK, Luu.d(), MM, M, n, Q, st, Lsy.d(), gU.d(), rdiag.d(), nullptr, 3, lsym_valid);   // T = U Kuu^-1
    } else {
      HIP_TRY(hipMemsetAsync(gT.p, 0, sizeof(double) * Q * sK, st));
      acc(A_q, C.d(), 1, 0, gT.d());                                           // T = A C_q
    }
    XgradArgs xa;
    xa.P = P, xa.Q = Q, xa.M = M, xa.ldz = Q * P, xa.n = n, xa.sK = sK, xa.ldo = n;
    xa.A = A_q, xa.T = gT.d(), xa.Z = dZ.d(), xa.a = a.d(), xa.ell = dell.d(), xa.X = dX.d();
    xa.gp = ggp.d(), xa.gc = ggc.d();
    launch_qf_xgrad(xa, st);
    launch_qf_xgrad_combine(ggp.d(), ggc.d(), n, n, Q, Df, P, dW.d(), gdm.d(), gdv.d(), st);
    HIP_TRY(hipGetLastError());
    if (m) HIP_TRY(hipMemcpyAsync(m + r0 * Df, dm.p, sizeof(double) * n * Df, hipMemcpyDeviceToHost, st));
    if (v) HIP_TRY(hipMemcpyAsync(v + r0 * Df, dv.p, sizeof(double) * n * Df, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dm_out + r0 * Df * P, gdm.p, sizeof(double) * n * Df * P, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(dv_out + r0 * Df * P, gdv.p, sizeof(double) * n * Df * P, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (dX is reused by the next chunk's upload)
  }
}

// pathwise (Matheron) posterior samples.  A path set is drawn ONCE from the parameters of the last evaluation -- q(u_q) =
// N(m_q, L_q L_q^T) in dmu / L, K_q = k_q(Z_q, Z_q) from Z and the kernel parameters -- and is a snapshot:
//   omega = zeta / (pi ell_q); theta, eps; u = m_q + eps L_q^T (ONE b_tri product onto the mean); Phi_Z = Phi_q(Z_q) by the feature kernel;
//   R = u - theta Phi_Z^T; v = R K_q^-1 by the row solves against the set's OWN factor of K_q; Theta~ = w theta + sqrt(kappa) theta', V~ = w v.
// One set of bits whatever mode the evaluation ran in.  (a) The factor is NOT the engine's Luu buffer: an M <= 64 evaluation in the default
// mode leaves the factor of the fused small-model kernel there, a strict one the blocked potrf's -- both valid, not the same last bits.
// The set forms K_q itself (launch_rbf with the arguments u_algebra passes) and factorises it with jitchol_batched forced onto the rung
// the evaluation took: the regular kernels' factor of the same matrix on every path, O(Q M^3 / 3) once per set.  (b) The solve is
// potrs_rows_inplace WITHOUT a mirrored factor and pivots' reciprocals: the blocked substitution kernels whatever S is (no strict-mode
// workspace is read).  Every product is the existing GEMM accumulating into its target (beta = 1): the general FP64-MFMA kernel
// whatever the shape.  Every refusal comes before the first device call, each memory question before the allocation it is about.
hmogp_engine::PathSet& hmogp_engine::path_set(int id) {
  if (id < 0 || id >= HMOGP_PATHS_MAXSETS || !path_sets[id].live) throw EngineError{HMOGP_E_INVALID, "paths: unknown or freed path-set id"};
  return path_sets[id];
}

void hmogp_engine::paths_create(int nD, const int* d, int S, int Lf, unsigned long long seed, int* id) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to draw paths from"};
  if (nD < 1 || !d) throw EngineError{HMOGP_E_INVALID, "paths: nD must be >= 1 and d_index given"};
  {
    std::vector<char> seen((size_t)Df, 0);
    for (int j = 0; j < nD; ++j) {
      if (d[j] < 0 || d[j] >= Df) throw EngineError{HMOGP_E_INVALID, "paths: a function index is out of range"};
      if (seen[d[j]]) throw EngineError{HMOGP_E_INVALID, "paths: a function index is repeated"};
      seen[d[j]] = 1;
    }
  }
  if (S < 1) throw EngineError{HMOGP_E_INVALID, "paths: S must be >= 1"};
  if (Lf < 1) throw EngineError{HMOGP_E_INVALID, "paths: Lf must be >= 1"};
  if (Lf > HMOGP_PATHS_MAXFEAT) throw EngineError{HMOGP_E_INVALID, "paths: Lf exceeds HMOGP_PATHS_MAXFEAT"};
  if ((long long)nD * S > HMOGP_PATHS_MAXCOLS) throw EngineError{HMOGP_E_INVALID, "paths: nD * S exceeds HMOGP_PATHS_MAXCOLS"};
  if (!id) throw EngineError{HMOGP_E_INVALID, "paths: id is NULL"};
  int slot = -1;
  for (int i = 0; i < HMOGP_PATHS_MAXSETS && slot < 0; ++i)
    if (!path_sets[i].live) slot = i;
  if (slot < 0) throw EngineError{HMOGP_E_INVALID, "paths: no free slot (HMOGP_PATHS_MAXSETS live path sets)"};

  HIP_TRY(hipSetDevice(device));
  const long long K2 = 2LL * Lf, nc = (long long)nD * S, MM = (long long)M * M, sU = (long long)S * M;
  const long long nZ = (long long)M * Q * P;
  {   // the memory question: the set's state and the draw's workspace, before any allocation
    const double state = 8.0 * ((double)nZ + (double)Q * Lf * P + 3.0 * Q + (double)Q * K2 * nc + (double)Q * M * nc + (double)Q * sU);
    const double work = 8.0 * ((double)Q * S * K2 + 2.0 * Q * sU + (double)Q * M * K2 + 3.0 * Q * MM + 2.0 * Q * nD + HMOGP_MAXQ) + 4.0 * (nD + HMOGP_MAXQ);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (state + work > (double)free_b) {
      char buf[256];
      std::snprintf(buf, sizeof buf, "paths: the set's state (%.0f bytes) and the draw's workspace (%.0f bytes) need %.0f bytes, the device has %.0f free",
                    state, work, state + work, (double)free_b);
      throw EngineError{HMOGP_E_INVALID, buf};
    }
  }
  PathSet& ps = path_sets[slot];
  ps.nD = nD, ps.S = S, ps.Lf = Lf, ps.seed = seed;
  try {
  ps.Z.ensure(sizeof(double) * nZ), ps.omega.ensure(sizeof(double) * Q * Lf * P);
  ps.cq.ensure(sizeof(double) * Q), ps.var.ensure(sizeof(double) * Q), ps.ell.ensure(sizeof(double) * Q);
  ps.Theta.ensure(sizeof(double) * Q * K2 * nc), ps.V.ensure(sizeof(double) * Q * M * nc), ps.u.ensure(sizeof(double) * Q * sU);
  DevBuf dd, dws, dth, deps, dR, dPZ, pK, pLuu, pscr, pinfo, pjit;
  pK.ensure(sizeof(double) * Q * MM), pLuu.ensure(sizeof(double) * Q * MM, true), pscr.ensure(sizeof(double) * Q * MM);
  pinfo.ensure(sizeof(int) * HMOGP_MAXQ), pjit.ensure(sizeof(double) * HMOGP_MAXQ);
  dd.ensure(sizeof(int) * nD), dws.ensure(sizeof(double) * 2 * Q * nD);
  dth.ensure(sizeof(double) * Q * S * K2), deps.ensure(sizeof(double) * Q * sU), dR.ensure(sizeof(double) * Q * sU);
  dPZ.ensure(sizeof(double) * Q * M * K2);
  std::vector<double> hc((size_t)Q), hws((size_t)2 * Q * nD);
  for (int q = 0; q < Q; ++q) {
    hc[q] = std::sqrt(h_var[q] / (double)Lf);
    for (int j = 0; j < nD; ++j) {
      hws[(size_t)q * nD + j] = h_W[(size_t)q * Df + d[j]];
      hws[(size_t)(Q + q) * nD + j] = std::sqrt(h_kap[(size_t)q * Df + d[j]]);
    }
  }
  HIP_TRY(hipMemcpyAsync(dd.p, d, sizeof(int) * nD, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(dws.p, hws.data(), sizeof(double) * 2 * Q * nD, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ps.cq.p, hc.data(), sizeof(double) * Q, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ps.var.p, h_var.data(), sizeof(double) * Q, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ps.ell.p, h_ell.data(), sizeof(double) * Q, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ps.Z.p, dZ.p, sizeof(double) * nZ, hipMemcpyDeviceToDevice, st));
  launch_paths_draw(seed, Q, P, Lf, S, M, ps.ell.d(), dmu.d(), ps.omega.d(), dth.d(), deps.d(), ps.u.d(), st);
  {   // u[q][s][:] = m_q + L_q eps[q][s][:]: op(B)[k][j] = L_q[j][k], zero for k > j
    GemmArgs g;
    g.A = deps.d(), g.lda = M, g.a_kmajor = 0, g.sA = sU;
    g.B = L.d(), g.ldb = M, g.b_kmajor = 0, g.sB = MM, g.b_tri = -1;
    g.C = ps.u.d(), g.ldc = M, g.sC = sU;
    g.M = S, g.N = M, g.K = M;
    g.nbatch = Q;
    g.alpha = 1.0, g.beta = 1.0;
    launch_gemm_f64(g, st);
  }
  PathsArgs fa;
  fa.P = P, fa.Q = Q, fa.Lf = Lf, fa.ldx = Q * P, fa.rows = M, fa.sX = P;
  fa.X = ps.Z.d(), fa.omega = ps.omega.d(), fa.cq = ps.cq.d(), fa.Phi = dPZ.d();
  launch_paths_features(fa, st);                                              // Phi_q(Z_q): [Q][M][2 Lf]
  HIP_TRY(hipMemcpyAsync(dR.p, ps.u.p, sizeof(double) * Q * sU, hipMemcpyDeviceToDevice, st));
  {   // R = u - theta Phi_Z^T: op(B)[k][m] = Phi_Z[m][k]
    GemmArgs g;
    g.A = dth.d(), g.lda = (int)K2, g.a_kmajor = 0, g.sA = (long long)S * K2;
    g.B = dPZ.d(), g.ldb = (int)K2, g.b_kmajor = 0, g.sB = (long long)M * K2;
    g.C = dR.d(), g.ldc = M, g.sC = sU;
    g.M = S, g.N = M, g.K = (int)K2;
    g.nbatch = Q;
    g.alpha = -1.0, g.beta = 1.0;
    launch_gemm_f64(g, st);
  }
  {   // the set's own factor of K_q (see above): K_uu as u_algebra builds it, the blocked potrf on the rung the evaluation took
    RbfBatch kb;
    kb.nq = Q, kb.var = ps.var.d(), kb.ell = ps.ell.d(), kb.sZ = P, kb.sX = P, kb.sK = MM;
    launch_rbf(ps.Z.d(), Q * P, M, P, ps.Z.d(), Q * P, M, 0.0, 1.0, pK.d(), false, st, nullptr, true, &kb);
    std::vector<int> r(rung.begin(), rung.end());
    r.resize((size_t)Q, -1);
    jitchol_batched(pK.d(), pLuu.d(), Q, M, h_var.data(), r.data(), pinfo.as<int>(), pjit.d(), pscr.d(), st);
  }
  potrs_rows_inplace(dR.d(), sU, pLuu.d(), MM, M, S, Q, st);                   // v = R K_q^-1, in place, the rows as right-hand sides
  launch_paths_scale(seed, Q, Lf, S, M, nD, dd.as<int>(), dws.d(), dws.d() + (long long)Q * nD, dth.d(), dR.d(), ps.Theta.d(), ps.V.d(), st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(st));   // (the workspace and the host vectors go out of scope)
  } catch (...) {
    (void)hipStreamSynchronize(st);
    ps.reset();
    throw;
  }
  ps.live = true;
  *id = slot;
}

void hmogp_engine::paths_eval(int id, const double* Xnew, long long Nnew, double* F) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to draw paths from"};
  PathSet& ps = path_set(id);
  if (Nnew < 0) throw EngineError{HMOGP_E_INVALID, "paths: Nnew must be >= 0"};
  if (Nnew > 0 && (!Xnew || !F)) throw EngineError{HMOGP_E_INVALID, "paths: Xnew and F must be given"};
  if (Nnew == 0) return;

  HIP_TRY(hipSetDevice(device));
  const int Lf = ps.Lf;
  const long long K2 = 2LL * Lf, nc = (long long)ps.nD * ps.S;
  // rows per chunk: Phi [Q][rows][2 Lf] of one chunk within PATHS_PHI_BUDGET, and so A [Q][rows][M] and F [S nD][rows] each (a multiple
  // of 128 rows, at least 128), at most the engine's chunk_rows
  const long long widest = std::max<long long>(std::max<long long>(Q * K2, (long long)Q * M), nc);
  long long rows = std::max<long long>(128, PATHS_PHI_BUDGET / (8 * widest) / 128 * 128);
  rows = std::min(std::min(rows, chunk), std::min<long long>(Nnew, 1LL << 20));
  // the chunk workspace stays with the engine (released with the last live set) and only grows: the memory question is about the growth
  DevBuf &pX = paths_wX, &pPhi = paths_wPhi, &pA = paths_wA, &pF = paths_wF;
  const size_t want[4] = {sizeof(double) * rows * P, sizeof(double) * Q * rows * K2, sizeof(double) * Q * rows * M, sizeof(double) * nc * rows};
  DevBuf* const ws[4] = {&pX, &pPhi, &pA, &pF};
  double grow = 0.0;
  for (int i = 0; i < 4; ++i)
    if (want[i] > ws[i]->bytes) grow += (double)want[i] - (double)ws[i]->bytes;
  if (grow > 0.0) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (grow > (double)free_b) {
      char buf[256];
      std::snprintf(buf, sizeof buf, "paths: the evaluation's chunk workspace needs %.0f more bytes, the device has %.0f free", grow, (double)free_b);
      throw EngineError{HMOGP_E_INVALID, buf};
    }
  }
  for (int i = 0; i < 4; ++i) ws[i]->ensure(want[i]);
  for (long long r0 = 0; r0 < Nnew; r0 += rows) {
    const long long n = std::min(rows, Nnew - r0), sK = n * M;
    HIP_TRY(hipMemcpyAsync(pX.p, Xnew + r0 * P, sizeof(double) * n * P, hipMemcpyHostToDevice, st));
    PathsArgs fa;
    fa.P = P, fa.Q = Q, fa.Lf = Lf, fa.ldx = P, fa.rows = n, fa.sX = 0;
    fa.X = pX.d(), fa.omega = ps.omega.d(), fa.cq = ps.cq.d(), fa.Phi = pPhi.d();
    launch_paths_features(fa, st);
    RbfBatch rbt;
    rbt.nq = Q, rbt.var = ps.var.d(), rbt.ell = ps.ell.d(), rbt.sZ = P, rbt.sK = sK;
    launch_rbf(pX.d(), P, n, P, ps.Z.d(), Q * P, M, 0.0, 1.0, pA.d(), false, st, nullptr, true, &rbt);   // A_q: K_uf as the strict qf_chunk rounds it
    HIP_TRY(hipMemsetAsync(pF.p, 0, sizeof(double) * nc * n, st));
    for (int q = 0; q < Q; ++q) {     // F[(s, j)][i] += sum_k Theta~_q[k][(s, j)] Phi_q[i][k] + sum_m V~_q[m][(s, j)] A_q[i][m]
      GemmArgs g;
      g.A = ps.Theta.d() + (long long)q * K2 * nc, g.lda = (int)nc, g.a_kmajor = 1;
      g.B = pPhi.d() + (long long)q * n * K2, g.ldb = (int)K2, g.b_kmajor = 0;
      g.C = pF.d(), g.ldc = (int)n;
      g.M = (int)nc, g.N = (int)n, g.K = (int)K2;
      g.alpha = 1.0, g.beta = 1.0;
      launch_gemm_f64(g, st);
      g.A = ps.V.d() + (long long)q * M * nc;
      g.B = pA.d() + (long long)q * sK, g.ldb = M;
      g.K = M;
      launch_gemm_f64(g, st);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(F + r0, sizeof(double) * Nnew, pF.p, sizeof(double) * n, sizeof(double) * n, (size_t)nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (pX is reused by the next chunk's upload)
  }
}

// G[s][j][i][p] = d f_{d_j}^s / d x_p at Xnew.  Both parts of a path are linear in what the set stores: the prior part is the
// evaluation's own feature image Phi against the rotated operand Theta~(p) (built at the set's first gradient call, kept with it), the
// update part the P derivative images D(p)_q = A_q .* (z_qp - x_p) / l_q^2 of the evaluation's own A_q against V~.  The products are
// paths_eval's, issued per p into G [P][S nD][rows]: every launch has a shape paths_eval runs, an entry's k-order depends on none of N,
// the chunks, S, the function list, or whether F was asked for.  F (optional) comes from the same Phi and A_q by paths_eval's two
// products per latent: its bits.  The workspace is transposed to the caller's layout (P innermost) on the device, then one pitched
// download per chunk.  Every refusal comes before the first device call, the memory question before the allocations it is about.
void hmogp_engine::paths_eval_grad(int id, const double* Xnew, long long Nnew, double* F, double* G) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to draw paths from"};
  PathSet& ps = path_set(id);
  if (Nnew < 0) throw EngineError{HMOGP_E_INVALID, "paths: Nnew must be >= 0"};
  if (Nnew > 0 && (!Xnew || !G)) throw EngineError{HMOGP_E_INVALID, "paths: Xnew and G must be given"};
  if (Nnew == 0) return;

  HIP_TRY(hipSetDevice(device));
  const int Lf = ps.Lf;
  const long long K2 = 2LL * Lf, nc = (long long)ps.nD * ps.S;
  // rows per chunk: paths_eval's rule with the derivative images D [P][Q][rows][M] and the gradient workspace G [P][S nD][rows] counted
  // against the same budget (a multiple of 128 rows, at least 128), at most the engine's chunk_rows
  const long long widest = std::max<long long>(std::max<long long>(Q * K2, (long long)P * Q * M), P * nc);
  long long rows = std::max<long long>(128, PATHS_PHI_BUDGET / (8 * widest) / 128 * 128);
  rows = std::min(std::min(rows, chunk), std::min<long long>(Nnew, 1LL << 20));
  DevBuf &pX = paths_wX, &pPhi = paths_wPhi, &pA = paths_wA, &pF = paths_wF, &pD = paths_wD, &pG = paths_wG, &pGt = paths_wGt;
  const size_t dth_bytes = sizeof(double) * Q * P * K2 * nc;
  const size_t want[7] = {sizeof(double) * rows * P,     sizeof(double) * Q * rows * K2,  sizeof(double) * Q * rows * M,
                          F ? sizeof(double) * nc * rows : 0, sizeof(double) * P * Q * rows * M, sizeof(double) * P * nc * rows,
                          P > 1 ? sizeof(double) * P * nc * rows : 0};
  DevBuf* const ws[7] = {&pX, &pPhi, &pA, &pF, &pD, &pG, &pGt};
  {   // the memory question: the set's rotated operand (first gradient call only) and the workspace's growth, before any allocation
    const double rot = ps.dTheta.p ? 0.0 : (double)dth_bytes;
    double grow = 0.0;
    for (int i = 0; i < 7; ++i)
      if (want[i] > ws[i]->bytes) grow += (double)want[i] - (double)ws[i]->bytes;
    if (rot + grow > 0.0) {
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      if (rot + grow > (double)free_b) {
        char buf[256];
        std::snprintf(buf, sizeof buf, "paths: the gradient's rotated operand (%.0f bytes) and the chunk workspace's growth (%.0f bytes) need %.0f bytes, the device has %.0f free",
                      rot, grow, rot + grow, (double)free_b);
        throw EngineError{HMOGP_E_INVALID, buf};
      }
    }
  }
  if (!ps.dTheta.p) {
    ps.dTheta.ensure(dth_bytes);
    launch_paths_dtheta(Q, P, Lf, (int)nc, ps.omega.d(), ps.Theta.d(), ps.dTheta.d(), st);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < 7; ++i) ws[i]->ensure(want[i]);
  for (long long r0 = 0; r0 < Nnew; r0 += rows) {
    const long long n = std::min(rows, Nnew - r0), sK = n * M;
    HIP_TRY(hipMemcpyAsync(pX.p, Xnew + r0 * P, sizeof(double) * n * P, hipMemcpyHostToDevice, st));
    PathsArgs fa;
    fa.P = P, fa.Q = Q, fa.Lf = Lf, fa.ldx = P, fa.rows = n, fa.sX = 0;
    fa.X = pX.d(), fa.omega = ps.omega.d(), fa.cq = ps.cq.d(), fa.Phi = pPhi.d();
    launch_paths_features(fa, st);
    RbfBatch rbt;
    rbt.nq = Q, rbt.var = ps.var.d(), rbt.ell = ps.ell.d(), rbt.sZ = P, rbt.sK = sK;
    launch_rbf(pX.d(), P, n, P, ps.Z.d(), Q * P, M, 0.0, 1.0, pA.d(), false, st, nullptr, true, &rbt);   // A_q: as paths_eval forms it
    RbfDxArgs dx;
    dx.P = P, dx.Q = Q, dx.M = M, dx.ldz = Q * P, dx.n = n, dx.sK = sK;
    dx.A = pA.d(), dx.X = pX.d(), dx.Z = ps.Z.d(), dx.ell = ps.ell.d(), dx.D = pD.d();
    launch_rbf_dx(dx, st);
    GemmArgs g;
    g.lda = (int)nc, g.a_kmajor = 1, g.b_kmajor = 0;
    g.ldc = (int)n, g.M = (int)nc, g.N = (int)n;
    g.alpha = 1.0, g.beta = 1.0;
    if (F) {
      HIP_TRY(hipMemsetAsync(pF.p, 0, sizeof(double) * nc * n, st));
      for (int q = 0; q < Q; ++q) {   // paths_eval's two products per latent, from the same Phi and A_q
        g.C = pF.d();
        g.A = ps.Theta.d() + (long long)q * K2 * nc;
        g.B = pPhi.d() + (long long)q * n * K2, g.ldb = (int)K2, g.K = (int)K2;
        launch_gemm_f64(g, st);
        g.A = ps.V.d() + (long long)q * M * nc;
        g.B = pA.d() + (long long)q * sK, g.ldb = M, g.K = M;
        launch_gemm_f64(g, st);
      }
    }
    HIP_TRY(hipMemsetAsync(pG.p, 0, sizeof(double) * P * nc * n, st));
    for (int p = 0; p < P; ++p)
      for (int q = 0; q < Q; ++q) {   // G[p][(s, j)][i] += sum_k Theta~(p)_q[k][(s, j)] Phi_q[i][k] + sum_m V~_q[m][(s, j)] D(p)_q[i][m]
        g.C = pG.d() + (long long)p * nc * n;
        g.A = ps.dTheta.d() + ((long long)q * P + p) * K2 * nc;
        g.B = pPhi.d() + (long long)q * n * K2, g.ldb = (int)K2, g.K = (int)K2;
        launch_gemm_f64(g, st);
        g.A = ps.V.d() + (long long)q * M * nc;
        g.B = pD.d() + ((long long)p * Q + q) * sK, g.ldb = M, g.K = M;
        launch_gemm_f64(g, st);
      }
    const double* out = pG.d();
    if (P > 1) {
      launch_paths_gtrans(pG.d(), P, nc, n, pGt.d(), st);
      out = pGt.d();
    }
    HIP_TRY(hipGetLastError());
    if (F) HIP_TRY(hipMemcpy2DAsync(F + r0, sizeof(double) * Nnew, pF.p, sizeof(double) * n, sizeof(double) * n, (size_t)nc, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpy2DAsync(G + r0 * P, sizeof(double) * Nnew * P, out, sizeof(double) * n * P, sizeof(double) * n * P, (size_t)nc,
                             hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // (pX is reused by the next chunk's upload)
  }
}

void hmogp_engine::paths_state(int id, double* omega, double* theta, double* v, double* u) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to draw paths from"};
  PathSet& ps = path_set(id);
  HIP_TRY(hipSetDevice(device));
  const long long K2 = 2LL * ps.Lf, nc = (long long)ps.nD * ps.S;
  if (omega) HIP_TRY(hipMemcpyAsync(omega, ps.omega.p, sizeof(double) * Q * ps.Lf * P, hipMemcpyDeviceToHost, st));
  if (theta) HIP_TRY(hipMemcpyAsync(theta, ps.Theta.p, sizeof(double) * Q * K2 * nc, hipMemcpyDeviceToHost, st));
  if (v) HIP_TRY(hipMemcpyAsync(v, ps.V.p, sizeof(double) * Q * M * nc, hipMemcpyDeviceToHost, st));
  if (u) HIP_TRY(hipMemcpyAsync(u, ps.u.p, sizeof(double) * Q * ps.S * M, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
}

void hmogp_engine::paths_free(int id) {
  if (!evaluated && !began) throw EngineError{HMOGP_E_STATE, "no evaluation to draw paths from"};
  PathSet& ps = path_set(id);
  HIP_TRY(hipSetDevice(device));
  ps.reset();
  bool any = false;
  for (const PathSet& o : path_sets) any = any || o.live;
  if (!any)
    for (DevBuf* b : {&paths_wX, &paths_wPhi, &paths_wA, &paths_wF, &paths_wD, &paths_wG, &paths_wGt}) b->release();
}
