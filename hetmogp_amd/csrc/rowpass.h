// rowpass.h -- launchers of the row-streaming kernels: K_uf and its windows (kuf.hip), the quadrature (quad.hip), the column statistics,
// reductions and wire format (rowpass.hip), the strict mode's row kernels (strict_rows.hip, trsm_panel.hip), the joint posterior (joint.hip).
// The per-family building blocks: lik_launch.h.
#pragma once
#include "common.h"
#include "../../include/hetmogp_hip.h"

#define HMOGP_MAXJ 8  // max latent functions per task (Categorical K <= 9; Dirichlet K <= 4)
#define HMOGP_MAXQ 8  // max latent GPs
// scalar statistics one quad block emits: [0] sum ve, [1] #(v<0), [2+2q] sa_q, [3+2q] sl_q, then J x sgv, then Q x J x swk
#define HMOGP_MAXSCAL (2 + 2 * HMOGP_MAXQ + HMOGP_MAXJ + HMOGP_MAXQ * HMOGP_MAXJ)

struct QuadArgs {
  int lik = 0;
  double lik_param = 0.0;
  int dimf = 1, Q = 1;
  long long N = 0;                 // rows of this chunk
  long long off = 0;               // added to the row index of the [Q][ldn] vectors below (0: the pointers are already offset)
  const double* y = nullptr;       // [N]
  const double* yaux = nullptr;    // [N] gammaln(y+1) (Poisson, Negative Binomial, zero-inflated Poisson) or nullptr
  // Ordinal: y / yaux are the row's own LOWER / UPPER cut point (-inf / +inf at the ends) and lik_param is sigma
  const double* p = nullptr;       // [Q][ldn]  K^ a
  const double* c = nullptr;       // [Q][ldn]  rowsum(P~ .* K^)
  const double* pt = nullptr;      // [Q][ldn]  r2-weighted twins (nullptr when no hyper-gradients are wanted)
  const double* ct = nullptr;
  long long ldn = 0;
  double w[HMOGP_MAXQ][HMOGP_MAXJ];    // live W[q][d(j)]
  double w0[HMOGP_MAXQ][HMOGP_MAXJ];   // construction-time W (quirk Q3)
  double kap[HMOGP_MAXQ][HMOGP_MAXJ];  // live kappa
  double var[HMOGP_MAXQ];              // RBF variances
  double scale = 1.0;                  // batch_scale[t]
  // [r4] the same five inputs read from DEVICE memory instead (all non-null together; the by-value copies above are then ignored):
  // what lets a captured hipGraph of the evaluation be replayed with new hyper-parameters.  Wd / W0d / kapd: [Q][Df] (row q,
  // column d0 + j), vard: [Q], scaled: one value
  const double *Wd = nullptr, *W0d = nullptr, *kapd = nullptr, *vard = nullptr, *scaled = nullptr;
  int Df = 0, d0 = 0;
  unsigned quirks = 0x1fu;             // HMOGP_QUIRK_* (default: reproduce the reference)
  double* alpha = nullptr;             // [Q][ldn] outputs: row weights of the backward pass
  double* beta = nullptr;
  double* alpha0 = nullptr;
  double* beta0 = nullptr;
  double* partials = nullptr;          // [nblocks][nscal]
  double* out_mu = nullptr;            // optional [N][dimf]: q(f) mean / variance (prediction, parity tests)
  double* out_v = nullptr;
  double* out_gm = nullptr;            // optional [N][dimf]: scaled d ve / d m, d ve / d v (inner-protocol debug export)
  double* out_gv = nullptr;
  // strict q(f) (HMOGP_CFG_STRICT_QF): p / c above are the solve-based forms (q(f) of svmogp_inf.py:212-218); the block scalars
  // sa / swk take these explicit-inverse forms instead (K^ a, rowsum(P~ .* K^): the reference's gradient code, :157-161)
  const double* pg = nullptr;          // [Q][ldn] or nullptr (= p)
  const double* cg = nullptr;          // [Q][ldn] or nullptr (= c)
  // Dirichlet: `y` is row 0 of the task's [K][ldy] array of log y_k, offset to the chunk's first row like every per-row
  // vector; ldy is the task's own row count, whatever slice of it the chunk is.  Weibull: `y` is row 0 of the task's
  // [2][ldy] image (log y, delta); delta = y[ldy + n] takes the place of yaux.  No other likelihood reads it.
  long long ldy = 0;
};

// strict q(f): the row statistics of the solve-based forms (strict_rows.hip: strict_rowstats_kernel)
struct StrictRows {
  int phase = 0, M = 0, Q = 1, P = 1, ldz = 0;
  long long n = 0, ldn = 0, sK = 0, sZ = 0;
  const double *Kh = nullptr, *Ah = nullptr, *Tt = nullptr, *Pt = nullptr;   // [Q][sK] row-major n x M
  const double* mu = nullptr;     // [M][Q] q_u_means                     (two-solve form: Ah holds A = K^ Kuu^-1)
  const double* w3 = nullptr;     // [Q][M] Luu^-1 m_q  ([r6] one-solve form: Ah holds X = K^ Luu^-T; nullptr = two-solve form)
  const double* a = nullptr;      // [Q][M] Kuu^-1 m
  const double *X = nullptr, *Z = nullptr, *ell = nullptr;
  double *p = nullptr, *c = nullptr, *pg = nullptr, *cg = nullptr, *pt = nullptr, *ct = nullptr;   // [Q][ldn]
  const double* t2 = nullptr;     // [Q][ldn] phase 0: rowsum(T .* T) already formed by the product's epilogue (Tt is not read)
};
void launch_strict_rowstats(const StrictRows& a, hipStream_t s);
// one <= 32-column diagonal block of the blocked triangular solves V L^T = B (dir 0) / A L = V (dir 1), in place, batched over Q
// [u0, u1): columns of the same 128-column block that receive the block's right-looking update inside the launch (needs
// trsm_diag_can_fuse; u0 == u1: none)
void launch_trsm_diag(int dir, double* V, long long sV, const double* L, long long sL, int M, int j0, int nb, long long n, int Q,
                      hipStream_t s, int u0 = 0, int u1 = 0, const double* Vsrc = nullptr);
bool trsm_diag_can_fuse(const double* V, long long sV, int M);
// [r6] one 128-column block of the same solves as ONE launch: long-K update + in-tile substitution (trsm_panel.hip)
struct TrsmPanelArgs {
  double* V = nullptr;             // [Q][sV]: n x M row-major (ldv), solved in place
  const double* Vsrc = nullptr;    // optional: this block's right-hand sides are read from here (first touch of the forward solve)
  long long sV = 0;
  int ldv = 0;
  const double* Lsym = nullptr;    // [Q][sL]: the factor mirrored into a full symmetric image (launch_mirror_lower), ldl
  long long sL = 0;
  int ldl = 0;
  const double* rdiag = nullptr;   // [Q][sR]: 1 / Luu[j][j]  (launch_rdiag)
  long long sR = 0;
  long long n = 0;
  int M = 0, j0 = 0, Q = 1;
  // row statistics of the solved tile in the epilogue of the LAST direction a caller runs (nullptr: none):
  //   sp += tile . st_vec[columns],   sk += rowsum(tile .* st_K)  -- or rowsum(tile .* tile) when st_K is null
  const double* st_K = nullptr;    // same layout as V
  const double* st_vec = nullptr;  // element (column j, batch q) at st_vec[q * st_vecB + j * st_vecS]
  long long st_vecB = 0, st_vecS = 1;
  double* st_part = nullptr;       // [Q][st_sPart]: [2 statistics][4 wave columns][st_ld]
  long long st_sPart = 0, st_ld = 0;
};
bool trsm_panel_eligible(const TrsmPanelArgs& g);
void launch_trsm_panel(int dir, const TrsmPanelArgs& g, hipStream_t s);
void launch_rdiag(const double* L, long long sL, int M, int Q, double* out, long long sR, hipStream_t s);
void launch_trsm_stats_combine(const double* part, long long sPart, long long ld, int nparts, long long n, int Q, const double* t2,
                               double* p, double* c, long long ldn, hipStream_t s);

// [r4] every segment (task x row range) of a pool in one launch -- small models only: the weights are read from device memory
#define HMOGP_QUAD_MULTI 8
struct QuadSeg {
  int lik = 0, dimf = 1, d0 = 0, t = 0;  // likelihood id, functions, first function column, task (index of its batch scale)
  double lik_param = 0.0;
  long long N = 0, off = 0;              // rows, first row within the pool's row vectors
  const double* y = nullptr;
  const double* yaux = nullptr;
  unsigned blk0 = 0;                     // first block of the segment        } filled by launch_quad_multi
  long long part0 = 0;                   // its first word in `partials`      }
  long long ldy = 0;                     // Dirichlet: row stride of y = log y_k [K][ldy]; Weibull: of (log y, delta) [2][ldy] (QuadArgs::ldy)
};
struct QuadMulti {
  int nseg = 0, Q = 1, Df = 0;
  long long ldn = 0;
  const double *p = nullptr, *c = nullptr, *pt = nullptr, *ct = nullptr;
  const double *Wd = nullptr, *W0d = nullptr, *kapd = nullptr, *vard = nullptr, *scale_base = nullptr;
  unsigned quirks = 0x1fu;
  double *alpha = nullptr, *beta = nullptr, *alpha0 = nullptr, *beta0 = nullptr, *partials = nullptr;
  QuadSeg seg[HMOGP_QUAD_MULTI];
};

// per-latent strides of the batched (grid.z = latent) row kernels
struct RbfBatch {
  int nq = 1;
  const double* var = nullptr;  // [nq] device
  const double* ell = nullptr;  // [nq] device
  long long sZ = 0, sK = 0, sWin = 0;
  long long sX = 0;             // per-latent offset of the row inputs (K_uu: the rows are the latent's own inducing inputs)
};
struct ColBatch {
  int nq = 1;
  long long sK = 0, sA = 0, sV = 0, sZ = 0, sPart = 0, sWin = 0;
};

// the quadrature's block partials of every segment of the pool, summed into the bundle by small_red_kernel's extra plane (small models) or by
// reduce_rows_multi_kernel (regular path)
struct SmallQuadRed {
  int nseg = 0;
  struct {
    const double* part = nullptr;  // [nrows][nscal]
    long long nrows = 0;
    int nscal = 0;
    const long long* off = nullptr;   // [nscal] slot -> bundle offset (distinct within a segment)
  } s[8];
};

long long quad_blocks(int lik, long long N);
// [r5] is there an instantiation of quad_multi_kernel for exactly this set of likelihoods (other than the all-inclusive one, which
// runs one wave per SIMD)?
bool quad_multi_specialised(const QuadMulti& m);
// the block partials of every segment of a quad_multi launch -> bundle, segment after segment per slot (the order and the per-
// segment sums of launch_reduce_rows called once per segment: same bits)
void launch_reduce_rows_multi(const SmallQuadRed& qr, double* dst, hipStream_t s);
void launch_quad(const QuadArgs& a, hipStream_t s);
void launch_quad_multi(const QuadMulti& m, hipStream_t s);   // fills blk0 / part0 of the segments; partials laid out segment by segment
// Joint posterior covariance at new inputs (joint.hip): cov[(j, i), (j', i')] = sum_q (w_jq w_j'q + kap_jq [j == j']) k_q(x_i, x_i')
// + w_jq w_j'q G_q[max(i, i'), min(i, i')] for every pair of the nD functions d[j], one 64 x 64 tile of (i, i') per block; lower tiles
// computed, their mirror images written from the same registers.  G: [Q][N][N] (only its lower triangle is read); W, kap: [Q][Df];
// var, ell: [Q]; X: [N][P]; cov: [nD N][nD N].  Every pointer is device memory.
struct JointArgs {
  int P = 1, Q = 1, Df = 1, nD = 1;
  long long N = 0;
  const double *X = nullptr, *G = nullptr, *W = nullptr, *kap = nullptr, *var = nullptr, *ell = nullptr;
  const int* d = nullptr;          // [nD]
  double* cov = nullptr;
};
void launch_joint_assemble(const JointArgs& a, hipStream_t s);
// Z[s][i] = z0 of normal_pair(seed, row i, sample s, pair 0) for s < S, i < n; with F (and mean [n]): F[s][i] = mean[i] beside it
void launch_joint_normal(unsigned long long seed, int S, long long n, double* Z, const double* mean, double* F, hipStream_t s);
// mean[j * N + i] = m[i * Df + d[j]]: the joint vector's function-major mean out of q(f)'s [N][Df] rows (i0: first row of the chunk)
void launch_joint_gather(const double* m, int Df, const int* d, int nD, long long N, long long i0, long long nrows, double* mean,
                         hipStream_t s);
// Pathwise posterior samples (paths.hip).  The feature map of `rows` inputs for every latent:
//   Phi[q][i][l] = c_q cos(pi t), Phi[q][i][Lf + l] = c_q sin(pi t), t = sum_p omega[q][l][p] x_ip in p order (one sincospi per (i, l)).
// X: row i of latent q at X + q sX + i ldx (sX = 0: the same rows for every latent; the inducing inputs: X = Z, ldx = Q P, sX = P);
// omega: [Q][Lf][P]; cq: [Q]; Phi: [Q][rows][2 Lf].  Every pointer is device memory.  A value depends on its own row and frequency alone.
struct PathsArgs {
  int P = 1, Q = 1, Lf = 1, ldx = 1;
  long long rows = 0, sX = 0;
  const double *X = nullptr, *omega = nullptr, *cq = nullptr;
  double* Phi = nullptr;
};
void launch_paths_features(const PathsArgs& a, hipStream_t s);
// The draws of one path set (header of include/hetmogp_hip.h's paths block: the stream tags): omega [Q][Lf][P] = zeta / (pi ell_q);
// theta [Q][S][2 Lf]; eps [Q][S][M]; u [Q][S][M] = m_q (mu: [M][Q]) for the b_tri product u += eps L_q^T to accumulate onto
void launch_paths_draw(unsigned long long seed, int Q, int P, int Lf, int S, int M, const double* ell, const double* mu, double* omega,
                       double* theta, double* eps, double* u, hipStream_t s);
// Theta~[q][k][s nD + j] = w[q][j] theta[q][s][k] + sk[q][j] theta'(d[j], q, s)[k];  V~[q][m][s nD + j] = w[q][j] v[q][s][m]
// (w, sk: [Q][nD] -- W_q[d_j], sqrt(kappa_q[d_j]); d: [nD]; theta: [Q][S][2 Lf]; v: [Q][S][M])
void launch_paths_scale(unsigned long long seed, int Q, int Lf, int S, int M, int nD, const int* d, const double* w, const double* sk,
                        const double* theta, const double* v, double* Theta, double* V, hipStream_t s);
// Gradients of the paths with respect to the new inputs (pathsgrad.hip).  The rotated operand of the prior part,
//   dTheta[q][p][l][c] = (pi omega[q][l][p]) Theta[q][Lf + l][c],  dTheta[q][p][Lf + l][c] = -(pi omega[q][l][p]) Theta[q][l][c]
// (omega: [Q][Lf][P]; Theta: [Q][2 Lf][nc]; dTheta: [Q][P][2 Lf][nc]): d/dx_p (phi^T Theta) = phi^T dTheta(p).
void launch_paths_dtheta(int Q, int P, int Lf, int nc, const double* omega, const double* Theta, double* dTheta, hipStream_t s);
// The derivative images of A_q = k_q(X, Z_q) for the n rows of one chunk: D[p][q][i][m] = A[q][i][m] ((z_qmp - x_ip) inv_l2), inv_l2 =
// 1 / (l_q l_q), in that order of operations.  A: [Q][sK], n x M row-major; D: [P][Q][sK]; Z: latent q's inducing inputs at Z + q P, row
// stride ldz; X: [n][P]; ell: [Q].  Every pointer is device memory.  An entry depends on its own row, m and p alone.
struct RbfDxArgs {
  int P = 1, Q = 1, M = 0, ldz = 0;
  long long n = 0, sK = 0;
  const double *A = nullptr, *X = nullptr, *Z = nullptr, *ell = nullptr;
  double* D = nullptr;
};
void launch_rbf_dx(const RbfDxArgs& g, hipStream_t s);
// Gt[c][i][p] = G[p][c][i] (G: [P][nc][n], Gt: [nc][n][P]): the gradient workspace of a chunk into the caller's layout, P innermost
void launch_paths_gtrans(const double* G, int P, long long nc, long long n, double* Gt, hipStream_t s);
// Gradients of q(f) with respect to the new inputs (xgrad.hip): gp[q][i][j] = (1 / l_q^2) sum_m a_qm A_q[i][m] (z_qmj - x_ij),
// gc[q][i][j] = (2 / l_q^2) sum_m T_q[i][m] A_q[i][m] (z_qmj - x_ij) for the n rows of one chunk.  A, T: [Q][sK], n x M row-major (lda = M);
// Z: latent q's inducing inputs at Z + q P, row stride ldz; a: [Q][M]; ell: [Q]; X: [n][P]; gp, gc: [Q][ldo][P].  Every pointer is device
// memory.  A wave owns a few rows and shares nothing between them but the loaded a and z: a row's bits depend on that row's own inputs alone.
struct XgradArgs {
  int P = 1, Q = 1, M = 0, ldz = 0;
  long long n = 0, sK = 0, ldo = 0;
  const double *A = nullptr, *T = nullptr, *Z = nullptr, *a = nullptr, *ell = nullptr, *X = nullptr;
  double *gp = nullptr, *gc = nullptr;
  int vec = 0;                     // (set by the launcher: M even and the rows 16-byte aligned)
};
void launch_qf_xgrad(const XgradArgs& a, hipStream_t s);
// dm[i][d][j] = sum_q W_qd gp[q][i][j], dv[i][d][j] = sum_q W_qd^2 gc[q][i][j] (q from left to right); W: [Q][Df]; dm, dv: [n][Df][P]
void launch_qf_xgrad_combine(const double* gp, const double* gc, long long ldo, long long n, int Q, int Df, int P, const double* W,
                             double* dm, double* dv, hipStream_t s);
// K[n][m] = var * exp(-r2/2); X rows have stride ldx, Z rows stride ldz (block q of the M x Q*P inducing array)
void launch_rbf(const double* X, int ldx, long long N, int P, const double* Z, int ldz, int M, double var, double ell,
                double* K, bool same, hipStream_t s, const int* rowwin = nullptr, bool exact = true,
                const RbfBatch* batch = nullptr);
void launch_reduce_slabs_lower(const double* slabs, int nslabs, int M, double* dst, bool accumulate, hipStream_t s, int nb = 1,
                               long long sSlabs = 0, long long sDst = 0);
// exact-zero windows of K^ = k(X, Z) for one (row chunk, latent): rowwin [tiles][2] column range per 128-row tile,
// colwin [ncb][2] row range per 128-column block, hit [tiles][ncb] scratch (see kuf.hip)
void launch_windows(const double* X, long long N, int P, const double* Z, int ldz, int M, double ell, int* rowwin, int* colwin,
                    unsigned char* hit, hipStream_t s);
void launch_colstats(const double* Kh, const double* Pt, const double* a, const double* alpha, const double* alpha0,
                     const double* beta0, const double* X, int P, const double* Z, int ldz, long long N, int M, int rows,
                     bool want_z, double* partials, hipStream_t s, const int* colwin = nullptr, const ColBatch* batch = nullptr,
                     int max_blocks = 0, const double* Ar = nullptr, const double* ell = nullptr);
// partial slab per row split: [ r (M) | dZ (M*P) | s2 (M) ], s2[m] = sum_n E_nm |x_n - z_m|^2 / l^2 when `ell` ([nq], device) is given
void launch_sum_cols(const double* v, int Q, int M, double* dst, long long sDst, hipStream_t s);   // dst[q * sDst] += sum_m v[q][m]
void launch_reduce_rows(const double* partials, long long nrows, int len, const long long* off, double* dst, bool accumulate,
                        hipStream_t s);
void launch_reduce_slabs(const double* slabs, int nslabs, long long stride, long long len, double* dst, bool accumulate,
                         hipStream_t s, int nb = 1, long long sSlabs = 0, long long sDst = 0);
void launch_mirror_lower(double* A, int Q, int M, long long stride, hipStream_t s);
// statistic bundle <-> wire format (lower triangles of H_q only); dir 0 = pack, 1 = unpack (lower triangle only)
void launch_wire_copy(double* bundle, double* wire, long long NG, int Q, int M, long long per_q, int dir, hipStream_t s);
// inner-protocol debug export: out[m][n] = a[m] gm[n][j] + 2 w gv[n][j] Pt[n][m]   (svmogp_inf.py:157-161), out is [M][N]
void launch_raw_kmn(const double* a, const double* gm, const double* gv, int J, int j, double w, const double* Pt, int M,
                    long long N, double* out, hipStream_t s);
