// pipeline_kernels.hip -- the hand-offs of the drop-state chain (included by capi.hip; host side in pipeline_capi.inc).
// Every production caller of the reference runs three solves per drop state, back to back (generate_data/generate_training_data_automated.m:121-219,
// main_scripts/landing_optimization.m:300-322,360-435): the SRBM solve, the kinodynamic refinement from [X*; jpos_guess; U*], the `_ws` re-solve from
// the refinement's x.  The kernels here pose the refinement from the SRBM batch, pick each member's final result and compact the training pairs,
// so that no member array leaves the device between the passes.  Plain loads and stores, one workgroup per member; no scratch, no LDS beyond a few
// scalars (and the scan's 2 x 256 counts).
#pragma once

namespace landing {

constexpr int PL_THREADS = 256;

struct PlPoseArgs {
  Layout L;                       // offsets into p (make_layout(N))
  int B, N;
  const double* p;                // [B][np]
  const double* xs;               // [B][36N + 12] SRBM solutions [X(:); U(:)]
  double comp_eps, slip_eps, fk_band, kbx0, kby0, kby_in, kbz_lo, kbz_hi, tau[3];      // landing_kinodyn_form
  double jmin[12], jmax[12], jguess[3];
  double *lbg, *ubg, *cost, *x0;  // [B][ng], [B][ng], [B][24], [B][48N + 12]
};

// rpyToRotMat_xyz.m:2  R = rx(r)' ry(p)' rz(y)', formed as the host mirror forms it (kinodyn.rot_xyz: the two products left to right, no fused terms)
__device__ inline void pl_rot_xyz(double r, double pt, double y, double R[3][3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const double cr = cos(r), sr = sin(r), cp = cos(pt), sp = sin(pt), cy = cos(y), sy = sin(y);
  const double A[3][3] = {{1, 0, 0}, {0, cr, -sr}, {0, sr, cr}};      // rx'
  const double Bm[3][3] = {{cp, 0, sp}, {0, 1, 0}, {-sp, 0, cp}};     // ry'
  const double Cm[3][3] = {{cy, -sy, 0}, {sy, cy, 0}, {0, 0, 1}};     // rz'
  double T[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[i][j] = A[i][0] * Bm[0][j] + A[i][1] * Bm[1][j] + A[i][2] * Bm[2][j];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = T[i][0] * Cm[0][j] + T[i][1] * Cm[1][j] + T[i][2] * Cm[2][j];
}

// test_scripts/kin_box_limits.m (kinodyn.kin_box_limits)
__device__ inline double pl_kin_box_limit(double v, double box_max) { return fabs(v) < 2.0 ? fabs(v * (box_max / 2.0)) : box_max; }

// Member b's refinement problem (kinodyn.member_problem with every value read from p): lbg / ubg in the row order of landing_kinodyn_bounds, the
// terminal-cost data QN | Xref(:, end), the initial guess [X*; jpos_guess; U*].  Thread 0 forms the attitude-dependent values (c_init of
// landing_optimization.m:232-236, the kinematic box of :249-251); then every thread writes rows tid, tid + 256, ... of each array.
__global__ __launch_bounds__(PL_THREADS) void landing_kd_pose_kernel(PlPoseArgs A) {
  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, N = A.N;
  const Layout& L = A.L;
  const double* p = A.p + (size_t)b * L.np;
  __shared__ double s_c[12], s_kb[2];
  if (tid == 0) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const double* q = p + L.o_q_init;
    const double* qd = p + L.o_qd_init;
    double R[3][3];
    pl_rot_xyz(q[3], q[4], q[5], R);
    const double side[12] = {1, -1, 1, 1, 1, 1, -1, -1, 1, -1, 1, 1}, rel[3] = {0.2, 0.15, -0.3};      // kinodyn.SIDE_SIGN_C, C_REL_INIT (:204, :235)
    for (int l = 0; l < 4; ++l) {
      const double v[3] = {side[3 * l] * rel[0], side[3 * l + 1] * rel[1], side[3 * l + 2] * rel[2]};
      for (int i = 0; i < 3; ++i) s_c[3 * l + i] = q[i] + (R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2]);
    }
    const double vb0 = R[0][0] * qd[3] + R[1][0] * qd[4] + R[2][0] * qd[5];      // body-frame velocity R' v
    const double vb1 = R[0][1] * qd[3] + R[1][1] * qd[4] + R[2][1] * qd[5];
    s_kb[0] = A.kbx0 + pl_kin_box_limit(vb0, 0.15);
    s_kb[1] = A.kby0 + pl_kin_box_limit(vb1, 0.25);
  }
  __syncthreads();
  const int ng = kd_ng(N), nxk = kd_nx(N), nX = 12 * (N + 1);
  const double INF = INFINITY;
  double* lb = A.lbg + (size_t)b * ng;
  double* ub = A.ubg + (size_t)b * ng;
  for (int r = tid; r < ng; r += NT) {
    double lo, hi;
    if (r < KD_BND) {
      const int g = r / 6, i = r % 6;
      switch (g) {
        case 0: lo = hi = p[L.o_q_init + i]; break;
        case 1: lo = hi = p[L.o_qd_init + i]; break;
        case 2: case 3: lo = hi = s_c[r - 12]; break;
        case 4: lo = p[L.o_q_term_min + i]; hi = INF; break;
        case 5: lo = -INF; hi = p[L.o_q_term_max + i]; break;
        case 6: lo = p[L.o_qd_term_min + i]; hi = INF; break;
        default: lo = -INF; hi = p[L.o_qd_term_max + i]; break;
      }
    } else {
      const int k = (r - KD_BND) / KD_ROWS, j = (r - KD_BND) % KD_ROWS;
      const bool last = k == N - 1;
      const int S = last ? 9 : 15;      // rows per leg (the last interval has no slip rows)
      if (j < 12) { lo = 0.0; hi = 0.0; }                                    // Euler defects
      else if (j < 16) { lo = 0.0; hi = INF; }                               // f_z >= 0
      else if (j < 16 + 4 * S) {
        const int l = (j - 16) / S, m = (j - 16) % S, o = last ? 2 : 8;
        if (m == 0) { lo = 0.0; hi = INF; }                                  // c_z >= 0
        else if (m == 1) { lo = -INF; hi = A.comp_eps; }                     // f_z c_z <= eps
        else if (m < o) { if (m < 5) { lo = -INF; hi = A.slip_eps; } else { lo = -A.slip_eps; hi = INF; } }
        else if (m == o) { lo = -s_kb[0]; hi = s_kb[0]; }
        else if (m == o + 1) { if (l == 0 || l == 2) { lo = -s_kb[1]; hi = A.kby_in; } else { lo = -A.kby_in; hi = s_kb[1]; } }
        else if (m == o + 2) { lo = A.kbz_lo; hi = A.kbz_hi; }
        else if (m == o + 3) { const double ll = p[L.o_l_leg_max]; lo = -INF; hi = ll * ll; }
        else { const double t = A.tau[m - o - 4]; lo = -t; hi = t; }
      } else {
        const int m = j - 16 - 4 * S;
        if (m < 16) { lo = -INF; hi = 0.0; }                                 // friction
        else if (m == 16) { lo = p[L.o_q_min + 2]; hi = INF; }               // z >= q_min(3)
        else if (m < 29) { lo = -A.fk_band; hi = INF; }
        else if (m < 41) { lo = -INF; hi = A.fk_band; }
        else if (m < 53) { lo = A.jmin[m - 41]; hi = INF; }
        else { lo = -INF; hi = A.jmax[m - 53]; }
      }
    }
    lb[r] = lo; ub[r] = hi;
  }
  const double* xs = A.xs + (size_t)b * L.nx;
  double* x0 = A.x0 + (size_t)b * nxk;
  for (int i = tid; i < nxk; i += NT) x0[i] = i < nX ? xs[i] : (i < nX + 12 * N ? A.jguess[(i - nX) % 3] : xs[i - 12 * N]);
  if (tid < 24) A.cost[(size_t)b * 24 + tid] = tid < 12 ? p[L.o_QN + tid] : p[12 * N + tid - 12];
}

// dt, mass, Ib, Ib_inv, mu of every member against member 0's: the refinement takes them as one set per batch (landing_kinodyn_params)
__global__ __launch_bounds__(PL_THREADS) void landing_pl_check_kernel(Layout L, int B, const double* p, int* mismatch) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double* q = p + (size_t)b * L.np;
  bool same = q[L.o_mass] == p[L.o_mass] && q[L.o_mu] == p[L.o_mu];
  for (int k = 0; k < L.N; ++k) same = same && q[L.o_dt + k] == p[L.o_dt + k];
  for (int i = 0; i < 3; ++i) same = same && q[L.o_Ib + i] == p[L.o_Ib + i] && q[L.o_Ib_inv + i] == p[L.o_Ib_inv + i];
  if (!same) *mismatch = 1;
}

// final status of a member (landing_nlp.h, landing_pipeline_refine_batch): the warm re-solve's outcome if it converged, else the refinement's if
// that converged (a KKT point of the same NLP), else the warm re-solve's; without the re-solve (s2 < 0) the refinement's
__host__ __device__ inline int pl_final_status(int s1, int s2) { return s2 < 0 ? s1 : (s2 == 0 || s1 == 0 ? 0 : s2); }

struct PlSelectArgs {
  int B, nx, ng, warm;
  const int *st0, *it0;                     // SRBM pass (NULL: column 0 = -1 / 0)
  const int *st1, *it1, *st2, *it2;         // refinement, warm re-solve (warm = 1)
  const double *x1, *f1, *lam1, *kkt1;      // the refinement's result (warm = 1; lam1 NULL when lam is not asked for)
  double *x, *f, *lam, *kkt;                // the warm re-solve's result on entry, the final one on exit (warm = 1)
  int *status3, *iters3, *final_st;         // [B][3], [B][3], [B]
};

__global__ __launch_bounds__(PL_THREADS) void landing_kd_select_kernel(PlSelectArgs A) {
  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int s1 = A.st1[b], s2 = A.warm ? A.st2[b] : -1;
  if (tid == 0) {
    A.status3[3 * b] = A.st0 ? A.st0[b] : -1; A.iters3[3 * b] = A.it0 ? A.it0[b] : 0;
    A.status3[3 * b + 1] = s1; A.iters3[3 * b + 1] = A.it1[b];
    A.status3[3 * b + 2] = s2; A.iters3[3 * b + 2] = A.warm ? A.it2[b] : 0;
    A.final_st[b] = pl_final_status(s1, s2);
  }
  if (!(A.warm && s2 != 0 && s1 == 0)) return;      // (uniform per workgroup)
  for (int i = tid; i < A.nx; i += NT) A.x[(size_t)b * A.nx + i] = A.x1[(size_t)b * A.nx + i];
  if (A.lam && A.lam1)
    for (int i = tid; i < A.ng; i += NT) A.lam[(size_t)b * A.ng + i] = A.lam1[(size_t)b * A.ng + i];
  if (tid == 0 && A.f) A.f[b] = A.f1[b];
  if (tid < 3 && A.kkt) A.kkt[3 * b + tid] = A.kkt1[3 * b + tid];
}

// Stable compaction of the CONVERGED members (final status 0), one workgroup: each thread counts a contiguous run of members, an inclusive scan
// of the 256 counts gives the runs' first columns.  index[j] = member of column j (j < count), -1 behind the last column.
__global__ __launch_bounds__(PL_THREADS) void landing_pl_scan_kernel(int B, const int* final_st, int* index, int* count) {
  __shared__ int s[2][PL_THREADS];
  const int t = threadIdx.x, NT = blockDim.x;
  const int chunk = (B + NT - 1) / NT, lo = t * chunk < B ? t * chunk : B, hi = lo + chunk < B ? lo + chunk : B;
  int n = 0;
  for (int b = lo; b < hi; ++b) n += final_st[b] == 0;
  int cur = 0;
  s[0][t] = n;
  __syncthreads();
  for (int d = 1; d < NT; d <<= 1) {
    s[cur ^ 1][t] = s[cur][t] + (t >= d ? s[cur][t - d] : 0);
    cur ^= 1;
    __syncthreads();
  }
  const int total = s[cur][NT - 1];
  int j = s[cur][t] - n;
  for (int b = lo; b < hi; ++b)
    if (final_st[b] == 0) index[j++] = b;
  for (int k = total + t; k < B; k += NT) index[k] = -1;
  if (t == 0) *count = total;
}

// column j of the training pairs (generate_training_data_automated.m:204-219, dataset.training_pairs with jpos_star): input [q_init(4:6); qd_init]
// (9), output [X(:); U(:); jpos(:)] (48N + 12) from the refinement's x = [X(:); jpos(:); U(:)]
__global__ __launch_bounds__(PL_THREADS) void landing_training_pairs_kernel(Layout L, int N, const double* p, const double* x, const int* index,
                                                                             const int* count, double* in, double* out) {
  const int j = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  if (j >= *count) return;
  const int b = index[j], nxk = kd_nx(N), nX = 12 * (N + 1), nJ = 12 * N, nU = 24 * N;
  const double* xb = x + (size_t)b * nxk;
  const double* pb = p + (size_t)b * L.np;
  double* o = out + (size_t)j * nxk;
  for (int i = tid; i < nxk; i += NT) o[i] = i < nX ? xb[i] : (i < nX + nU ? xb[i + nJ] : xb[i - nU]);
  if (tid < 9) in[(size_t)j * 9 + tid] = tid < 3 ? pb[L.o_q_init + 3 + tid] : pb[L.o_qd_init + tid - 3];
}

}  // namespace landing
