// actuator_kernels.hip -- the actuator audit of a refined trajectory (included by capi.hip; host side in actuator_capi.inc).
// Every production caller of the reference LOOKS at the refined trajectory before it keeps it: utilities_landing/plot_results.m:12-39 computes the joint
// torques, joint velocities and motor voltages and draws them against tauMax and batteryV (:120-136), and generate_training_data_automated.m:200-218
// asks "Save trajectory for training?" behind that figure.  landing_actuator_audit_kernel is that look per member, on the device:
//   tau[k, leg] = J_f(jpos_k)' (-R_world_to_body(rpy_k) f_k,leg)            plot_results.m:14-22, the formulas of landing_kinodyn_rows_kernel (rbd_kernels.hip)
//   jvel[k]     = (jpos[k+1] - jpos[k]) / dt[k], k = 0 .. N-2; jvel[N-1] = 0  :27-29 (diff(jpos) ./ dt_val, zero last column)
//   volt[k]     = tau[k] / gr / (1.5 kt) * Rm + jvel[k] * gr * kt * 2        :31-38
// One workgroup of 256 threads per member; the member's x = [X (12 x (N+1)); jpos (12 x N); U (24 x N)] and its dt go to LDS with contiguous loads, one
// thread per (knot, leg) computes the three joints of that leg from there (4 N <= 256 items), the summary is reduced with __shfl_xor inside a wave
// and through LDS across the four.  The reductions are max, min and integer counts (ties of a peak go to the lowest 12 k + joint), so no result depends
// on the order.  No scratch: every per-thread array is indexed by unrolled constants.
#pragma once

namespace landing {

constexpr int AUD_NSUM = 8, AUD_NMAX = 64, AUD_XMAX = 48 * AUD_NMAX + 12;

struct AuditArgs {
  const RbdModel* model;            // leg lengths l1 .. l4
  int B, N;
  const double* dt; int dt_stride;  // member b's grid = dt + b * dt_stride (0: one grid for all)
  const double* x;                  // [B][48N + 12]
  double gr[3], kt[3], Rm[3], tau_max[3], battery_v;      // landing_actuator_model
  double volt_max, tau_ratio_max, jvel_max; int drive_only;      // landing_actuator_screen (a limit <= 0 is not screened)
  double *tau, *jvel, *volt;        // [B][N][12], each may be NULL
  double* summary;                  // [B][8]
  int* where;                       // [B][4]
  int* ok;                          // [B]
  const int* status3;               // NULL, or the chain's status [B][3] ...
  int* keep;                        // ... and [B]: 0 where the final status is 0 and the member is ok (what the pair writer's scan counts)
};

// a peak and the sample 12 k + joint it was found at; of two equal peaks the lower sample stays
struct AudPeak { double v; int at; };
__device__ inline void aud_take(AudPeak& p, double v, int at) {
  if (v > p.v || (v == p.v && at >= 0 && (p.at < 0 || at < p.at))) { p.v = v; p.at = at; }
}

__global__ __launch_bounds__(PL_THREADS) void landing_actuator_audit_kernel(AuditArgs A) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  const int b = blockIdx.x, tid = threadIdx.x, NT = blockDim.x, N = A.N;
  const int nxk = kd_nx(N), nX = 12 * (N + 1), nJ = 12 * N;
  __shared__ double s_x[AUD_XMAX], s_dt[AUD_NMAX];
  __shared__ double s_red[PL_THREADS / 64][6];
  __shared__ int s_redi[PL_THREADS / 64][5];
  const double* xb = A.x + (size_t)b * nxk;
  const double* dtb = A.dt + (size_t)b * A.dt_stride;
  int bad = 0;
  for (int i = tid; i < nxk; i += NT) { const double v = xb[i]; s_x[i] = v; bad |= !isfinite(v); }
  if (tid < N) { const double v = dtb[tid]; s_dt[tid] = v; bad |= !isfinite(v); }
  __syncthreads();

  AudPeak pv{-1.0, -1}, pd{-1.0, -1};      // peak |v|, peak |v| where tau * jvel > 0
  double ratio = 0.0, vel = 0.0, pmax = -INFINITY, pmin = INFINITY;
  int nv = 0, nd = 0;
  if (tid < 4 * N) {
    const int k = tid >> 2, leg = tid & 3;
    const RbdModel& M = *A.model;
    const double* X = s_x + 12 * k;
    const double* jp = s_x + nX + 12 * k + 3 * leg;
    const double* f = s_x + nX + nJ + 24 * k + 12 + 3 * leg;
    double R[3][3];      // body -> world (rpyToRotMat_xyz.m:2); R_world_to_body is its transpose
    pl_rot_xyz(X[3], X[4], X[5], R);
    const double fb0 = -(R[0][0] * f[0] + R[1][0] * f[1] + R[2][0] * f[2]);
    const double fb1 = -(R[0][1] * f[0] + R[1][1] * f[1] + R[2][1] * f[2]);
    const double fb2 = -(R[0][2] * f[0] + R[1][2] * f[1] + R[2][2] * f[2]);
    const double ss = (leg & 1) ? 1.0 : -1.0;      // sideSign = [-1, 1, -1, 1] (get_foot_jacobians_mc.m:3)
    double s1, c1, s2, c2, s3, c3;
    sincos(jp[0], &s1, &c1); sincos(jp[1], &s2, &c2); sincos(jp[2], &s3, &c3);
    const double c23 = c2 * c3 - s2 * s3, s23 = s2 * c3 + c2 * s3, l14 = M.l1 + M.l4;
    const double J[3][3] = {{0.0, M.l3 * c23 + M.l2 * c2, M.l3 * c23},      // get_foot_jacobians_mc.m:19-21
                            {M.l3 * c1 * c23 + M.l2 * c1 * c2 - l14 * s1 * ss, -M.l3 * s1 * s23 - M.l2 * s1 * s2, -M.l3 * s1 * s23},
                            {M.l3 * s1 * c23 + M.l2 * c2 * s1 + l14 * ss * c1, M.l3 * c1 * s23 + M.l2 * c1 * s2, M.l3 * c1 * s23}};
    const bool last = k == N - 1;
    const double h = last ? 1.0 : s_dt[k];
    const size_t o = ((size_t)b * N + k) * 12 + 3 * leg;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double tau = J[0][j] * fb0 + J[1][j] * fb1 + J[2][j] * fb2;
      const double qd = last ? 0.0 : (jp[12 + j] - jp[j]) / h;
      const double cur = tau / A.gr[j] / (1.5 * A.kt[j]);
      const double v = cur * A.Rm[j] + qd * A.gr[j] * A.kt[j] * 2.0;
      if (A.tau) A.tau[o + j] = tau;
      if (A.jvel) A.jvel[o + j] = qd;
      if (A.volt) A.volt[o + j] = v;
      bad |= !(isfinite(tau) && isfinite(qd) && isfinite(v));
      const double av = fabs(v), pw = tau * qd, r = fabs(tau) / A.tau_max[j], aq = fabs(qd);
      const int at = 12 * k + 3 * leg + j;
      if (r > ratio) ratio = r;
      if (aq > vel) vel = aq;
      if (pw > pmax) pmax = pw;
      if (pw < pmin) pmin = pw;
      aud_take(pv, av, at);
      nv += av > A.battery_v;
      if (pw > 0.0) { aud_take(pd, av, at); nd += av > A.battery_v; }
    }
  }
  // wave reduction (every lane of the workgroup takes part; lanes without an item hold the neutral values)
  for (int m = 1; m < 64; m <<= 1) {
    const double r2 = __shfl_xor(ratio, m), q2 = __shfl_xor(vel, m), a2 = __shfl_xor(pmax, m), i2 = __shfl_xor(pmin, m);
    if (r2 > ratio) ratio = r2;
    if (q2 > vel) vel = q2;
    if (a2 > pmax) pmax = a2;
    if (i2 < pmin) pmin = i2;
    const double v2 = __shfl_xor(pv.v, m), w2 = __shfl_xor((double)pv.at, m), d2 = __shfl_xor(pd.v, m), e2 = __shfl_xor((double)pd.at, m);
    aud_take(pv, v2, (int)w2); aud_take(pd, d2, (int)e2);
    nv += (int)__shfl_xor((double)nv, m); nd += (int)__shfl_xor((double)nd, m);
    bad |= (int)__shfl_xor((double)bad, m);
  }
  const int w = tid >> 6;
  if ((tid & 63) == 0) {
    s_red[w][0] = ratio; s_red[w][1] = vel; s_red[w][2] = pv.v; s_red[w][3] = pd.v; s_red[w][4] = pmax; s_red[w][5] = pmin;
    s_redi[w][0] = pv.at; s_redi[w][1] = pd.at; s_redi[w][2] = nv; s_redi[w][3] = nd; s_redi[w][4] = bad;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int u = 1; u < PL_THREADS / 64; ++u) {
    if (s_red[u][0] > ratio) ratio = s_red[u][0];
    if (s_red[u][1] > vel) vel = s_red[u][1];
    if (s_red[u][4] > pmax) pmax = s_red[u][4];
    if (s_red[u][5] < pmin) pmin = s_red[u][5];
    aud_take(pv, s_red[u][2], s_redi[u][0]); aud_take(pd, s_red[u][3], s_redi[u][1]);
    nv += s_redi[u][2]; nd += s_redi[u][3]; bad |= s_redi[u][4];
  }
  const double peak = pv.at >= 0 ? pv.v : 0.0, drive = pd.at >= 0 ? pd.v : 0.0;
  double* S = A.summary + (size_t)b * AUD_NSUM;
  S[0] = ratio; S[1] = vel; S[2] = peak; S[3] = drive; S[4] = pmax; S[5] = pmin; S[6] = (double)nv; S[7] = (double)nd;
  int* W = A.where + 4 * (size_t)b;
  W[0] = pv.at >= 0 ? pv.at / 12 : -1; W[1] = pv.at >= 0 ? pv.at % 12 : -1;
  W[2] = pd.at >= 0 ? pd.at / 12 : -1; W[3] = pd.at >= 0 ? pd.at % 12 : -1;
  bool ok = !bad;
  if (A.volt_max > 0.0) ok = ok && (A.drive_only ? drive : peak) <= A.volt_max;
  if (A.tau_ratio_max > 0.0) ok = ok && ratio <= A.tau_ratio_max;
  if (A.jvel_max > 0.0) ok = ok && vel <= A.jvel_max;
  A.ok[b] = ok ? 1 : 0;
  if (A.status3) {      // the pair writer behind the screen: final status of the chain's three columns, rejected members marked
    const int fin = pl_final_status(A.status3[3 * b + 1], A.status3[3 * b + 2]);
    A.keep[b] = fin != 0 ? fin : (ok ? 0 : -1);
  }
}

}  // namespace landing
