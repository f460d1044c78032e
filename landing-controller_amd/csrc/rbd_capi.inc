// rbd_capi.inc -- host side of the rigid-body entry points (included by capi.hip; kernels in rbd_kernels.hip and wb_kernels.hip): the model upload,
// floating-base dynamics, leg IK, the kinodynamic rows, the whole-body backward pass / roll-out / selection, and the reference's Mini-Cheetah model.

// Foot forces, foot positions and the leg IK reach a foot by composing bodies 0..5 and then b_foot-3 .. b_foot-1: a tree numbered otherwise (landing_rbd_set_model
// accepts any) would give wrong numbers without an error, so the entry points that touch a foot refuse it.
static int rbd_need_legs(const landing_ctx* ctx, const std::string& who) {
  if (!ctx->rbd_legs) return fail(LANDING_E_ARG, who + ": needs a model whose bodies 0..5 are the base chain and whose legs are the consecutive bodies b_foot-3 .. b_foot-1 on body 6 (landing_rbd_set_model)");
  return 0;
}

extern "C" {

// ---- floating-base rigid-body routines (rbd_kernels.hip) ------------------------------------------------------------------
int landing_rbd_set_model(landing_ctx* ctx, const landing_rbd_model* model) {
  if (!ctx || !model) return fail(LANDING_E_ARG, "landing_rbd_set_model: bad argument");
  static_assert(sizeof(landing_rbd_model) == sizeof(landing::RbdModel), "C ABI and device model layouts agree");
  for (int i = 0; i < 18; ++i) {
    if (model->parent[i] < 0 || model->parent[i] > i || model->jtype[i] < 0 || model->jtype[i] > 5) return fail(LANDING_E_ARG, "landing_rbd_set_model: parent must precede its child, joint type 0..5");
  }
  for (int l = 0; l < 4; ++l) if (model->b_foot[l] < 3 || model->b_foot[l] > 18) return fail(LANDING_E_ARG, "landing_rbd_set_model: foot bodies are the third link of a leg chain");
  HIP_TRY(hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!ctx->d_rbd) HIP_TRY(ctx->d_rbd.alloc(1));
  HIP_TRY(hipMemcpy(ctx->d_rbd.get(), model, sizeof(landing::RbdModel), hipMemcpyHostToDevice));
  if (ctx->d_kd_pairs) {      // the Hessian pair table of the kinodynamic NLP was probed with the previous model (kd_ensure_pairs): built again at the next use
    HIP_TRY(hipDeviceSynchronize());      // (a launch of an earlier call may still read it)
    ctx->d_kd_pairs.reset(); ctx->kd_npair = 0;
  }
  if (ctx->d_kd_jpat) { HIP_TRY(hipDeviceSynchronize()); ctx->d_kd_jpat.reset(); }      // (kd_ensure_jpat: the same)
  { bool arrow = true;       // parent = [0 1 2 3 4 5 | 6 7 8 | 6 10 11 | 6 13 14 | 6 16 17]
    for (int i = 0; i < 6; ++i) arrow = arrow && model->parent[i] == i;
    for (int l = 0; l < 4; ++l) arrow = arrow && model->parent[6 + 3 * l] == 6 && model->parent[7 + 3 * l] == 7 + 3 * l && model->parent[8 + 3 * l] == 8 + 3 * l;
    ctx->rbd_arrow = arrow; }
  { bool legs = true;        // what hand_c, rnea_tangent, the kinodynamic rows and the IK compose for a foot: bodies 0..5, then b_foot-3 .. b_foot-1 (0-based), each on its predecessor
    for (int i = 0; i < 6; ++i) legs = legs && model->parent[i] == i;
    for (int l = 0; l < 4; ++l) { const int jb = model->b_foot[l] - 1; legs = legs && model->parent[jb - 2] == 6 && model->parent[jb - 1] == jb - 1 && model->parent[jb] == jb; }
    ctx->rbd_legs = legs; }
  { bool sb = true;      // base joints Px Py Pz Rx Ry Rz in a chain, identity tree transforms: the kinodynamic rows take the base transform from R and pos (rbd_kernels.hip kd_stage_rows)
    const int want[6] = {3, 4, 5, 0, 1, 2};
    for (int i = 0; i < 6; ++i) {
      sb = sb && model->parent[i] == i && model->jtype[i] == want[i];
      for (int j = 0; j < 9; ++j) sb = sb && model->E[i][j] == ((j % 4 == 0) ? 1.0 : 0.0);
      for (int j = 0; j < 3; ++j) sb = sb && model->r[i][j] == 0.0;
    }
    ctx->rbd_std_base = sb ? 1 : 0; }
  return 0;
}

int landing_fb_dynamics_batch(landing_ctx* ctx, int npts, const double* d_q, const double* d_qd, const double* d_tau, const double* d_f_foot,
                              double* d_H, double* d_C, double* d_qdd, double* d_A, double* d_Hinv, double fd_h, void* stream) {
  if (ctx && npts == 0) return 0;
  if (!ctx || npts < 0 || !d_q || !d_qd) return fail(LANDING_E_ARG, "landing_fb_dynamics_batch: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_fb_dynamics_batch: no model (landing_rbd_set_model)");
  if ((d_qdd || d_A) && !d_tau) return fail(LANDING_E_ARG, "landing_fb_dynamics_batch: qdd / A need tau");
  if (d_f_foot) if (const int rc = rbd_need_legs(ctx, "landing_fb_dynamics_batch with foot forces")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::FbArgs a{ctx->d_rbd.get(), npts, d_q, d_qd, d_tau, d_f_foot, d_H, d_C, d_qdd, d_A, d_Hinv, fd_h > 0.0 ? fd_h : 1e-6, ctx->rbd_arrow ? 1 : 0};
  if (d_H || d_C || (d_qdd && !(d_A && fd_h <= 0.0))) hipLaunchKernelGGL(landing::landing_fb_hc_kernel, dim3((npts + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
  if (d_A && fd_h <= 0.0) {
    // exact linearisation (forward mode): pass 1 leaves qdd and H^-1 per knot in the caller's buffers or in a context scratch
    // (stream-ordered reuse: one linearisation in flight per context), pass 2 pushes the 36 tangent directions through the recursion
    double* qs = d_qdd; double* hs = d_Hinv;
    std::lock_guard<std::mutex> lock(ctx->mu);      // the scratch belongs to the context (host threads sharing it are serialised here)
    if (!qs || !hs) {
      HIP_TRY(ctx->d_fb_scratch.grow((size_t)npts * (18 + 324)));      // hipFree waits for the device: no launch still reads the old block
      if (!qs) qs = ctx->d_fb_scratch.get();
      if (!hs) hs = ctx->d_fb_scratch.get() + (size_t)npts * 18;
    }
    const bool own = (qs == ctx->d_fb_scratch.get()) || (hs == ctx->d_fb_scratch.get() + (size_t)npts * 18);
    if (own) HIP_TRY(scratch_acquire(ctx, (hipStream_t)stream));
    hipLaunchKernelGGL(landing::landing_fb_lin_exact_prep_kernel, dim3((npts + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, qs, hs);
    const long long n = 36LL * npts;
    if (a.arrow) hipLaunchKernelGGL(landing::landing_fb_lin_exact_kernel<true>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a, (const double*)qs, (const double*)hs);
    else hipLaunchKernelGGL(landing::landing_fb_lin_exact_kernel<false>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a, (const double*)qs, (const double*)hs);
    if (own) HIP_TRY(scratch_release(ctx, (hipStream_t)stream));
  } else if (d_A || d_Hinv) {
    const long long n = 54LL * npts;
    hipLaunchKernelGGL(landing::landing_fb_lin_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

int landing_leg_ik_batch(landing_ctx* ctx, int npts, const double* d_q6, const double* d_c, const double* jpos_min3, const double* jpos_max3,
                         int iters, double* d_jpos, double* d_res, void* stream) {
  if (ctx && npts == 0) return 0;
  if (!ctx || npts < 0 || !d_q6 || !d_c || !d_jpos || !jpos_min3 || !jpos_max3 || iters < 1) return fail(LANDING_E_ARG, "landing_leg_ik_batch: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_leg_ik_batch: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_leg_ik_batch")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::IkArgs a{ctx->d_rbd.get(), npts, d_q6, d_c, d_jpos, d_res, iters, {jpos_min3[0], jpos_min3[1], jpos_min3[2]}, {jpos_max3[0], jpos_max3[1], jpos_max3[2]}};
  const long long n = 4LL * npts;
  hipLaunchKernelGGL(landing::landing_leg_ik_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int landing_kinodyn_rows_batch(landing_ctx* ctx, int npts, const double* d_q6, const double* d_c, const double* d_f, const double* d_jpos,
                               double* d_fk, double* d_fk_err, double* d_tau, void* stream) {
  if (ctx && npts == 0) return 0;
  if (!ctx || npts < 0 || !d_q6 || !d_jpos || (d_fk_err && !d_c) || (d_tau && !d_f)) return fail(LANDING_E_ARG, "landing_kinodyn_rows_batch: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_rows_batch: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_rows_batch")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::KdArgs a{ctx->d_rbd.get(), npts, d_q6, d_c, d_f, d_jpos, d_fk, d_fk_err, d_tau};
  hipLaunchKernelGGL(landing::landing_kinodyn_rows_kernel, dim3((npts + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int landing_wb_backward(landing_ctx* ctx, int B, int N, double dt, double reg, const double* d_x, const double* d_u, const double* d_xref,
                        const double* d_A, const double* d_Hinv, const double* Q36, const double* R12, const double* QN36,
                        double* d_K, double* d_kff, double* d_dV, int* d_ok, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 1 || !(dt > 0.0) || !d_x || !d_u || !d_xref || !d_A || !d_Hinv || !Q36 || !R12 || !QN36 || !d_K || !d_kff || !d_dV || !d_ok)
    return fail(LANDING_E_ARG, "landing_wb_backward: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  landing::WbBackArgs a;
  a.B = B; a.N = N; a.dt = dt; a.reg = reg; a.semi = ctx->wb_semi; a.x = d_x; a.u = d_u; a.xref = d_xref; a.A = d_A; a.Hinv = d_Hinv;
  for (int i = 0; i < 36; ++i) { a.Q[i] = Q36[i]; a.QN[i] = QN36[i]; }
  for (int i = 0; i < 12; ++i) a.R[i] = R12[i];
  a.K = d_K; a.kff = d_kff; a.dV = d_dV; a.ok = d_ok;
  hipLaunchKernelGGL(landing::landing_wb_backward_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int landing_wb_set_integrator(landing_ctx* ctx, int semi_implicit) {
  if (!ctx) return fail(LANDING_E_ARG, "landing_wb_set_integrator: bad argument");
  ctx->wb_semi = semi_implicit ? 1 : 0;
  return 0;
}

/* the NEXT landing_wb_rollout call on this context skips the members whose d_step entry is non-zero (second stage of a two-stage step-length search) */
int landing_wb_skip_taken(landing_ctx* ctx, const double* d_step) {
  if (!ctx) return fail(LANDING_E_ARG, "landing_wb_skip_taken: bad argument");
  ctx->wb_skip = d_step;
  return 0;
}

int landing_wb_select(landing_ctx* ctx, int B, int N, int nalpha, const double* d_alphas, const int* d_ok, const double* d_xnew, const double* d_unew,
                      const double* d_costnew, double* d_x, double* d_u, double* d_cost, double* d_step, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 1 || nalpha == 0 || !d_alphas || !d_ok || !d_xnew || !d_unew || !d_costnew || !d_x || !d_u || !d_cost || (nalpha < 0 && !d_step)) return fail(LANDING_E_ARG, "landing_wb_select: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  landing::WbSelArgs a{B, N, nalpha < 0 ? -nalpha : nalpha, nalpha < 0 ? 1 : 0, d_alphas, d_ok, d_xnew, d_unew, d_costnew, d_x, d_u, d_cost, d_step};
  hipLaunchKernelGGL(landing::landing_wb_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

int landing_wb_rollout(landing_ctx* ctx, int B, int N, int nalpha, const double* d_alphas, double dt, const double* d_x, const double* d_u,
                       const double* d_xref, const double* d_f_foot, const double* d_K, const double* d_kff, const double* Q36, const double* R12,
                       const double* QN36, double* d_xnew, double* d_unew, double* d_cost, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 1 || nalpha < 1 || !(dt > 0.0) || !d_alphas || !d_x || !d_u || !d_xref || !Q36 || !R12 || !QN36 || !d_xnew || !d_unew || !d_cost ||
      ((d_K == nullptr) != (d_kff == nullptr)))
    return fail(LANDING_E_ARG, "landing_wb_rollout: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_wb_rollout: no model (landing_rbd_set_model)");
  if (d_f_foot) if (const int rc = rbd_need_legs(ctx, "landing_wb_rollout with foot forces")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::WbRollArgs a;
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N; a.nalpha = nalpha; a.dt = dt; a.semi = ctx->wb_semi; a.alphas = d_alphas; a.x = d_x; a.u = d_u; a.xref = d_xref; a.f_foot = d_f_foot;
  a.K = d_K; a.kff = d_kff; a.skip = ctx->wb_skip; ctx->wb_skip = nullptr;
  a.arrow = ctx->rbd_arrow ? 1 : 0;
  for (int i = 0; i < 36; ++i) { a.Q[i] = Q36[i]; a.QN[i] = QN36[i]; }
  for (int i = 0; i < 12; ++i) a.R[i] = R12[i];
  a.xnew = d_xnew; a.unew = d_unew; a.cost = d_cost;
  const long long n = (long long)nalpha * B;
  hipLaunchKernelGGL(landing::landing_wb_rollout_lds_kernel, dim3((unsigned)((n + landing::WB_TPB - 1) / landing::WB_TPB)), dim3(64), 0, (hipStream_t)stream, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

/* The reference's 'quad3D' Mini-Cheetah tree with the 'mc3D' parameters (get_robot_model.m:134-234, get_robot_params.m:50-115) in the compact
 * form of landing_rbd_model -- what landing-controller_amd/rbd.py::quad3d_model builds for the Python callers, for C / mex callers. */
void landing_rbd_model_mc3d(landing_rbd_model* M) {
  memset(M, 0, sizeof(*M));
  struct Rbi { double m, h[3], I[6]; };
  auto rbi = [](double m, const double* com, const double (*rot)[3]) {      /* spatialInertia.m: (m, m c, rot + m (c'c 1 - c c')) about the origin */
    Rbi o; o.m = m;
    const double cc = com[0] * com[0] + com[1] * com[1] + com[2] * com[2];
    double Ib[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) Ib[i][j] = rot[i][j] + m * ((i == j ? cc : 0.0) - com[i] * com[j]);
    for (int i = 0; i < 3; ++i) o.h[i] = m * com[i];
    o.I[0] = Ib[0][0]; o.I[1] = Ib[0][1]; o.I[2] = Ib[0][2]; o.I[3] = Ib[1][1]; o.I[4] = Ib[1][2]; o.I[5] = Ib[2][2];
    return o;
  };
  auto flip_y = [](Rbi a) { a.h[1] = -a.h[1]; a.I[1] = -a.I[1]; a.I[4] = -a.I[4]; return a; };      /* flipAlongAxis(I, 'Y'), get_robot_model.m:852-889 */
  const double c_ab[3] = {0, 0.036, 0}, c_hip[3] = {0, 0.016, -0.02}, c_kn[3] = {0, 0, -0.061}, c_b[3] = {0, 0, 0};
  const double r_ab[3][3] = {{381e-6, 58e-6, 0.45e-6}, {58e-6, 560e-6, 0.95e-6}, {0.45e-6, 0.95e-6, 444e-6}};
  const double r_hip[3][3] = {{1983e-6, 245e-6, 13e-6}, {245e-6, 2103e-6, 1.5e-6}, {13e-6, 1.5e-6, 408e-6}};
  const double r_kn[3][3] = {{6e-6, 0, 0}, {0, 248e-6, 0}, {0, 0, 245e-6}};
  const double r_b[3][3] = {{11253e-6, 0, 0}, {0, 36203e-6, 0}, {0, 0, 42673e-6}};
  const Rbi abad = rbi(0.54, c_ab, r_ab), hip = rbi(0.634, c_hip, r_hip), knee = rbi(0.064, c_kn, r_kn), body = rbi(3.3, c_b, r_b);
  const double abad_loc[3] = {0.19, 0.049, 0.0}, hip_loc[3] = {0, 0.062, 0.0}, knee_loc[3] = {0, 0, -0.209}, foot_loc[3] = {0, 0, -0.195};
  const double side[3][4] = {{1, 1, -1, -1}, {-1, 1, -1, 1}, {1, 1, 1, 1}};
  const double cpi = cos(M_PI), spi = sin(M_PI);      /* rz(pi) as the reference (and rbd.py) forms it: sin(pi) = 1.2e-16, not 0 */
  const double eye[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, rzpi[9] = {cpi, spi, 0, -spi, cpi, 0, 0, 0, 1};
  auto put = [&](int i, int parent, int jt, const double* E, const double* r, const Rbi* in) {
    M->parent[i] = parent; M->jtype[i] = jt;
    for (int j = 0; j < 9; ++j) M->E[i][j] = E[j];
    for (int j = 0; j < 3; ++j) { M->r[i][j] = r[j]; M->h[i][j] = in ? in->h[j] : 0.0; }
    M->m[i] = in ? in->m : 0.0;
    for (int j = 0; j < 6; ++j) M->I[i][j] = in ? in->I[j] : 0.0;
  };
  const double zero3[3] = {0, 0, 0};
  const int base_jt[6] = {3, 4, 5, 0, 1, 2};      /* Px Py Pz Rx Ry Rz */
  for (int i = 0; i < 6; ++i) put(i, i, base_jt[i], eye, zero3, i == 5 ? &body : nullptr);
  int nb = 6, leg_side = -1;
  for (int leg = 0; leg < 4; ++leg) {
    const double s[3] = {side[0][leg], side[1][leg], side[2][leg]};
    const Rbi la = leg_side > 0 ? abad : flip_y(abad), lh = leg_side > 0 ? hip : flip_y(hip), lk = leg_side > 0 ? knee : flip_y(knee);
    double r1[3], r2[3], r3[3];
    for (int j = 0; j < 3; ++j) { r1[j] = s[j] * abad_loc[j]; r2[j] = s[j] * hip_loc[j]; r3[j] = s[j] * knee_loc[j]; M->foot_r[leg][j] = s[j] * foot_loc[j]; }
    put(nb, 6, 0, eye, r1, &la); put(nb + 1, nb + 1, 1, rzpi, r2, &lh); put(nb + 2, nb + 2, 1, eye, r3, &lk);
    M->b_foot[leg] = nb + 3;
    nb += 3; leg_side = -leg_side;
  }
  M->l1 = 0.062; M->l2 = 0.209; M->l3 = 0.195; M->l4 = 0.004;      /* get_foot_jacobians_mc.m:5-8 */
}

}  // extern "C"
