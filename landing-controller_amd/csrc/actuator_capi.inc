// actuator_capi.inc -- host side of the actuator audit (included by capi.hip; kernel in actuator_kernels.hip): the motor data of the reference's model,
// the audit of a batch of refined trajectories on device or host arrays, and the chain's pair writer behind the screen.

static_assert(landing::AUD_NSUM == LANDING_AUDIT_NSUM, "summary length of the header and the kernel agree");

static int aud_check(landing_ctx* ctx, int B, const void* dt, int dt_stride, const void* x, const void* summary, const void* where, const void* ok, const char* who) {
  if (!ctx || B < 0 || !dt || !x || !summary || !where || !ok) return fail(LANDING_E_ARG, std::string(who) + ": bad argument");
  if (ctx->L.N < 2 || ctx->L.N > landing::AUD_NMAX) return fail(LANDING_E_ARG, std::string(who) + ": the refinement takes 2 <= N <= 64 intervals");
  if (dt_stride != 0 && dt_stride < ctx->L.N) return fail(LANDING_E_ARG, std::string(who) + ": dt_stride is 0 (one grid for all members) or at least N");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, std::string(who) + ": no model (landing_rbd_set_model)");
  return rbd_need_legs(ctx, who);
}

static int aud_launch(landing_ctx* ctx, int B, const double* d_dt, int dt_stride, const double* d_x_kd, const landing_actuator_model* model,
                      const landing_actuator_screen* screen, double* d_tau, double* d_jvel, double* d_volt, double* d_summary, int* d_where, int* d_ok,
                      const int* d_status3, int* d_keep, hipStream_t st) {
  landing_actuator_model m;
  landing_actuator_screen s;
  if (model) m = *model; else landing_actuator_model_mc3d(&m);
  if (screen) s = *screen; else landing_actuator_screen_default(&s);
  landing::AuditArgs A;
  A.model = ctx->d_rbd.get(); A.B = B; A.N = ctx->L.N; A.dt = d_dt; A.dt_stride = dt_stride; A.x = d_x_kd;
  for (int i = 0; i < 3; ++i) { A.gr[i] = m.gr[i]; A.kt[i] = m.kt[i]; A.Rm[i] = m.Rm[i]; A.tau_max[i] = m.tau_max[i]; }
  A.battery_v = m.battery_v;
  A.volt_max = s.volt_max; A.tau_ratio_max = s.tau_ratio_max; A.jvel_max = s.jvel_max; A.drive_only = s.drive_only;
  A.tau = d_tau; A.jvel = d_jvel; A.volt = d_volt; A.summary = d_summary; A.where = d_where; A.ok = d_ok; A.status3 = d_status3; A.keep = d_keep;
  hipLaunchKernelGGL(landing::landing_actuator_audit_kernel, dim3(B), dim3(landing::PL_THREADS), 0, st, A);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

void landing_actuator_model_mc3d(landing_actuator_model* m) {
  const double gr[3] = {6.0, 6.0, 9.33}, kt = 0.05, Rm = 0.173, motor_tau_max = 3.0;      // get_robot_params.m:109-114
  for (int i = 0; i < 3; ++i) { m->gr[i] = gr[i]; m->kt[i] = kt; m->Rm[i] = Rm; m->tau_max[i] = gr[i] * motor_tau_max; }      // get_robot_model.m:237-241
  m->battery_v = 24.0;      // get_robot_params.m:115
}

void landing_actuator_screen_default(landing_actuator_screen* s) {
  s->volt_max = 24.0; s->tau_ratio_max = 0.0; s->jvel_max = 0.0; s->drive_only = 1;      // landing_optimization.m:191-199: the limit binds where the motor does positive work
}

int landing_actuator_audit_batch(landing_ctx* ctx, int B, const double* d_dt, int dt_stride, const double* d_x_kd, const landing_actuator_model* model,
                                 const landing_actuator_screen* screen, double* d_tau, double* d_jvel, double* d_volt, double* d_summary, int* d_where,
                                 int* d_ok, void* stream) {
  if (ctx && B == 0) return 0;
  if (const int rc = aud_check(ctx, B, d_dt, dt_stride, d_x_kd, d_summary, d_where, d_ok, "landing_actuator_audit_batch")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  return aud_launch(ctx, B, d_dt, dt_stride, d_x_kd, model, screen, d_tau, d_jvel, d_volt, d_summary, d_where, d_ok, nullptr, nullptr, (hipStream_t)stream);
}

int landing_actuator_audit_host(landing_ctx* ctx, int B, const double* dt, int dt_stride, const double* x_kd, const landing_actuator_model* model,
                                const landing_actuator_screen* screen, double* tau, double* jvel, double* volt, double* summary, int* where, int* ok) {
  if (ctx && B == 0) return 0;
  if (const int rc = aud_check(ctx, B, dt, dt_stride, x_kd, summary, where, ok, "landing_actuator_audit_host")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t b = (size_t)B, N = (size_t)ctx->L.N;
  Staging st(nullptr);
  const double* d_dt = st.in(dt, dt_stride ? (b - 1) * (size_t)dt_stride + N : N); const double* d_x = st.in(x_kd, b * (size_t)landing::kd_nx(ctx->L.N));
  double* d_tau = st.out(tau, b * N * 12); double* d_jvel = st.out(jvel, b * N * 12); double* d_volt = st.out(volt, b * N * 12);
  double* d_sum = st.out(summary, b * landing::AUD_NSUM); int* d_where = st.out(where, 4 * b); int* d_ok = st.out(ok, b);
  HIP_TRY(st.error());
  if (const int rc = aud_launch(ctx, B, d_dt, dt_stride, d_x, model, screen, d_tau, d_jvel, d_volt, d_sum, d_where, d_ok, nullptr, nullptr, nullptr)) return rc;
  HIP_TRY(st.fetch());
  return 0;
}

int landing_pipeline_screened_pairs_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x_kd, const int* d_status3,
                                          const landing_actuator_model* model, const landing_actuator_screen* screen, double* d_summary, int* d_where,
                                          int* d_ok, double* d_in, double* d_out, int* d_index, int* d_count, void* stream) {
  const char* who = "landing_pipeline_screened_pairs_batch";
  if (!ctx || B < 0 || !d_p || !d_x_kd || !d_status3 || !d_summary || !d_where || !d_ok || !d_in || !d_out || !d_index || !d_count) return fail(LANDING_E_ARG, std::string(who) + ": bad argument");
  { const int rc = pl_check_ctx(ctx, who, true); if (rc) return rc; }
  HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  if (B == 0) { HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int), st)); return 0; }
  std::lock_guard<std::mutex> lock(ctx->pl_mu);      // the kept-status block is the chain's (PlBufs::fin), fenced like a chain call
  PlBufs P;
  { const int rc = pl_ensure(ctx, B, &P); if (rc) return rc; }
  HIP_TRY(hipStreamWaitEvent(st, ctx->pl_done, 0));
  struct Fence { landing_ctx* c; hipStream_t s; ~Fence() { (void)hipEventRecord(c->pl_done, s); } } fence{ctx, st};
  if (const int rc = aud_launch(ctx, B, d_p + ctx->L.o_dt, (int)ctx->L.np, d_x_kd, model, screen, nullptr, nullptr, nullptr, d_summary, d_where, d_ok, d_status3, P.fin, st)) return rc;
  return pl_pairs(ctx, B, d_p, d_x_kd, P.fin, d_in, d_out, d_index, d_count, st);
}

}  // extern "C"
