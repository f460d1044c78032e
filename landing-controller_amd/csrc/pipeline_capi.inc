// pipeline_capi.inc -- host side of the drop-state chain (included by capi.hip; kernels in pipeline_kernels.hip, the passes in solver_capi.inc and
// kd_capi.inc).  One call per batch: SRBM solve -> pose -> refinement -> warm re-solve -> final choice -> training pairs, all on the caller's stream.
// The hand-off arrays live in blocks of the context (d_pl, d_pl_int) grown to the largest batch seen; the host reads member 0's dt / mass / Ib /
// Ib_inv / mu (one small copy) and the 4-byte counts of the refinement's host loop, nothing else.

namespace {
struct PlBufs {
  double *lbg, *ubg, *cost, *x0, *x1, *f1, *kkt1, *lam1, *xs;      // pose outputs | the refinement's result | SRBM solutions (landing_pipeline_batch)
  int *flag, *st0, *it0, *st1, *it1, *st2, *it2, *fin;              // parameter mismatch | status / iterations of the three passes | final status
};
}  // namespace

static int pl_check_ctx(landing_ctx* ctx, const char* who, bool need_model) {
  if (ctx->L.run_cost != 0) return fail(LANDING_E_ARG, std::string(who) + ": the chain poses the refinement from the terminal-cost NLP's p (run_cost = 0)");
  if (ctx->L.N < 2 || ctx->L.N > 64) return fail(LANDING_E_ARG, std::string(who) + ": the refinement takes 2 <= N <= 64 intervals");
  if (need_model && !ctx->d_rbd) return fail(LANDING_E_ARG, std::string(who) + ": no model (landing_rbd_set_model)");
  if (need_model) if (const int rc = rbd_need_legs(ctx, who)) return rc;
  return 0;
}

// call with ctx->pl_mu held
static int pl_ensure(landing_ctx* ctx, int B, PlBufs* P) {
  const int N = ctx->L.N;
  const size_t b = (size_t)B, ng = (size_t)landing::kd_ng(N), nxk = (size_t)landing::kd_nx(N), nx = (size_t)ctx->L.nx;
  const size_t nd = b * (3 * ng + 24 + 2 * nxk + 4 + nx), ni = 4 + 7 * b;
  if (!ctx->pl_done) HIP_TRY(hipEventCreateWithFlags(&ctx->pl_done, hipEventDisableTiming));
  if (ctx->d_pl.size() < nd || ctx->d_pl_int.size() < ni) {
    HIP_TRY(hipEventSynchronize(ctx->pl_done));      // (a chain queued by an earlier call may still use the old blocks)
    HIP_TRY(ctx->d_pl.grow(nd)); HIP_TRY(ctx->d_pl_int.grow(ni));
  }
  double* d = ctx->d_pl.get();
  P->lbg = d; d += b * ng; P->ubg = d; d += b * ng; P->lam1 = d; d += b * ng; P->cost = d; d += b * 24; P->x0 = d; d += b * nxk; P->x1 = d; d += b * nxk;
  P->f1 = d; d += b; P->kkt1 = d; d += 3 * b; P->xs = d;
  int* i = ctx->d_pl_int.get();
  P->flag = i; i += 4; P->st0 = i; i += b; P->it0 = i; i += b; P->st1 = i; i += b; P->it1 = i; i += b; P->st2 = i; i += b; P->it2 = i; i += b; P->fin = i;
  return 0;
}

static int pl_pose(landing_ctx* ctx, int B, const double* d_p, const double* d_xs, const landing_pipeline_opts& o, double* d_lbg, double* d_ubg, double* d_cost,
                   double* d_x0, hipStream_t st) {
  landing::PlPoseArgs A;
  A.L = ctx->L; A.B = B; A.N = ctx->L.N; A.p = d_p; A.xs = d_xs;
  A.comp_eps = o.form.comp_eps; A.slip_eps = o.form.slip_eps; A.fk_band = o.form.fk_band; A.kbx0 = o.form.kin_box_x0; A.kby0 = o.form.kin_box_y0;
  A.kby_in = o.form.kin_box_y_in; A.kbz_lo = o.form.kin_box_z_lo; A.kbz_hi = o.form.kin_box_z_hi;
  for (int i = 0; i < 3; ++i) { A.tau[i] = o.form.tau_max[i]; A.jguess[i] = o.jpos_guess[i]; }
  for (int i = 0; i < 12; ++i) { A.jmin[i] = o.jpos_min[i]; A.jmax[i] = o.jpos_max[i]; }
  A.lbg = d_lbg; A.ubg = d_ubg; A.cost = d_cost; A.x0 = d_x0;
  hipLaunchKernelGGL(landing::landing_kd_pose_kernel, dim3(B), dim3(landing::PL_THREADS), 0, st, A);
  HIP_TRY(hipGetLastError());
  return 0;
}

static int pl_pairs(landing_ctx* ctx, int B, const double* d_p, const double* d_x_kd, const int* d_fin, double* d_in, double* d_out, int* d_index, int* d_count,
                    hipStream_t st) {
  hipLaunchKernelGGL(landing::landing_pl_scan_kernel, dim3(1), dim3(landing::PL_THREADS), 0, st, B, d_fin, d_index, d_count);
  hipLaunchKernelGGL(landing::landing_training_pairs_kernel, dim3(B), dim3(landing::PL_THREADS), 0, st, ctx->L, ctx->L.N, d_p, d_x_kd, (const int*)d_index,
                     (const int*)d_count, d_in, d_out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The whole chain behind the SRBM solutions d_xs (or behind the SRBM solve of d_x0 when that is given).  Call with ctx->pl_mu held and the
// blocks ensured; the stream waits for the previous chain call first.
static int pl_chain(landing_ctx* ctx, int B, const double* d_p, const double* d_x0, const double* d_xs_in, double* d_xs_out, const int* d_srbm_st,
                    const int* d_srbm_it, const landing_pipeline_opts& o, const PlBufs& P, double* d_x, double* d_f, double* d_lam_g, int* d_status,
                    int* d_iters, double* d_kkt, double* d_in, double* d_out, int* d_index, int* d_count, hipStream_t st, const char* who) {
  const Layout& L = ctx->L;
  const int N = L.N;
  // the refinement's parameter set is one per batch: member 0's, checked against every member before anything is solved
  landing_kinodyn_params prm;
  memset(&prm, 0, sizeof(prm));
  double sc[10];      // mu l_leg_max f_max mass | Ib | Ib_inv
  int flag = 0;
  HIP_TRY(hipMemsetAsync(P.flag, 0, sizeof(int), st));
  hipLaunchKernelGGL(landing::landing_pl_check_kernel, dim3((B + landing::PL_THREADS - 1) / landing::PL_THREADS), dim3(landing::PL_THREADS), 0, st, L, B, d_p, P.flag);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(prm.dt, d_p + L.o_dt, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(sc, d_p + L.o_mu, sizeof(sc), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&flag, P.flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (flag) return fail(LANDING_E_ARG, std::string(who) + ": dt, mu, mass, Ib, Ib_inv must be the same for every member of a call");
  prm.mu = sc[0]; prm.mass = sc[3];
  for (int i = 0; i < 3; ++i) { prm.Ib[i] = sc[4 + i]; prm.Ib_inv[i] = sc[7 + i]; }
  const double* xs = d_xs_in;
  if (d_x0) {      // the SRBM pass
    double* xo = d_xs_out ? d_xs_out : P.xs;
    const int rc = landing_solve_batch(ctx, B, d_p, d_x0, &o.srbm, xo, nullptr, nullptr, P.st0, P.it0, nullptr, st);
    if (rc) return rc;
    xs = xo; d_srbm_st = P.st0; d_srbm_it = P.it0;
  }
  { const int rc = pl_pose(ctx, B, d_p, xs, o, P.lbg, P.ubg, P.cost, P.x0, st); if (rc) return rc; }
  const bool warm = o.warm != 0;
  // refinement: straight into the caller's outputs without the re-solve, else into the context's block (the re-solve starts from its x)
  int rc = landing_kinodyn_solve_batch(ctx, B, N, &prm, P.lbg, P.ubg, P.cost, P.x0, &o.refine, warm ? P.x1 : d_x, warm ? P.f1 : d_f,
                                       warm ? (d_lam_g ? P.lam1 : nullptr) : d_lam_g, P.st1, P.it1, warm ? P.kkt1 : d_kkt, st);
  if (rc) return rc;
  if (warm) {
    rc = landing_kinodyn_solve_batch(ctx, B, N, &prm, P.lbg, P.ubg, P.cost, P.x1, &o.resolve, d_x, d_f, d_lam_g, P.st2, P.it2, d_kkt, st);
    if (rc) return rc;
  }
  landing::PlSelectArgs S;
  S.B = B; S.nx = landing::kd_nx(N); S.ng = landing::kd_ng(N); S.warm = warm ? 1 : 0;
  S.st0 = d_srbm_st; S.it0 = d_srbm_it; S.st1 = P.st1; S.it1 = P.it1; S.st2 = P.st2; S.it2 = P.it2;
  S.x1 = P.x1; S.f1 = P.f1; S.lam1 = d_lam_g ? P.lam1 : nullptr; S.kkt1 = P.kkt1;
  S.x = d_x; S.f = d_f; S.lam = d_lam_g; S.kkt = d_kkt; S.status3 = d_status; S.iters3 = d_iters; S.final_st = P.fin;
  hipLaunchKernelGGL(landing::landing_kd_select_kernel, dim3(B), dim3(landing::PL_THREADS), 0, st, S);
  HIP_TRY(hipGetLastError());
  if (d_in) return pl_pairs(ctx, B, d_p, d_x, P.fin, d_in, d_out, d_index, d_count, st);
  return 0;
}

static int pl_run(landing_ctx* ctx, int B, const double* d_p, const double* d_x0, const double* d_xs_in, double* d_xs_out, const int* d_srbm_st,
                  const int* d_srbm_it, const landing_pipeline_opts* opts, double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters,
                  double* d_kkt, double* d_in, double* d_out, int* d_index, int* d_count, void* stream, const char* who) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || !d_p || (!d_x0 && !d_xs_in) || !d_x || !d_f || !d_status || !d_iters || !d_kkt) return fail(LANDING_E_ARG, std::string(who) + ": bad argument");
  const int npair = (d_in != nullptr) + (d_out != nullptr) + (d_index != nullptr) + (d_count != nullptr);
  if (npair != 0 && npair != 4) return fail(LANDING_E_ARG, std::string(who) + ": d_in, d_out, d_index, d_count go together");
  { const int rc = pl_check_ctx(ctx, who, true); if (rc) return rc; }
  HIP_TRY(hipSetDevice(ctx->device));
  landing_pipeline_opts o;
  if (opts) o = *opts; else landing_pipeline_opts_default(&o);
  const hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(ctx->pl_mu);
  PlBufs P;
  { const int rc = pl_ensure(ctx, B, &P); if (rc) return rc; }
  HIP_TRY(hipStreamWaitEvent(st, ctx->pl_done, 0));
  struct Fence { landing_ctx* c; hipStream_t s; ~Fence() { (void)hipEventRecord(c->pl_done, s); } } fence{ctx, st};      // (every exit path: what is queued so far is fenced)
  return pl_chain(ctx, B, d_p, d_x0, d_xs_in, d_xs_out, d_srbm_st, d_srbm_it, o, P, d_x, d_f, d_lam_g, d_status, d_iters, d_kkt, d_in, d_out, d_index, d_count, st, who);
}

extern "C" {

void landing_pipeline_opts_default(landing_pipeline_opts* o) {
  memset(o, 0, sizeof(*o));
  landing_solver_opts_default(&o->srbm);
  landing_kinodyn_solver_opts_default(&o->refine);
  landing_kinodyn_solver_opts_warm(&o->resolve);
  landing_kinodyn_form_knitro(&o->form);      // the chain calls the function generate_landingCtrller_KNITRO.m builds
  const double lo[3] = {-M_PI / 3.0, -M_PI / 2.0, 0.0}, hi[3] = {M_PI / 3.0, M_PI / 2.0, 3.0 * M_PI / 4.0};      // landing_optimization.m:246-247
  for (int i = 0; i < 12; ++i) { o->jpos_min[i] = lo[i % 3]; o->jpos_max[i] = hi[i % 3]; }
  o->jpos_guess[0] = 0.0; o->jpos_guess[1] = -M_PI / 4.0; o->jpos_guess[2] = M_PI / 2.0;      // generate_training_data_automated.m:142
  o->warm = 1;
}

int landing_pipeline_final_status(int refine_status, int resolve_status) { return landing::pl_final_status(refine_status, resolve_status); }

int landing_kinodyn_pose_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x_srbm, const landing_pipeline_opts* opts,
                               double* d_lbg, double* d_ubg, double* d_cost, double* d_x0, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || !d_p || !d_x_srbm || !d_lbg || !d_ubg || !d_cost || !d_x0) return fail(LANDING_E_ARG, "landing_kinodyn_pose_batch: bad argument");
  { const int rc = pl_check_ctx(ctx, "landing_kinodyn_pose_batch", false); if (rc) return rc; }
  HIP_TRY(hipSetDevice(ctx->device));
  landing_pipeline_opts o;
  if (opts) o = *opts; else landing_pipeline_opts_default(&o);
  return pl_pose(ctx, B, d_p, d_x_srbm, o, d_lbg, d_ubg, d_cost, d_x0, (hipStream_t)stream);
}

int landing_training_pairs_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x_kd, const int* d_status_final,
                                 double* d_in, double* d_out, int* d_index, int* d_count, void* stream) {
  if (!ctx || B < 0 || !d_p || !d_x_kd || !d_status_final || !d_in || !d_out || !d_index || !d_count) return fail(LANDING_E_ARG, "landing_training_pairs_batch: bad argument");
  { const int rc = pl_check_ctx(ctx, "landing_training_pairs_batch", false); if (rc) return rc; }
  HIP_TRY(hipSetDevice(ctx->device));
  if (B == 0) { HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(int), (hipStream_t)stream)); return 0; }
  return pl_pairs(ctx, B, d_p, d_x_kd, d_status_final, d_in, d_out, d_index, d_count, (hipStream_t)stream);
}

int landing_pipeline_refine_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x_srbm, const int* d_srbm_status, const int* d_srbm_iters,
                                  const landing_pipeline_opts* opts, double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters, double* d_kkt,
                                  double* d_in, double* d_out, int* d_index, int* d_count, void* stream) {
  if (ctx && B > 0 && !d_x_srbm) return fail(LANDING_E_ARG, "landing_pipeline_refine_batch: bad argument");
  return pl_run(ctx, B, d_p, nullptr, d_x_srbm, nullptr, d_srbm_status, d_srbm_iters, opts, d_x, d_f, d_lam_g, d_status, d_iters, d_kkt, d_in, d_out, d_index,
                d_count, stream, "landing_pipeline_refine_batch");
}

int landing_pipeline_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x0, const landing_pipeline_opts* opts, double* d_x_srbm,
                           double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters, double* d_kkt,
                           double* d_in, double* d_out, int* d_index, int* d_count, void* stream) {
  if (ctx && B > 0 && !d_x0) return fail(LANDING_E_ARG, "landing_pipeline_batch: bad argument");
  return pl_run(ctx, B, d_p, d_x0, nullptr, d_x_srbm, nullptr, nullptr, opts, d_x, d_f, d_lam_g, d_status, d_iters, d_kkt, d_in, d_out, d_index, d_count, stream,
                "landing_pipeline_batch");
}

int landing_pipeline_21(landing_ctx* ctx, int B, const double* Xref, const double* Uref, const double* dt,
                        const double* q_min, const double* q_max, const double* qd_min, const double* qd_max,
                        const double* q_init, const double* qd_init, const double* q_term_min, const double* q_term_max,
                        const double* qd_term_min, const double* qd_term_max, const double* QN, const double* x0,
                        const double* mu, const double* l_leg_max, const double* f_max, const double* mass,
                        const double* Ib, const double* Ib_inv, const landing_pipeline_opts* opts,
                        double* x, double* f, double* lam_g, int* status, int* iters, double* kkt, double* pair_in, double* pair_out, int* n_kept) {
  if (!ctx || B <= 0 || !x0 || !x || !status) return fail(LANDING_E_ARG, "landing_pipeline_21: bad argument");
  { const int rc = pl_check_ctx(ctx, "landing_pipeline_21", true); if (rc) return rc; }
  const landing_args21 a = {Xref, Uref, dt, q_min, q_max, qd_min, qd_max, q_init, qd_init, q_term_min, q_term_max,
                            qd_term_min, qd_term_max, QN, x0, mu, l_leg_max, f_max, mass, Ib, Ib_inv};
  const Layout& L = ctx->L;
  const size_t b = (size_t)B, nxk = (size_t)landing::kd_nx(L.N), ng = (size_t)landing::kd_ng(L.N);
  std::vector<double> p(b * L.np);
  { const int rc = landing_pack_args21(L.N, B, &a, p.data()); if (rc) return rc; }
  HIP_TRY(hipSetDevice(ctx->device));
  Staging st(nullptr);
  const double* d_p = st.in(p.data(), p.size()); const double* d_x0 = st.in(x0, b * L.nx);
  double* d_x = st.out(x, b * nxk); double* d_f = st.out_always(f, b); double* d_kkt = st.out_always(kkt, 3 * b); double* d_lam = st.out(lam_g, b * ng);
  double* d_in = st.block<double>(9 * b); double* d_out = st.block<double>(b * nxk);      // (the first `kept` rows are the caller's: read below)
  int* d_st = st.out(status, 3 * b); int* d_it = st.out_always(iters, 3 * b); int* d_idx = st.block<int>(b + 1);
  HIP_TRY(st.error());
  if (const int rc = landing_pipeline_batch(ctx, B, d_p, d_x0, opts, nullptr, d_x, d_f, d_lam, d_st, d_it, d_kkt, d_in, d_out, d_idx, d_idx + B, nullptr)) return rc;
  HIP_TRY(st.fetch());
  int kept = 0;
  HIP_TRY(st.pull(&kept, d_idx + B, 1));
  if (pair_in && kept) HIP_TRY(st.pull(pair_in, d_in, 9 * (size_t)kept));
  if (pair_out && kept) HIP_TRY(st.pull(pair_out, d_out, (size_t)kept * nxk));
  if (n_kept) *n_kept = kept;
  return 0;
}

int landing_pipeline_21_on(int device, int N, int B, const double* Xref, const double* Uref, const double* dt,
                           const double* q_min, const double* q_max, const double* qd_min, const double* qd_max,
                           const double* q_init, const double* qd_init, const double* q_term_min, const double* q_term_max,
                           const double* qd_term_min, const double* qd_term_max, const double* QN, const double* x0,
                           const double* mu, const double* l_leg_max, const double* f_max, const double* mass,
                           const double* Ib, const double* Ib_inv, const landing_pipeline_opts* opts,
                           double* x, double* f, double* lam_g, int* status, int* iters, double* kkt, double* pair_in, double* pair_out, int* n_kept) {
  if (N < 2 || N > 64) return fail(LANDING_E_ARG, "landing_pipeline_21_on: the refinement takes 2 <= N <= 64 intervals");
  landing_ctx* ctx;
  if (const int rc = cached_mc3d_ctx(N, device, &ctx)) return rc;      // (kd_capi.inc: the context landing_solve_kinodyn_24_on uses for this N and device)
  return landing_pipeline_21(ctx, B, Xref, Uref, dt, q_min, q_max, qd_min, qd_max, q_init, qd_init, q_term_min, q_term_max, qd_term_min, qd_term_max, QN, x0,
                             mu, l_leg_max, f_max, mass, Ib, Ib_inv, opts, x, f, lam_g, status, iters, kkt, pair_in, pair_out, n_kept);
}

}  // extern "C"
