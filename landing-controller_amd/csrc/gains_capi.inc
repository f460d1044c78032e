// gains_capi.inc -- tracking gains straight from a solved batch (included by capi.hip; kernels in vbl_kernels.hip, the Riccati launch in
// solver_capi.inc).  landing_sample_reference_kernel puts the solutions onto the controller's uniform grid, landing_rde_kernel runs behind it on
// the same stream; the host reads nothing in between.

namespace {
struct GainsIn { int B, n; const double *d_x, *d_p; double dt_r; };
}  // namespace

static int gains_check(const landing_ctx* ctx, const char* who, const GainsIn& g, bool any_out) {
  const std::string w(who);
  if (!ctx || g.B < 0) return fail(LANDING_E_ARG, w + ": bad argument");
  if (!g.d_x || !g.d_p) return fail(LANDING_E_ARG, w + ": x and p are required");
  if (g.n < 2) return fail(LANDING_E_ARG, w + ": the grid needs n >= 2 points");
  if (!(g.dt_r > 0.0)) return fail(LANDING_E_ARG, w + ": dt_r must be positive");
  if (!any_out) return fail(LANDING_E_ARG, w + ": no output requested");
  if (ctx->L.N > landing::SR_NMAX) return fail(LANDING_E_ARG, w + ": the resampler takes N <= 96 intervals");
  return 0;
}

static int gains_sample(landing_ctx* ctx, const GainsIn& g, const int* d_status, double* d_xref, double* d_fref, hipStream_t st) {
  const Layout& L = ctx->L;
  landing::SampleArgs a;
  a.B = g.B; a.N = L.N; a.n = g.n; a.nx = L.nx; a.np = L.np; a.o_dt = L.o_dt; a.dt_r = g.dt_r;
  a.x = g.d_x; a.p = g.d_p; a.status = d_status; a.xref = d_xref; a.fref = d_fref;
  const size_t total = (size_t)g.B * g.n;
  hipLaunchKernelGGL(landing::landing_sample_reference_kernel, dim3((unsigned)((total + landing::SR_THREADS - 1) / landing::SR_THREADS)), dim3(landing::SR_THREADS), 0, st, a);
  HIP_TRY(hipGetLastError());
  return 0;
}

extern "C" {

int landing_sample_reference_batch(landing_ctx* ctx, int B, const double* d_x, const double* d_p, double dt_r, int n,
                                   double* d_xref, double* d_fref, void* stream) {
  const GainsIn g{B, n, d_x, d_p, dt_r};
  if (const int rc = gains_check(ctx, "landing_sample_reference_batch", g, d_xref || d_fref)) return rc;
  if (B == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  return gains_sample(ctx, g, nullptr, d_xref, d_fref, (hipStream_t)stream);
}

int landing_tracking_gains_batch(landing_ctx* ctx, int B, const double* d_x, const double* d_p, const int* d_status,
                                 double dt_r, int n, const double* Ib3x3, double mass, const double* Q, const double* r_diag, const double* F, int rk4,
                                 double* d_P, double* d_K, double* d_A, double* d_B, double* d_xref, double* d_fref, void* stream) {
  const char* who = "landing_tracking_gains_batch";
  const GainsIn g{B, n, d_x, d_p, dt_r};
  if (const int rc = gains_check(ctx, who, g, d_P || d_K || d_A || d_B || d_xref || d_fref)) return rc;
  landing::RdeArgs a;
  a.B = B; a.n = n; a.rk4 = rk4 ? 1 : 0; a.dt = dt_r; a.P = d_P; a.K = d_K; a.Aout = d_A; a.Bout = d_B; a.status = d_status;
  if (const int rc = vbl_model(who, Ib3x3, mass, Q, r_diag, a)) return rc;
  if (B == 0) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  const hipStream_t st = (hipStream_t)stream;
  const size_t pts = (size_t)B * n;
  if (!d_P && !d_K && !d_A && !d_B) return gains_sample(ctx, g, d_status, d_xref, d_fref, st);      // only the reference is wanted
  std::lock_guard<std::mutex> lock(ctx->mu);
  if (!d_xref || !d_fref) {
    HIP_TRY(ctx->d_gref.grow(pts * 36));      // hipFree waits for the device: no launch still reads the old block
    HIP_TRY(scratch_acquire(ctx, st));        // ... and the previous call's Riccati kernel (any stream) may still read this one
    if (!d_xref) d_xref = ctx->d_gref.get();
    if (!d_fref) d_fref = ctx->d_gref.get() + pts * 24;
  }
  if (const int rc = gains_sample(ctx, g, d_status, d_xref, d_fref, st)) return rc;
  a.xref = d_xref; a.fref = d_fref;
  return vbl_launch(ctx, a, Q, r_diag, F, st);      // (records the scratch fence behind the Riccati kernel)
}

// Host-pointer twin (FFI callers): x [B][nx], p [B][np], status [B] or NULL in; any of P [B][n][576], K [B][n][288], A [B][n][576], Bm [B][n][288],
// xref [B][n][24], fref [B][n][12] out.  Copies and launches go to the context's own stream, as in landing_solve_batch_host.
int landing_tracking_gains_host(landing_ctx* ctx, int B, const double* x, const double* p, const int* status,
                                double dt_r, int n, const double* Ib3x3, double mass, const double* Q, const double* r_diag, const double* F, int rk4,
                                double* P, double* K, double* A, double* Bm, double* xref, double* fref) {
  const char* who = "landing_tracking_gains_host";
  if (!ctx || B <= 0) return fail(LANDING_E_ARG, std::string(who) + ": bad argument");
  const GainsIn g{B, n, x, p, dt_r};
  if (const int rc = gains_check(ctx, who, g, P || K || A || Bm || xref || fref)) return rc;
  { landing::RdeArgs a; if (const int rc = vbl_model(who, Ib3x3, mass, Q, r_diag, a)) return rc; }      // (argument errors before any allocation)
  const Layout& L = ctx->L;
  HIP_TRY(hipSetDevice(ctx->device));
  { std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->host_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->host_stream, hipStreamNonBlocking)); }
  hipStream_t hs = ctx->host_stream;
  const size_t b = (size_t)B, pts = b * n;
  Staging st(hs);
  const double* dx = st.in(x, b * L.nx); const double* dp = st.in(p, b * L.np); const int* ds = st.in(status, b);
  double* dP = st.out(P, pts * 576); double* dK = st.out(K, pts * 288); double* dA = st.out(A, pts * 576); double* dB = st.out(Bm, pts * 288);
  double* dxr = st.out(xref, pts * 24); double* dfr = st.out(fref, pts * 12);
  HIP_TRY(st.error());
  if (const int rc = landing_tracking_gains_batch(ctx, B, dx, dp, ds, dt_r, n, Ib3x3, mass, Q, r_diag, F, rk4, dP, dK, dA, dB, dxr, dfr, hs)) return rc;      // (st drains the stream)
  HIP_TRY(st.fetch());
  return 0;
}

}  // extern "C"
