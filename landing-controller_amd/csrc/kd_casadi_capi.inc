// kd_casadi_capi.inc -- the CasADi-external face of the kinodynamic refinement NLP (VERDICT r4 item 7 / r5 item 4).
//
// The reference generates this NLP's external library and loads it back through CasADi (generate_solver/generate_landingCtrller_KNITRO.m:360-377:
// opti.to_function + nlpsol('solver', 'knitro', './landingCtrller_KNITRO.so')); its generated artefacts are missing blobs (.MISSING_LARGE_BLOBS:1-4), so the
// interface is rebuilt from the rules that produced the IPOPT variant's library, which IS in the tree and was checked line by line in round 1:
//   * x = [X(:) 12 x (N+1); jpos(:) 12 x N; U(:) 24 x N]  (declaration order, :40-46) -- the order landing_kinodyn_nlp_eval already uses;
//   * p = the ACTIVE Opti parameters in declaration order (:51-82; SURVEY row a2 verified the rule on landingCtrller_IPOPT.c: np 354 = 252 + 20 + 82 there):
//       Xref 12(N+1) | dt N | q_init 6 | qd_init 6 | c_init 12 | jpos_min 12 | jpos_max 12 | q_term_min 6 | q_term_max 6 | qd_term_min 6 | qd_term_max 6 |
//       q_min 6 | QN 12 | mu | l_leg_max | mass | Ib 3 | Ib_inv 3 | kin_box 2          np = 13 N + 113  (373 at the script's N = 20 intervals)
//     Uref is declared and never used; q_max, qd_min, qd_max are declared and never used (only q_min(3) is bounded, :181): dropped like Uref of the IPOPT variant;
//   * g in Opti's canonical form (optistack_internal.cpp:742-856): the rows of landing_kinodyn_nlp_eval (round 6: the `>=` friction rows as -km f_z - f_xy);
//     parameters enter g through dt, mass, Ib, Ib_inv, mu only -- every other parameter sits in lbg / ubg (landing_kinodyn_casadi_bounds);
//   * f = sum_i QN_i (X_i,N+1 - Xref_i,N+1)^2  (:84-87);
//   * CCS patterns of jac_g_x and triu(hess_gamma_x_x) = landing_kinodyn_pattern (structural, from the derivative kernels); multiplier sign as CasADi's.
// One problem per call, host arrays, every output optional (res[i] == NULL); derivatives are the exact ones of the function layer (dual / hyper-dual numbers);
// grad_gamma_p: closed form for Xref(:, end) and QN, central differences of lam' g for dt, mass, Ib, Ib_inv, mu (g is linear in all of them but mass).
namespace {
struct KdCasadi {
  int N = 0;
  std::vector<long long> jc, jr, hc, hr;            // CCS patterns
  std::vector<int> jsrc;                            // Jacobian nonzero -> index into the block array [N][141][72], or -1: the constant 1 of a boundary row
  std::vector<std::array<int, 2>> hsrc;             // Hessian nonzero -> up to two entries of the block array [N][72][72] (shared X_k+1 / c_k+1 pairs), -1: none
  std::vector<int> hterm;                           // ... and the index i of the terminal-cost diagonal 2 QN_i, or -1
  DevBuf<double> d_x, d_l, d_g, d_j, d_h;
};
void KdCasadiFree::operator()(KdCasadi* k) const { delete k; }
}  // namespace

extern "C" {

long long landing_kinodyn_casadi_np(int N) { return 13LL * N + 113; }

// offsets inside p (host helper of the bindings): [Xref, dt, q_init, qd_init, c_init, jpos_min, jpos_max, q_term_min, q_term_max, qd_term_min, qd_term_max, q_min, QN, mu, l_leg_max, mass, Ib, Ib_inv, kin_box]
int landing_kinodyn_casadi_offsets(int N, long long off[19]) {
  if (N < 2 || N > 64 || !off) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_offsets: bad argument");
  const int len[19] = {12 * (N + 1), N, 6, 6, 12, 12, 12, 6, 6, 6, 6, 6, 12, 1, 1, 1, 3, 3, 2};
  long long o = 0;
  for (int i = 0; i < 19; ++i) { off[i] = o; o += len[i]; }
  return 0;
}

// lbg / ubg of ONE problem from p -- what the serialized CasADi function evaluates as MX expressions of p (Opti keeps the bounds outside the external library)
int landing_kinodyn_casadi_bounds(int N, const landing_kinodyn_form* form, const double* p, double* lbg, double* ubg) {
  long long o[19];
  if (!p || !lbg || !ubg || landing_kinodyn_casadi_offsets(N, o)) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_bounds: bad argument");
  return landing_kinodyn_bounds(N, 1, form, p + o[2], p + o[3], p + o[4], p + o[11], p + o[7], p + o[8], p + o[9], p + o[10], p + o[5], p + o[6], p + o[18], p + o[14], lbg, ubg);
}

int landing_kinodyn_casadi_pattern(landing_ctx* ctx, int N, int which, const long long** colind, const long long** row, long long* nnz);

// the context's cache for horizon N, built at the first call
static KdCasadi* kdc_get(landing_ctx* ctx, int N) {
  std::lock_guard<std::mutex> lk(ctx->kdc_mu);
  auto it = ctx->kdc.find(N);
  if (it != ctx->kdc.end()) return it->second.get();
  std::unique_ptr<KdCasadi, KdCasadiFree> K(new KdCasadi());
  K->N = N;
  const int nx = landing::kd_nx(N), ng = landing::kd_ng(N), NW = landing::KD_NW, NR = landing::KD_ROWS;
  for (int which = 0; which < 2; ++which) {
    std::vector<long long>& c = which ? K->hc : K->jc; std::vector<long long>& r = which ? K->hr : K->jr;
    c.assign(nx + 1, 0);
    long long nnz = 0;
    if (landing_kinodyn_pattern(ctx, N, which, c.data(), nullptr, &nnz)) return nullptr;
    r.assign((size_t)nnz, 0);
    if (landing_kinodyn_pattern(ctx, N, which, c.data(), r.data(), &nnz)) return nullptr;
  }
  // inverse of kd_w_index per interval: x index -> block column
  std::vector<std::vector<int>> inv(N, std::vector<int>(nx, -1));
  for (int k = 0; k < N; ++k) for (int j = 0; j < NW; ++j) { const int xi = landing::kd_w_index(N, k, j); if (xi >= 0) inv[k][xi] = j; }
  K->jsrc.assign(K->jr.size(), -1);
  for (int c = 0; c < nx; ++c) for (long long q = K->jc[c]; q < K->jc[c + 1]; ++q) {
    const long long r = K->jr[q];
    if (r < landing::KD_BND) continue;                                   // boundary rows: coordinate picks
    const int k = (int)((r - landing::KD_BND) / NR), rr = (int)((r - landing::KD_BND) % NR), j = inv[k][c];
    if (j < 0) { fail(LANDING_E_ARG, "landing_kinodyn_casadi: pattern entry outside its block"); return nullptr; }
    K->jsrc[q] = (k * NR + rr) * NW + j;
  }
  K->hsrc.assign(K->hr.size(), std::array<int, 2>{-1, -1}); K->hterm.assign(K->hr.size(), -1);
  for (int c = 0; c < nx; ++c) for (long long q = K->hc[c]; q < K->hc[c + 1]; ++q) {
    const int lo = (int)K->hr[q], hi = c; int n = 0;
    for (int k = 0; k < N; ++k) { const int a = inv[k][lo], b = inv[k][hi]; if (a >= 0 && b >= 0 && n < 2) K->hsrc[q][n++] = (k * NW + a) * NW + b; }
    if (lo == hi && lo >= 12 * N && lo < 12 * (N + 1)) K->hterm[q] = lo - 12 * N;
  }
  if (hipSetDevice(ctx->device) != hipSuccess || K->d_x.alloc((size_t)nx) != hipSuccess || K->d_l.alloc((size_t)ng) != hipSuccess ||
      K->d_g.alloc((size_t)ng) != hipSuccess || K->d_j.alloc((size_t)N * NR * NW) != hipSuccess || K->d_h.alloc((size_t)N * NW * NW) != hipSuccess) {
    fail(LANDING_E_HIP, "landing_kinodyn_casadi: hipMalloc"); return nullptr;
  }
  KdCasadi* raw = K.get();
  ctx->kdc[N] = std::move(K);
  return raw;
}

void landing_kinodyn_casadi_release(landing_ctx* ctx) {      // drops the context's cache now (landing_destroy drops it too)
  if (!ctx) return;
  std::lock_guard<std::mutex> lk(ctx->kdc_mu);
  ctx->kdc.clear();
}

int landing_kinodyn_casadi_pattern(landing_ctx* ctx, int N, int which, const long long** colind, const long long** row, long long* nnz) {
  if (!ctx || N < 2 || N > 64 || which < 0 || which > 1) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_pattern: bad argument");
  KdCasadi* K = kdc_get(ctx, N);
  if (!K) return LANDING_E_HIP;
  if (colind) *colind = (which ? K->hc : K->jc).data();
  if (row) *row = (which ? K->hr : K->jr).data();
  if (nnz) *nnz = (long long)(which ? K->hr : K->jr).size();
  return 0;
}

int landing_kinodyn_casadi_eval_host(landing_ctx* ctx, int N, const double* x, const double* p, const double* lam_f, const double* lam_g,
                                     double* f, double* g, double* grad_f, double* jac, double* hess, double* ggx, double* ggp) {
  if (!ctx || N < 2 || N > 64 || !x || !p) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_eval_host: bad argument");
  if ((hess || ggx || ggp) && !lam_g) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_eval_host: lam_g needed");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_casadi_eval_host: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_casadi_eval_host")) return rc;
  KdCasadi* K = kdc_get(ctx, N);
  if (!K) return LANDING_E_HIP;
  long long o[19];
  (void)landing_kinodyn_casadi_offsets(N, o);
  const int nx = landing::kd_nx(N), ng = landing::kd_ng(N), NW = landing::KD_NW, NR = landing::KD_ROWS;
  const long long np = landing_kinodyn_casadi_np(N);
  const double lf = lam_f ? *lam_f : 1.0;
  const double* Xref_end = p + o[0] + 12 * N; const double* QN = p + o[12];
  landing_kinodyn_params prm;
  memset(&prm, 0, sizeof(prm));
  auto set_prm = [&](const double* q) {
    for (int k = 0; k < N; ++k) prm.dt[k] = q[o[1] + k];
    prm.mu = q[o[13]]; prm.mass = q[o[15]];
    for (int i = 0; i < 3; ++i) { prm.Ib[i] = q[o[16] + i]; prm.Ib_inv[i] = q[o[17] + i]; }
  };
  set_prm(p);
  // objective
  double fv = 0.0;
  for (int i = 0; i < 12; ++i) { const double d = x[12 * N + i] - Xref_end[i]; fv += QN[i] * d * d; }
  if (f) *f = fv;
  if (grad_f) { for (int i = 0; i < nx; ++i) grad_f[i] = 0.0; for (int i = 0; i < 12; ++i) grad_f[12 * N + i] = 2.0 * QN[i] * (x[12 * N + i] - Xref_end[i]); }
  if (!g && !jac && !hess && !ggx && !ggp) return 0;
  HIP_TRY(hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lk(ctx->kdc_mu);      // the device buffers of K are used by one call at a time (CasADi calls sequentially from IPOPT's / KNITRO's thread)
  HIP_TRY(hipMemcpy(K->d_x.get(), x, (size_t)nx * sizeof(double), hipMemcpyHostToDevice));
  const bool need_j = jac || ggx;
  { const int rc = landing_kinodyn_nlp_eval(ctx, 1, N, K->d_x.get(), &prm, g ? K->d_g.get() : nullptr, need_j ? K->d_j.get() : nullptr, nullptr); if ((g || need_j) && rc) return rc; }
  std::vector<double> blk;
  if (need_j) { blk.resize((size_t)N * NR * NW); HIP_TRY(hipMemcpy(blk.data(), K->d_j.get(), blk.size() * sizeof(double), hipMemcpyDeviceToHost)); }
  if (g) HIP_TRY(hipMemcpy(g, K->d_g.get(), (size_t)ng * sizeof(double), hipMemcpyDeviceToHost));
  if (jac) for (size_t q = 0; q < K->jr.size(); ++q) jac[q] = K->jsrc[q] < 0 ? 1.0 : blk[K->jsrc[q]];
  if (ggx) {      // lam_f grad f + J' lam
    for (int i = 0; i < nx; ++i) ggx[i] = 0.0;
    for (int i = 0; i < 12; ++i) ggx[12 * N + i] = lf * 2.0 * QN[i] * (x[12 * N + i] - Xref_end[i]);
    for (int c = 0; c < nx; ++c) { double a = 0.0; for (long long q = K->jc[c]; q < K->jc[c + 1]; ++q) a += (K->jsrc[q] < 0 ? 1.0 : blk[K->jsrc[q]]) * lam_g[K->jr[q]]; ggx[c] += a; }
  }
  if (hess) {
    HIP_TRY(hipMemcpy(K->d_l.get(), lam_g, (size_t)ng * sizeof(double), hipMemcpyHostToDevice));
    { const int rc = landing_kinodyn_nlp_hess(ctx, 1, N, K->d_x.get(), &prm, K->d_l.get(), K->d_h.get(), nullptr); if (rc) return rc; }
    std::vector<double> hb((size_t)N * NW * NW);
    HIP_TRY(hipMemcpy(hb.data(), K->d_h.get(), hb.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t q = 0; q < K->hr.size(); ++q) {
      double v = 0.0;
      for (int n = 0; n < 2; ++n) if (K->hsrc[q][n] >= 0) v += hb[K->hsrc[q][n]];
      if (K->hterm[q] >= 0) v += lf * 2.0 * QN[K->hterm[q]];
      hess[q] = v;
    }
  }
  if (ggp) {
    for (long long i = 0; i < np; ++i) ggp[i] = 0.0;
    for (int i = 0; i < 12; ++i) { const double d = x[12 * N + i] - Xref_end[i]; ggp[o[0] + 12 * N + i] = -lf * 2.0 * QN[i] * d; ggp[o[12] + i] = lf * d * d; }
    // d(lam' g)/dp for the parameters inside g: central differences (g is linear in dt, Ib, Ib_inv, mu; 1 / mass enters rddot)
    std::vector<long long> idx;
    for (int k = 0; k < N; ++k) idx.push_back(o[1] + k);
    idx.push_back(o[13]); idx.push_back(o[15]);
    for (int i = 0; i < 3; ++i) { idx.push_back(o[16] + i); idx.push_back(o[17] + i); }
    std::vector<double> pp(p, p + np), gp(ng), gm(ng);
    for (long long ip : idx) {
      const double h = 1e-4 * fmax(1e-2, fabs(p[ip]));
      for (int s = 0; s < 2; ++s) {
        pp[ip] = p[ip] + (s ? -h : h);
        set_prm(pp.data());
        { const int rc = landing_kinodyn_nlp_eval(ctx, 1, N, K->d_x.get(), &prm, K->d_g.get(), nullptr, nullptr); if (rc) return rc; }
        HIP_TRY(hipMemcpy((s ? gm : gp).data(), K->d_g.get(), (size_t)ng * sizeof(double), hipMemcpyDeviceToHost));
      }
      pp[ip] = p[ip];
      double a = 0.0;
      for (int r = 0; r < ng; ++r) a += lam_g[r] * (gp[r] - gm[r]);
      ggp[ip] = a / (2.0 * h);
    }
  }
  return 0;
}

}  // extern "C"
