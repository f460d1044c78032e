// kd_capi.inc -- host side of the kinodynamic refinement solve (included by capi.hip; kernels in kd_solver_kernels.hip, function layer in
// rbd_kernels.hip).  The interior-point loop runs here, one round of launches per iteration for the whole batch (members that have finished
// are skipped by every kernel); the only host <-> device traffic inside the loop is the 4-byte count of members still iterating.

extern "C" {

// The two derivative kernels of the kinodynamic NLP exist in two forms (rbd_kernels.hip kd_stage_rows): with the base transform of the tree taken from R and pos (the
// floating base Px Py Pz Rx Ry Rz of the reference's model -- landing_rbd_set_model checks it) or composed joint by joint
static void kd_launch_jac(landing_ctx* ctx, const landing::KdNlpArgs& a, long long B, int N, hipStream_t st) {
  const dim3 grid((unsigned)landing::kd_jac_blocks(B, N)), block(landing::KD_JAC_THREADS);
  if (ctx->rbd_std_base) hipLaunchKernelGGL(landing::landing_kinodyn_nlp_jac_kernel<1>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(landing::landing_kinodyn_nlp_jac_kernel<0>, grid, block, 0, st, a);
}
static void kd_launch_hess(landing_ctx* ctx, const landing::KdNlpArgs& a, long long B, int N, const unsigned char* pi, const unsigned char* pj, int npair, hipStream_t st) {
  const dim3 grid((unsigned)landing::kd_hess_blocks(B, N, npair)), block(64);
  if (ctx->rbd_std_base) hipLaunchKernelGGL(landing::landing_kinodyn_nlp_hess_kernel<1>, grid, block, 0, st, a, pi, pj, npair);
  else hipLaunchKernelGGL(landing::landing_kinodyn_nlp_hess_kernel<0>, grid, block, 0, st, a, pi, pj, npair);
}

// The constants of a call in the kernels' form: dt padded to its 64 slots, the base form from the context's model
static landing::KdNlpParams kd_params(const landing_ctx* ctx, const landing_kinodyn_params* prm, int N) {
  landing::KdNlpParams P;
  for (int k = 0; k < 64; ++k) P.dt[k] = k < N ? prm->dt[k] : 0.0;
  P.mass = prm->mass; P.mu = prm->mu; P.std_base = ctx->rbd_std_base;
  for (int i = 0; i < 3; ++i) { P.Ib[i] = prm->Ib[i]; P.Ibi[i] = prm->Ib_inv[i]; }
  return P;
}
// The constants of the structure probes below.  The structure must not depend on a caller's parameter VALUES (ADVICE r5: with Ib = (0.03, 0.03, 0.03) the omega-omega entries
// of omega x I omega vanish and a later call with the real inertia got 36 wrong zeros): fixed generic ones -- distinct inertias, mu > 0, unit mass, a uniform grid -- so that
// only the model (landing_rbd_set_model invalidates the tables) and the formulation decide what is kept.
static landing::KdNlpParams kd_probe_params(const landing_ctx* ctx, int N) {
  landing_kinodyn_params prm;
  for (int k = 0; k < 64; ++k) prm.dt[k] = 0.03;
  prm.mass = 1.0; prm.mu = 0.7; prm.Ib[0] = 0.05; prm.Ib[1] = 0.2; prm.Ib[2] = 0.3; prm.Ib_inv[0] = 17.0; prm.Ib_inv[1] = 4.3; prm.Ib_inv[2] = 3.6;
  return kd_params(ctx, &prm, N);
}
// Arguments of the function-layer kernels for B members of N intervals: the model and the sizes; dense strides, no array, no list
static landing::KdNlpArgs kd_nlp_args(const landing_ctx* ctx, int B, int N) {
  landing::KdNlpArgs a{};
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N;
  return a;
}
// The probes' random points: uniform in [0, 1) from a 64-bit linear congruential generator
struct KdRand {
  unsigned long long s;
  double operator()() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)((s >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0; }
};

int landing_kinodyn_nlp_dims(int N, long long* nx, long long* ng) {
  if (N < 2 || N > 64) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_dims: 2 <= N <= 64");
  if (nx) *nx = landing::kd_nx(N);
  if (ng) *ng = landing::kd_ng(N);
  return 0;
}

int landing_kinodyn_nlp_eval(landing_ctx* ctx, int B, int N, const double* d_x, const landing_kinodyn_params* prm, double* d_g, double* d_jac, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 2 || N > 64 || !d_x || !prm || (!d_g && !d_jac)) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_eval: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_eval: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_nlp_eval")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::KdNlpArgs a = kd_nlp_args(ctx, B, N);
  a.P = kd_params(ctx, prm, N); a.x = d_x; a.g = d_g; a.jac = d_jac;
  if (d_g) {
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(landing::landing_kinodyn_nlp_g_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  }
  if (d_jac) kd_launch_jac(ctx, a, B, N, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

// The pairs (i <= j) of a Hessian block of the kinodynamic NLP that are evaluated: kd_pair_list's 561 candidates (one leg's variables couple with
// themselves and the base only, ...) thinned out to those whose entry is not structurally zero.  Which those are is asked of the derivative kernel
// itself, once per context (round 5): the candidates are evaluated on a few members with random variables and multipliers (three intervals: two
// middle ones and a last one) and a pair is kept when its entry is non-zero anywhere -- a mixed second derivative through hyper-dual numbers is
// exactly 0.0 when no row couples the two variables (friction and contact rows are linear in the forces, the FK band is linear in the feet and the
// body position, omega x I omega has no squares, ...).  286 of the 561 remain; tests/test_n1_rows.py checks EVERY column of the blocks against
// central differences of the exact Jacobian, which also proves this list.  Caller holds ctx->mu.
static int kd_ensure_pairs(landing_ctx* ctx) {
  if (ctx->d_kd_pairs) return 0;
  const int NP = landing::KD_NPAIR;
  unsigned char host[2 * landing::KD_NPAIR];
  if (landing::kd_pair_list(host, host + NP) != NP) return fail(LANDING_E_ARG, "kinodynamic NLP: internal pair table");
  const int B = 6, N = 3, NW = landing::KD_NW;
  const size_t nx = (size_t)landing::kd_nx(N), ng = (size_t)landing::kd_ng(N), nh = (size_t)B * N * NW * NW;
  std::vector<double> hx(B * nx), hl(B * ng), hh(nh);
  KdRand rnd{0x9E3779B97F4A7C15ull};
  for (auto& v : hx) v = rnd() - 0.5;
  for (auto& v : hl) v = (0.5 + rnd()) * (rnd() < 0.5 ? -1.0 : 1.0);
  Staging st(nullptr);
  const unsigned char* d_full = st.in(host, sizeof(host));
  landing::KdNlpArgs a = kd_nlp_args(ctx, B, N);
  a.P = kd_probe_params(ctx, N); a.x = st.in(hx.data(), hx.size()); a.lam = st.in(hl.data(), hl.size()); a.hess = st.out(hh.data(), nh);
  HIP_TRY(st.error());
  HIP_TRY(hipMemset(a.hess, 0, nh * sizeof(double)));
  kd_launch_hess(ctx, a, B, N, d_full, d_full + NP, NP, (hipStream_t)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(st.fetch());
  unsigned char keep[2 * landing::KD_NPAIR]; int nk = 0;
  for (int q = 0; q < NP; ++q) {
    const int i = host[q], j = host[NP + q];
    bool nz = false;
    for (int b = 0; b < B && !nz; ++b) for (int k = 0; k < N && !nz; ++k) { const double v = hh[(((size_t)b * N + k) * NW + i) * NW + j]; nz = v != 0.0 || v != v; }
    if (nz) { keep[nk] = (unsigned char)i; keep[NP + nk] = (unsigned char)j; ++nk; }
  }
  if (nk < 1) return fail(LANDING_E_ARG, "kinodynamic NLP: empty pair table");
  // Wavefront-pure order: a lane's pair decides which legs' kinematic rows it evaluates (kd_stage_rows' legmask: all four for a pair inside the base, one for a pair
  // that involves a leg), and a wavefront runs the rows of every leg any of its lanes needs.  The pairs of the base fill their own wavefront(s), then leg by leg,
  // each class padded to a multiple of 64 with empty entries (255: the lane leaves at once).
  unsigned char packed[2 * 1024]; int np_ = 0;
  {
    unsigned char oi[1024], oj[1024];
    for (int cls = -1; cls < 4; ++cls) {
      for (int q = 0; q < nk; ++q) if (landing::kd_pair_leg(keep[q], keep[NP + q]) == cls) { oi[np_] = keep[q]; oj[np_] = keep[NP + q]; ++np_; }
      while (np_ % 64) { oi[np_] = 255; oj[np_] = 255; ++np_; }
    }
    for (int q = 0; q < np_; ++q) { packed[q] = oi[q]; packed[np_ + q] = oj[q]; }
  }
  nk = np_;
  DevBuf<unsigned char> d_pairs;
  HIP_TRY(d_pairs.alloc((size_t)2 * nk));
  HIP_TRY(hipMemcpy(d_pairs.get(), packed, (size_t)2 * nk, hipMemcpyHostToDevice));
  ctx->d_kd_pairs = std::move(d_pairs); ctx->kd_npair = nk;
  return 0;
}

// Structural non-zeros of the inequality rows of the kinodynamic NLP's Jacobian blocks (landing::KdJPat, read by the solver's forward sweep: ds = J_I dx over the non-zeros
// only).  Asked of the Jacobian kernel itself, once per context, like the pair table above: random variables on six members of a four-interval problem with fixed generic
// constants; an entry is kept when it is non-zero on any member (a forward-mode derivative is exactly 0.0 where the row does not depend on the variable).  The three
// intervals that are not the last must agree (they do: the rows depend on the interval through dt only).  tests/test_n1_rows.py checks every column of the blocks against
// central differences; tests/test_kd_solver_cpu.py pins the counts (529 / 457).  Caller holds ctx->mu.
static int kd_ensure_jpat(landing_ctx* ctx) {
  if (ctx->d_kd_jpat) return 0;
  const int B = 6, N = 4, NW = landing::KD_NW, NR = landing::KD_ROWS;
  const size_t nx = (size_t)landing::kd_nx(N), nj = (size_t)B * N * NR * NW;
  std::vector<double> hx(B * nx), hj(nj);
  KdRand rnd{0x2545F4914F6CDD1Dull};
  for (auto& v : hx) v = rnd() - 0.4;
  Staging st(nullptr);
  landing::KdNlpArgs a = kd_nlp_args(ctx, B, N);
  a.P = kd_probe_params(ctx, N); a.x = st.in(hx.data(), hx.size()); a.jac = st.out(hj.data(), nj);
  HIP_TRY(st.error());
  HIP_TRY(hipMemset(a.jac, 0, nj * sizeof(double)));
  kd_launch_jac(ctx, a, B, N, (hipStream_t)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(st.fetch());
  auto nz = [&](int k, int r, int c) { for (int b = 0; b < B; ++b) { const double v = hj[(((size_t)b * N + k) * NR + r) * NW + c]; if (v != 0.0 || v != v) return true; } return false; };
  for (int r = 12; r < NR; ++r) for (int c = 0; c < NW; ++c)
    if (nz(0, r, c) != nz(1, r, c) || nz(1, r, c) != nz(2, r, c)) return fail(LANDING_E_ARG, "kinodynamic NLP: the Jacobian blocks of two middle intervals differ in structure");
  std::vector<landing::KdJPat> T(1);
  memset(T.data(), 0, sizeof(landing::KdJPat));
  std::vector<landing::KdCPat> Cp(1);
  memset(Cp.data(), 0, sizeof(landing::KdCPat));
  for (int lp = 0; lp < 2; ++lp) {
    const int k = lp ? N - 1 : 1, nrow = (lp ? landing::KD_ROWS_LAST : NR) - 12;
    std::vector<std::vector<int>> cols(nrow);
    for (int j = 0; j < nrow; ++j) for (int c = 0; c < NW; ++c) if (nz(k, 12 + j, c)) cols[j].push_back(c);
    std::vector<int> order(nrow);
    for (int j = 0; j < nrow; ++j) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int p, int q) { return cols[p].size() > cols[q].size(); });
    int n = 0;
    for (int j = 0; j < nrow; ++j) {
      const std::vector<int>& cj = cols[order[j]];
      if ((int)cj.size() > landing::KD_JP_MAX || n + (int)cj.size() > landing::KD_JP_NNZ - landing::KD_JP_MAX) return fail(LANDING_E_ARG, "kinodynamic NLP: Jacobian block denser than the table of its non-zeros");
      T[0].perm[lp][j] = (unsigned char)(12 + order[j]); T[0].rp[lp][j] = (unsigned short)n;
      for (int c : cj) T[0].cl[lp][n++] = (unsigned char)c;
    }
    T[0].rp[lp][nrow] = (unsigned short)n;
    ctx->kd_jpat_nnz[lp] = n;
    // place table of the compact block (KdNlpArgs::jpos): defect rows dense, inequality entries in table order
    {
      std::vector<std::vector<unsigned>> colv(NW);
      for (int c = 0; c < NW; ++c) for (int r = 0; r < 12; ++r) colv[c].push_back(((unsigned)r << 16) | (unsigned)(r * NW + c));
      for (int j = 0; j < nrow; ++j) for (int t = T[0].rp[lp][j]; t < T[0].rp[lp][j + 1]; ++t) colv[T[0].cl[lp][t]].push_back(((unsigned)T[0].perm[lp][j] << 16) | (unsigned)(landing::KD_JC_DEF + t));
      for (int c = 0; c < NW; ++c) {
        std::sort(colv[c].begin(), colv[c].end());      // (by row: the kernel emits the rows of a column in rising order)
        if ((int)colv[c].size() >= landing::KD_JCOL) return fail(LANDING_E_ARG, "kinodynamic NLP: a column of the Jacobian block has more entries than its list holds");
        for (size_t i = 0; i < colv[c].size(); ++i) Cp[0].jcol[lp][c][i] = colv[c][i];
        for (int i = (int)colv[c].size(); i < landing::KD_JCOL; ++i) Cp[0].jcol[lp][c][i] = 0xffff0000u;
      }
    }
    // the condensation over these entries (landing::KdCPat): stage variable v of block column w (the inequality rows do not see X_k+1, columns 48..59)
    const int nv = lp ? 48 : landing::KD_NV;
    auto vof = [&](int w) { return w < 48 ? w : (w >= 60 ? w - 12 : -1); };
    std::map<std::pair<int, int>, std::vector<unsigned>> dest;
    std::vector<std::vector<unsigned>> rhs(landing::KD_NV);
    for (int j = 0; j < nrow; ++j)
      for (int ta = T[0].rp[lp][j]; ta < T[0].rp[lp][j + 1]; ++ta) {
        Cp[0].erow[lp][ta] = (unsigned char)j;
        const int va = vof(T[0].cl[lp][ta]);
        if (va < 0 || va >= nv) return fail(LANDING_E_ARG, "kinodynamic NLP: an inequality row depends on a variable outside its stage");
        rhs[va].push_back((unsigned)ta | ((unsigned)j << 10));
        for (int tb = T[0].rp[lp][j]; tb < T[0].rp[lp][j + 1]; ++tb) {
          const int vb = vof(T[0].cl[lp][tb]);
          if (vb >= va) dest[{va, vb}].push_back((unsigned)ta | ((unsigned)tb << 10) | ((unsigned)j << 20));
        }
      }
    std::vector<std::pair<std::pair<int, int>, std::vector<unsigned>>> dl(dest.begin(), dest.end());
    std::stable_sort(dl.begin(), dl.end(), [](const auto& p, const auto& q) { return p.second.size() > q.second.size(); });      // lanes of a wavefront: destinations of similar length
    int nd = 0, nt = 0;
    for (const auto& e : dl) {
      if (nd >= landing::KD_CP_ND || nt + (int)e.second.size() > landing::KD_CP_NT) return fail(LANDING_E_ARG, "kinodynamic NLP: condensation table too small");
      Cp[0].drp[lp][nd] = (unsigned short)nt; Cp[0].dab[lp][nd] = (unsigned short)(e.first.first | (e.first.second << 8));
      for (unsigned w : e.second) Cp[0].dterm[lp][nt++] = w;
      ++nd;
    }
    Cp[0].drp[lp][nd] = (unsigned short)nt; Cp[0].nd[lp] = nd; Cp[0].nt[lp] = nt;
    int nr = 0;
    for (int v = 0; v < landing::KD_NV; ++v) { Cp[0].rrp[lp][v] = (unsigned short)nr; for (unsigned w : rhs[v]) Cp[0].rterm[lp][nr++] = w; }
    Cp[0].rrp[lp][landing::KD_NV] = (unsigned short)nr;
  }
  DevBuf<unsigned char> d_t;      // [KdJPat | KdCPat]
  constexpr size_t JP8 = (sizeof(landing::KdJPat) + 15) / 16 * 16;
  HIP_TRY(d_t.alloc(JP8 + sizeof(landing::KdCPat)));
  HIP_TRY(hipMemcpy(d_t.get(), T.data(), sizeof(landing::KdJPat), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_t.get() + JP8, Cp.data(), sizeof(landing::KdCPat), hipMemcpyHostToDevice));
  ctx->kd_cpat_off = JP8;
  ctx->d_kd_jpat = std::move(d_t);
  return 0;
}

int landing_kinodyn_nlp_hess(landing_ctx* ctx, int B, int N, const double* d_x, const landing_kinodyn_params* prm, const double* d_lam_g, double* d_hess, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 2 || N > 64 || !d_x || !prm || !d_lam_g || !d_hess) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_hess: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_hess: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_nlp_hess")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing::KdNlpArgs a = kd_nlp_args(ctx, B, N);
  a.P = kd_params(ctx, prm, N); a.x = d_x; a.lam = d_lam_g; a.hess = d_hess;
  std::lock_guard<std::mutex> lock(ctx->mu);      // (the lazily built table below, like every other lazily created resource of the context)
  { const int rc = kd_ensure_pairs(ctx); if (rc) return rc; }      // the list of structurally non-zero pairs of a block, built once per context
  const long long n = (long long)B * N * ctx->kd_npair;
  if (n > 0x7fffffffLL * 64) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_hess: batch too large for one launch");
  HIP_TRY(hipMemsetAsync(d_hess, 0, (size_t)B * N * landing::KD_NW * landing::KD_NW * sizeof(double), (hipStream_t)stream));
  kd_launch_hess(ctx, a, B, N, ctx->d_kd_pairs.get(), ctx->d_kd_pairs.get() + ctx->kd_npair, ctx->kd_npair, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return 0;
}

// Warm-start preset of the refinement (round 6): every production caller solves this NLP twice, the second time from the first solution (`prevSoln`:
// main_scripts/landing_optimization.m:395-435; generate_solver/generate_landingCtrller_KNITRO_warmstart.m builds the `_ws` function for it).  From a solution the
// slacks of the active rows sit AT their bounds: pushed 1e-6 inside with mu_init = 1e-6 the iteration starts in the last barrier problem instead of walking back
// from mu = 0.1; the cold-start rules (4-slack clip, crawl detector, portfolio) are off.  MI355X, 216 converged members of a 256-member batch re-solved from x*
// (tools/dev/kd_warm_probe.py): push = mu = 1e-3 / 1e-4 / 1e-5 / 1e-6 -> 24.0 / 12.1 / 8.7 / 4.0 iterations on average, median 18 / 8 / 4 / 3, p99 131 / 92 / 82 / 5
// (one member in 216 needs ~110 on every setting); the cold-start defaults: 31.
void landing_kinodyn_solver_opts_warm(landing_solver_opts* o) {
  landing_kinodyn_solver_opts_default(o);
  o->bound_push = 1e-6; o->bound_frac = 1e-6; o->mu_init = 1e-6;
  o->clip_k = 0; o->fresh_restart = 0; o->restart_period = 0; o->jam_clip = 0; o->stag_relief = 0;
  o->kd_clone_after = 0; o->kd_clone_max = 0; o->kd_clone_iter = 0;
  o->max_iter = 100;
}

void landing_kinodyn_solver_opts_default(landing_solver_opts* o) {
  landing_solver_opts_default(o);
  o->max_iter = 500;
  // measured on 1024 drop states of the production sampling law (SRBM solution as the initial guess, MI355X, tools/dev/kd_lab.py): the SRBM
  // solver's slack initialisation (bound_push 0.5) pushes the slacks of the one-sided copies of the +-0.01 FK band half a unit away from
  // their rows (803 of 834 feasible members converge, mean 54 iterations); IPOPT's own defaults 0.01 / 0.01: 831 of 834, mean 43
  o->bound_push = 0.01; o->bound_frac = 0.01;
  o->mu_init = 0.1; o->theta_mu = 1.5;      // the reference's / IPOPT's values (the SRBM solver's automatic choices do not apply here)
  // (kappa_eps stays at the SRBM solver's 80: with these slacks 10 / 80 -> 834 / 834 feasible members both, mean 43.3 / 39.0, slowest 434 / 192 iterations)
  // Feasibility phase (round 5): on, entered where the solve would end as NUMERICAL / MAX_ITER only.  The jam rule of the SRBM solver is OFF here: from
  // the callers' guess this NLP takes tiny steps for its first iterations as a matter of course (one slack after the other), the rule sends members
  // into the phase that converge without it (law datagen, 1024 drop states: 960 converged + 30 undecided with feas_jam 8 against 985 + 3 with 0)
  o->feas_jam = 0;
  // Round 6: the SRBM solver's restoration-style rules (several entries with an early return, landing_nlp.h feas_max / feas_back) need the jam rule to pay; with entries at the
  // iteration limit only they triple the work of the members that end without a decision (MI355X, law datagen, seeds 102 / 104: 1500 instead of 700 iterations, 2.5 instead of
  // 1.4 s per batch), and with the jam rule on (8 / 12) the six hold-out batches of the hard law take 0.69-1.34 / 0.63-1.45 s against 0.70-1.82 s -- inside the spread, while
  // a batch of law main loses a member (round-6 measurement).  One entry, no early return, as in round 5; the polishing step, LANDING_STALLED and the adapted regularisation
  // decay of the phase apply.
  o->feas_max = 1; o->feas_back = 0.0;
  // Round 5, late (profiles/r05_ab_experiments.txt "kinodynamic portfolio"; 5 bench batches of 1024, law main): the batch time is set by single members
  // that need 400 .. 1000 iterations on ONE path and 28 .. 73 on another.  (i) Portfolio: after 56 rounds the members still iterating are posed again in
  // three clone slots each (landing_nlp.h kd_clone_after): 0.72 / 0.75 / 1.09 / 1.99 / 1.43 s per batch -> 0.70 .. 0.76 s, no member undecided.
  // (ii) clip_k 16 (histogram form of the rule in landing_kd_iter_kernel): mean 35.1 -> 31.3 iterations; its own outliers (up to 1343 iterations) are
  // what the portfolio removes.  (iii) The slack re-initialisation of a crawling first barrier problem after 30 instead of 75 iterations
  // (restart_period): p99 of the converged members 72 -> 62 iterations.  Together with the delta_w continuation (KD_DELTA_JUMP): 0.50 .. 0.62 s.
  o->clip_k = 16; o->restart_period = 30;
  o->kd_clone_after = 56; o->kd_clone_max = 96; o->kd_clone_iter = 200;
}

int landing_kinodyn_solve_batch(landing_ctx* ctx, int B, int N, const landing_kinodyn_params* prm, const double* d_lbg, const double* d_ubg,
                                const double* d_cost, const double* d_x0, const landing_solver_opts* opts,
                                double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters, double* d_kkt, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 2 || N > 64 || !prm || !d_lbg || !d_ubg || !d_cost || !d_x0 || !d_x) return fail(LANDING_E_ARG, "landing_kinodyn_solve_batch: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_solve_batch: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_solve_batch")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  landing_solver_opts o;
  if (opts) o = *opts; else landing_kinodyn_solver_opts_default(&o);
  if (!(o.kappa_eps > 0.0)) o.kappa_eps = 80.0;
  if (!(o.mu_init > 0.0)) o.mu_init = 0.1;
  if (!(o.bound_push > 0.0)) o.bound_push = 0.01;
  if (!(o.theta_mu > 0.0)) o.theta_mu = 1.5;
  hipStream_t st = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(ctx->mu);
  // portfolio (landing_nlp.h kd_clone_after): clone slots behind the callers' members -- KD_NWAVE waves of KD_NVAR variants of up to F families
  const int cloneF = (o.kd_clone_after > 0 && o.kd_clone_max > 0 && o.max_iter > 0) ? (o.kd_clone_max < B ? o.kd_clone_max : B) : 0;
  const int S = cloneF * landing::KD_NVAR * landing::KD_NWAVE, BT = B + S;
  const size_t stride = landing::kd_ws_stride(N), need = stride * (size_t)BT;
  if (ctx->d_kd_ws.size() < need) {
    if (ctx->d_kd_ws) HIP_TRY(hipDeviceSynchronize());      // (a launch of an earlier call may still use the old block)
    HIP_TRY(ctx->d_kd_ws.grow(need));
  }
  ctx->kd_ws_N = 0; ctx->kd_ws_B = 0;      // (the debug view describes a workspace only once every launch of this solve is queued: below)
  // counters: derivative list A | members still iterating | members the head kernel has prepared this round | derivative list B  (the two in the middle and the list of the NEXT round are cleared by one memset per round)
  if (!ctx->d_kd_active) HIP_TRY(ctx->d_kd_active.alloc(4));
  const size_t nflag = (size_t)BT + S + 3 * B + 3 * BT;      // done [BT] | src [S] | win [B] | cloned [B] | win_prev [B] | work list of the condensation [BT] | derivative lists A, B [BT] each
  if (ctx->d_kd_done.size() < nflag) {
    if (ctx->d_kd_done) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(ctx->d_kd_done.grow(nflag));
  }
  landing::KdSolveArgs A;
  A.model = ctx->d_rbd.get(); A.B = BT; A.N = N; A.o = o; A.iter_cap = ctx->iter_cap;
  A.B0 = B; A.F = cloneF > 0 ? cloneF : 1; A.m_lo = 0;
  A.src = ctx->d_kd_done.get() + BT; A.win = S > 0 ? A.src + S : nullptr; A.cloned = A.src + S + B; A.win_prev = A.cloned + B; A.cond_list = A.src + S + 3 * B;
  // the clones' option sets: what decided the outliers of five bench batches in 28 .. 73 iterations (profiles/r05_ab_experiments.txt, tools/dev/kd_variants.py) --
  // the step rule with 16 clipped slacks, the same with the slacks pushed 0.1 into their rows, a first barrier parameter of 1
  for (int v = 0; v < landing::KD_NVAR; ++v) { A.ov[v] = o; A.ov[v].max_iter = o.kd_clone_iter > 0 ? o.kd_clone_iter : 200; }
  A.ov[0].clip_k = o.clip_k > 4 ? 4 : 16;
  A.ov[1].clip_k = 16; A.ov[1].bound_push = 0.1; A.ov[1].bound_frac = 0.1;
  A.ov[2].mu_init = 1.0;
  A.P = kd_params(ctx, prm, N);
  { const int rc = kd_ensure_pairs(ctx); if (rc) return rc; }      // structurally non-zero pairs of a Hessian block
  { const int rc = kd_ensure_jpat(ctx); if (rc) return rc; }            // structurally non-zero entries of a Jacobian block
  A.jpat = (const landing::KdJPat*)ctx->d_kd_jpat.get(); A.cpat = (const landing::KdCPat*)(ctx->d_kd_jpat.get() + ctx->kd_cpat_off);
  A.x0 = d_x0; A.lb = d_lbg; A.ub = d_ubg; A.cost = d_cost; A.ws = ctx->d_kd_ws.get(); A.ws_stride = stride;
  int* const cnt = ctx->d_kd_active.get();
  A.x_out = d_x; A.f_out = d_f; A.lam_out = d_lam_g; A.status = d_status; A.iters = d_iters; A.kkt = d_kkt; A.n_active = cnt + 1; A.n_cond = cnt + 2; A.done = ctx->d_kd_done.get();
  int* const dlist[2] = {A.cond_list + BT, A.cond_list + 2 * BT}; int* const dcnt[2] = {cnt, cnt + 3};
  A.dlist_next = dlist[0]; A.n_dnext = dcnt[0];      // (the init kernel fills the list of round 0)
  // function-layer launches straight into the workspace of every member: the arrays of member 0's block, one block further per member
  const landing::KdMem M = landing::kd_carve(N, A.ws);
  landing::KdNlpArgs F = kd_nlp_args(ctx, BT, N);
  F.P = A.P; F.x = M.x; F.lam = M.y; F.jac = M.J; F.hess = M.H; F.jty = M.jty;
  F.jcol = &A.cpat->jcol[0][0][0];               // the Jacobian kernel writes compact blocks (rbd_kernels.hip KD_JCS)
  F.sx = F.sg = F.sj = F.sh = (long long)stride; F.skip = A.done;
  // structural zeros of the Hessian blocks are written once; the kernel rewrites the 561 pairs of every block each iteration.  (The whole
  // workspace is cleared: the blocks are its largest part.)
  const long long nh = (long long)BT * N * ctx->kd_npair;
  if (nh > 0x7fffffffLL * 64) return fail(LANDING_E_ARG, "landing_kinodyn_solve_batch: batch too large for one launch");      // (before anything is queued: ADVICE r5)
  HIP_TRY(scratch_acquire(ctx, st));      // an earlier call's finish kernel (any stream) may still read the workspace, the flags and the counter
  // whatever path leaves this function from here on, the work queued so far is fenced for the next user of the context's scratch blocks (ADVICE r5: the error returns
  // below used to skip scratch_release, and the next call on another stream was then not ordered behind the memsets and launches already queued)
  struct ScratchGuard { landing_ctx* c; hipStream_t s; ~ScratchGuard() { (void)scratch_release(c, s); } } scratch_guard{ctx, st};
  HIP_TRY(hipMemsetAsync(A.ws, 0, need * sizeof(double), st));
  if (S > 0) {      // clone slots start unused (src = -1) and "finished" for the derivative kernels; no family has a winner
    HIP_TRY(hipMemsetAsync(A.done + B, 0x01, (size_t)S * sizeof(int), st));      // (any non-zero word: only the originals' flags are compared with 1)
    HIP_TRY(hipMemsetAsync(A.src, 0xff, (size_t)S * sizeof(int), st));
    HIP_TRY(hipMemsetAsync(A.win, 0x7f, (size_t)B * sizeof(int), st));      // KD_NOWIN
    HIP_TRY(hipMemsetAsync(A.cloned + B, 0x7f, (size_t)B * sizeof(int), st));      // win_prev
    HIP_TRY(hipMemsetAsync(A.cloned, 0, (size_t)B * sizeof(int), st));
  }
  HIP_TRY(hipMemsetAsync(cnt, 0, 4 * sizeof(int), st));
  hipLaunchKernelGGL(landing::landing_kd_init_kernel, dim3(B), dim3(landing::KD_THREADS), 0, st, A);
  // The derivative launches cover the members of the round's list (kd_solver_kernels.hip dlist_next), gridded for `bound` members: the count the host saw at its last look
  // (+ the clones posed since) -- a launch over the whole batch cost 0.1-0.2 ms of workgroups that leave at once per round of the lock-step tail
  int cur = 0, bound = B;
  auto derivs = [&](bool with_hess) {
    F.list = dlist[cur]; F.n_list = dcnt[cur];
    const int nbd = bound < BT ? bound : BT;
    kd_launch_jac(ctx, F, nbd, N, st);
    if (with_hess)
      kd_launch_hess(ctx, F, nbd, N, ctx->d_kd_pairs.get(), ctx->d_kd_pairs.get() + ctx->kd_npair, ctx->kd_npair, st);
  };
  int active = B;
  // (rounds, not iterations: a member whose inertia correction is spread over several launches needs more rounds than iterations; its own
  // iteration limit is checked in the kernel.)  The host looks at the number of members still iterating every KD_SYNC_EVERY rounds only: a
  // launch over finished members costs microseconds (every workgroup leaves at once), a host round trip per round cost more
  constexpr int KD_SYNC_EVERY = 4;
  const long long max_rounds = 8LL * (o.max_iter > 0 ? (long long)o.max_iter : 0LL);
  for (long long it = 0; it <= max_rounds && active > 0; ++it) {
    for (int w = 0; w < landing::KD_NWAVE && S > 0; ++w)
      if (it == (long long)o.kd_clone_after * (w + 1)) {      // portfolio: the members still iterating are posed again under the variants' option sets
        hipLaunchKernelGGL(landing::landing_kd_clone_kernel, dim3(1), dim3(landing::KD_THREADS), 0, st, A, w);
        landing::KdSolveArgs Ai = A; Ai.m_lo = B + w * landing::KD_NVAR * cloneF;
        Ai.dlist_next = dlist[cur]; Ai.n_dnext = dcnt[cur];      // (the clones join the list of THIS round's derivative launches)
        hipLaunchKernelGGL(landing::landing_kd_init_kernel, dim3(landing::KD_NVAR * cloneF), dim3(landing::KD_THREADS), 0, st, Ai);
        bound += landing::KD_NVAR * cloneF;
      }
    derivs(true);
    const bool look = (it % KD_SYNC_EVERY) == KD_SYNC_EVERY - 1 || it == max_rounds;
    HIP_TRY(hipMemsetAsync(cnt + (cur == 0 ? 1 : 0), 0, 3 * sizeof(int), st));      // members still iterating, members prepared, the list of the next round
    A.dlist_next = dlist[cur ^ 1]; A.n_dnext = dcnt[cur ^ 1]; A.dlist_cur = dlist[cur]; A.n_dcur = dcnt[cur];
    if (S > 0 && it >= (long long)o.kd_clone_after) HIP_TRY(hipMemcpyAsync(A.cloned + B, A.win, (size_t)B * sizeof(int), hipMemcpyDeviceToDevice, st));      // winners of the earlier rounds end their relatives in this one
    // three launches per iteration (kd_solver_kernels.hip): head (stop test, barrier parameter) | condensation of the inequality rows, one workgroup per member and interval |
    // Riccati sweeps, line search, acceptance.  The head kernel runs over the round's derivative list (members with a new point + pending ones), the other two over the list the head passes on (ADVICE r5: no launch over empty clone slots)
    const int nb = bound < BT ? bound : BT;      // (the lists of the round hold at most as many members as the host saw at its last look + the clones posed since)
    hipLaunchKernelGGL(landing::landing_kd_head_kernel, dim3(nb), dim3(landing::KD_THREADS), 0, st, A);
    hipLaunchKernelGGL(landing::landing_kd_condense_kernel, dim3(nb * N < landing::KD_COND_GRID ? nb * N : landing::KD_COND_GRID), dim3(landing::KD_THREADS), 0, st, A);
    hipLaunchKernelGGL(landing::landing_kd_iter_kernel, dim3(nb), dim3(landing::KD_THREADS), 0, st, A);
    if (look) {
      HIP_TRY(hipMemcpyAsync(&active, A.n_active, sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      bound = active;
    }
    cur ^= 1;
  }
  if (active > 0) derivs(false);      // members stopped by the iteration limit: their J blocks belong to the previous iterate
  hipLaunchKernelGGL(landing::landing_kd_finish_kernel, dim3(B), dim3(landing::KD_THREADS), 0, st, A);
  HIP_TRY(hipGetLastError());
  ctx->kd_ws_N = N; ctx->kd_ws_B = BT;
  return 0;      // (scratch_guard records the fence)
}

void landing_kinodyn_form_knitro(landing_kinodyn_form* f) {      /* literals of generate_solver/generate_landingCtrller_KNITRO.m:139-189: kin_box_y = 0.125 + kin_box(2) (:154) */
  landing_kinodyn_form_default(f);
  f->kin_box_y0 = 0.125;
}
void landing_kinodyn_form_default(landing_kinodyn_form* f) {
  f->comp_eps = 1e-3; f->slip_eps = 1e-3; f->fk_band = 0.01;
  f->kin_box_x0 = 0.125; f->kin_box_y0 = 0.10; f->kin_box_y_in = 0.05; f->kin_box_z_lo = -0.4; f->kin_box_z_hi = -0.075;
  f->tau_max[0] = 18.0; f->tau_max[1] = 18.0; f->tau_max[2] = 3.0 * 9.33;      /* model.tauMax = gr .* motorTauMax (get_robot_model.m:236-240) */
}

/* lbg / ubg of B members in the row order of landing_kinodyn_nlp_eval (host arrays; Opti's canonicalisation of landing_optimization.m:89-189:
 * an expression bounded twice appears twice, each copy with one finite bound).  Per-member arguments carry a trailing batch axis. */
int landing_kinodyn_bounds(int N, int B, const landing_kinodyn_form* form, const double* q_init, const double* qd_init, const double* c_init,
                           const double* q_min, const double* q_term_min, const double* q_term_max, const double* qd_term_min, const double* qd_term_max,
                           const double* jpos_min, const double* jpos_max, const double* kin_box, const double* l_leg_max, double* lbg, double* ubg) {
  if (N < 2 || N > 64 || B < 0 || !q_init || !qd_init || !c_init || !q_min || !q_term_min || !q_term_max || !qd_term_min || !qd_term_max || !jpos_min || !jpos_max ||
      !kin_box || !l_leg_max || !lbg || !ubg)
    return fail(LANDING_E_ARG, "landing_kinodyn_bounds: bad argument");
  landing_kinodyn_form F;
  if (form) F = *form; else landing_kinodyn_form_default(&F);
  const size_t ng = (size_t)landing::kd_ng(N);
  const double INF = INFINITY;
  for (int b = 0; b < B; ++b) {
    double* lb = lbg + (size_t)b * ng; double* ub = ubg + (size_t)b * ng;
    for (int i = 0; i < 6; ++i) {
      lb[i] = ub[i] = q_init[6 * b + i]; lb[6 + i] = ub[6 + i] = qd_init[6 * b + i];
      lb[24 + i] = q_term_min[6 * b + i]; ub[24 + i] = INF; lb[30 + i] = -INF; ub[30 + i] = q_term_max[6 * b + i];
      lb[36 + i] = qd_term_min[6 * b + i]; ub[36 + i] = INF; lb[42 + i] = -INF; ub[42 + i] = qd_term_max[6 * b + i];
    }
    for (int i = 0; i < 12; ++i) lb[12 + i] = ub[12 + i] = c_init[12 * b + i];
    const double kbx = F.kin_box_x0 + kin_box[2 * b], kby = F.kin_box_y0 + kin_box[2 * b + 1], ll2 = l_leg_max[b] * l_leg_max[b];
    for (int k = 0; k < N; ++k) {
      const bool last = k == N - 1;
      size_t r = landing::KD_BND + (size_t)k * landing::KD_ROWS;
      for (int i = 0; i < 12; ++i) { lb[r] = 0.0; ub[r] = 0.0; ++r; }                       /* Euler defects */
      for (int l = 0; l < 4; ++l) { lb[r] = 0.0; ub[r] = INF; ++r; }                         /* f_z >= 0 */
      for (int l = 0; l < 4; ++l) {
        lb[r] = 0.0; ub[r] = INF; ++r;                                                        /* c_z >= 0 */
        lb[r] = -INF; ub[r] = F.comp_eps; ++r;                                                /* f_z c_z <= eps */
        if (!last) {
          for (int a = 0; a < 3; ++a) { lb[r] = -INF; ub[r] = F.slip_eps; ++r; }
          for (int a = 0; a < 3; ++a) { lb[r] = -F.slip_eps; ub[r] = INF; ++r; }
        }
        lb[r] = -kbx; ub[r] = kbx; ++r;
        if (l == 0 || l == 2) { lb[r] = -kby; ub[r] = F.kin_box_y_in; } else { lb[r] = -F.kin_box_y_in; ub[r] = kby; }      /* :159-163 (sideSign -1, 1, -1, 1) */
        ++r;
        lb[r] = F.kin_box_z_lo; ub[r] = F.kin_box_z_hi; ++r;
        lb[r] = -INF; ub[r] = ll2; ++r;
        for (int a = 0; a < 3; ++a) { lb[r] = -F.tau_max[a]; ub[r] = F.tau_max[a]; ++r; }
      }
      for (int s4 = 0; s4 < 4; ++s4) for (int l = 0; l < 4; ++l) { lb[r] = -INF; ub[r] = 0.0; ++r; }      /* friction: `g1 <= g2` with variables on both sides -> g1 - g2 in (-inf, 0] (optistack_internal.cpp:793-813) */
      lb[r] = q_min[6 * b + 2]; ub[r] = INF; ++r;                                            /* only the z bound is enforced (:181) */
      for (int i = 0; i < 12; ++i) { lb[r] = -F.fk_band; ub[r] = INF; ++r; }
      for (int i = 0; i < 12; ++i) { lb[r] = -INF; ub[r] = F.fk_band; ++r; }
      for (int i = 0; i < 12; ++i) { lb[r] = jpos_min[12 * b + i]; ub[r] = INF; ++r; }
      for (int i = 0; i < 12; ++i) { lb[r] = -INF; ub[r] = jpos_max[12 * b + i]; ++r; }
      if (r != landing::KD_BND + (size_t)k * landing::KD_ROWS + (last ? landing::KD_ROWS_LAST : landing::KD_ROWS)) return fail(LANDING_E_ARG, "landing_kinodyn_bounds: internal row count");
    }
  }
  return 0;
}

int landing_kinodyn_solve_batch_host(landing_ctx* ctx, int B, int N, const landing_kinodyn_params* prm, const double* lbg, const double* ubg,
                                     const double* cost, const double* x0, const landing_solver_opts* opts,
                                     double* x, double* f, double* lam_g, int* status, int* iters, double* kkt) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 2 || N > 64 || !lbg || !ubg || !cost || !x0 || !x) return fail(LANDING_E_ARG, "landing_kinodyn_solve_batch_host: bad argument");
  std::vector<int> status_own;      // the retry ladder below needs the outcome of the first pass also when the caller did not ask for it
  if (!opts && !status) { status_own.resize((size_t)B); status = status_own.data(); }
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t nx = (size_t)landing::kd_nx(N), ng = (size_t)landing::kd_ng(N);
  const size_t b = (size_t)B;
  {
    Staging st(nullptr);
    const double* d_lb = st.in(lbg, b * ng); const double* d_ub = st.in(ubg, b * ng); const double* d_cost = st.in(cost, b * 24); const double* d_x0 = st.in(x0, b * nx);
    double* d_x = st.out(x, b * nx); double* d_f = st.out_always(f, b); double* d_lam = st.out_always(lam_g, b * ng); double* d_kkt = st.out_always(kkt, b * 3);
    int* d_st = st.out_always(status, b); int* d_it = st.out_always(iters, b);
    HIP_TRY(st.error());
    if (const int rc = landing_kinodyn_solve_batch(ctx, B, N, prm, d_lb, d_ub, d_cost, d_x0, opts, d_x, d_f, d_lam, d_st, d_it, d_kkt, nullptr)) return rc;
    HIP_TRY(st.fetch());
  }      // (the staging blocks go before the retry ladder allocates its own)
  // ---- retry ladder (default options only): the members the first pass left undecided (iteration limit / numerical failure) are solved again
  // from the same initial guess with another slack initialisation, then with a smaller first barrier parameter.  Which members end undecided
  // depends on the path, not on the problem: on the hard sampling law 19 of 1024 with the defaults, 17 with each of the two alternatives, and
  // the three sets overlap in 5 (tools/dev/kd_lab.py --configs).  A member keeps the first decided outcome (converged or certified infeasible);
  // its iteration count is the sum over the passes.  Callers who pass their own options get exactly one pass with them.
  if (!opts && status) {
    for (int pass = 0; pass < 2; ++pass) {
      std::vector<int> idx;
      for (int b = 0; b < B; ++b) if (status[b] == LANDING_MAX_ITER || status[b] == LANDING_NUMERICAL) idx.push_back(b);
      if (idx.empty()) break;
      const size_t n = idx.size();
      std::vector<double> lb2(n * ng), ub2(n * ng), c2(n * 24), x02(n * nx), x2(n * nx), f2(n), l2(n * ng), k2(n * 3);
      std::vector<int> s2(n), i2(n);
      for (size_t j = 0; j < n; ++j) {
        const size_t b = (size_t)idx[j];
        std::copy(lbg + b * ng, lbg + (b + 1) * ng, lb2.begin() + j * ng); std::copy(ubg + b * ng, ubg + (b + 1) * ng, ub2.begin() + j * ng);
        std::copy(cost + b * 24, cost + (b + 1) * 24, c2.begin() + j * 24); std::copy(x0 + b * nx, x0 + (b + 1) * nx, x02.begin() + j * nx);
      }
      landing_solver_opts o2;
      landing_kinodyn_solver_opts_default(&o2);
      if (pass == 0) { o2.bound_push = 0.1; o2.bound_frac = 0.1; } else o2.mu_init = 0.02;
      const int rc2 = landing_kinodyn_solve_batch_host(ctx, (int)n, N, prm, lb2.data(), ub2.data(), c2.data(), x02.data(), &o2, x2.data(), f2.data(), l2.data(), s2.data(), i2.data(), k2.data());
      if (rc2) return rc2;
      for (size_t j = 0; j < n; ++j) {
        const size_t b = (size_t)idx[j];
        if (iters) iters[b] += i2[j];
        if (s2[j] != LANDING_CONVERGED && s2[j] != LANDING_INFEASIBLE) continue;
        std::copy(x2.begin() + j * nx, x2.begin() + (j + 1) * nx, x + b * nx);
        if (f) f[b] = f2[j];
        if (lam_g) std::copy(l2.begin() + j * ng, l2.begin() + (j + 1) * ng, lam_g + b * ng);
        if (kkt) std::copy(k2.begin() + j * 3, k2.begin() + (j + 1) * 3, kkt + b * 3);
        status[b] = s2[j];
      }
    }
  }
  return 0;
}


/* The reference's 24-argument solver function of the kinodynamic refinement (generate_solver/generate_landingCtrller_KNITRO.m:373-377; call
 * sites generate_data/generate_training_data_automated.m:150-156,169-175, codegen_casadi/test_loadCasadi.m), batched: HOST pointers,
 * column-major, trailing batch axis.  Inactive Opti parameters of that NLP (Uref, q_max, qd_min, qd_max; only q_min(3) of q_min) are accepted
 * and ignored as CasADi ignores them. */
int landing_solve_kinodyn_24(landing_ctx* ctx, int N, int B, const landing_kinodyn_form* form,
                             const double* Xref, const double* Uref, const double* dt, const double* q_min, const double* q_max, const double* qd_min,
                             const double* qd_max, const double* q_init, const double* qd_init, const double* c_init, const double* q_term_min,
                             const double* q_term_max, const double* qd_term_min, const double* qd_term_max, const double* QN, const double* x0,
                             const double* jpos_min, const double* jpos_max, const double* kin_box, const double* mu, const double* l_leg_max,
                             const double* mass, const double* Ib, const double* Ib_inv, const landing_solver_opts* opts,
                             double* x_star, double* f_star, double* lam_g, int* status, int* iters, double* kkt) {
  (void)Uref; (void)q_max; (void)qd_min; (void)qd_max;
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || N < 2 || N > 64 || !Xref || !dt || !q_min || !q_init || !qd_init || !c_init || !q_term_min || !q_term_max || !qd_term_min || !qd_term_max ||
      !QN || !x0 || !jpos_min || !jpos_max || !kin_box || !mu || !l_leg_max || !mass || !Ib || !Ib_inv || !x_star)
    return fail(LANDING_E_ARG, "landing_solve_kinodyn_24: NULL argument");
  landing_kinodyn_params prm;
  memset(&prm, 0, sizeof(prm));
  for (int k = 0; k < N; ++k) prm.dt[k] = dt[k];
  prm.mass = mass[0]; prm.mu = mu[0];
  for (int i = 0; i < 3; ++i) { prm.Ib[i] = Ib[i]; prm.Ib_inv[i] = Ib_inv[i]; }
  for (int b = 1; b < B; ++b) {      // the batch shares one time grid and one robot (constants of every caller of the reference)
    bool same = mass[b] == mass[0] && mu[b] == mu[0];
    for (int k = 0; k < N && same; ++k) same = dt[(size_t)b * N + k] == dt[k];
    for (int i = 0; i < 3 && same; ++i) same = Ib[3 * b + i] == Ib[i] && Ib_inv[3 * b + i] == Ib_inv[i];
    if (!same) return fail(LANDING_E_ARG, "landing_solve_kinodyn_24: dt, mu, mass, Ib, Ib_inv must be the same for every member of a call");
  }
  const size_t ng = (size_t)landing::kd_ng(N);
  std::vector<double> lbg((size_t)B * ng), ubg((size_t)B * ng), cost((size_t)B * 24);
  landing_kinodyn_form Fk;      // this entry point stands for the function generate_landingCtrller_KNITRO.m builds: NULL = THAT script's literals
  if (form) Fk = *form; else landing_kinodyn_form_knitro(&Fk);
  int rc = landing_kinodyn_bounds(N, B, &Fk, q_init, qd_init, c_init, q_min, q_term_min, q_term_max, qd_term_min, qd_term_max, jpos_min, jpos_max, kin_box,
                                  l_leg_max, lbg.data(), ubg.data());
  if (rc) return rc;
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < 12; ++i) { cost[(size_t)b * 24 + i] = QN[12 * b + i]; cost[(size_t)b * 24 + 12 + i] = Xref[(size_t)b * 12 * (N + 1) + 12 * N + i]; }
  return landing_kinodyn_solve_batch_host(ctx, B, N, &prm, lbg.data(), ubg.data(), cost.data(), x0, opts, x_star, f_star, lam_g, status, iters, kkt);
}

/* CCS patterns of the refinement NLP in CasADi's compressed form -- jac_g_x (ng x nx) and the UPPER triangle of hess_gamma_x_x (nx x nx) --
 * taken from the very derivative kernels the solver uses: their block outputs at three random points (random multipliers for the Hessian)
 * are scanned for entries that are not identically zero.  colind [nx + 1], row [nnz]; *nnz receives the count (call with row = NULL first).
 * Needs a context with a model (the kernels run on the device).  The reference's own generated code for this NLP is a missing blob
 * (.MISSING_LARGE_BLOBS:1-4), so there is no casadi_s* table to compare with; the counts are pinned in tests/test_kd_solver_cpu.py. */
int landing_kinodyn_pattern(landing_ctx* ctx, int N, int which /* 0 = jac_g_x, 1 = triu hess */, long long* colind, long long* row, long long* nnz) {
  if (!ctx || N < 2 || N > 64 || !colind || !nnz || which < 0 || which > 1) return fail(LANDING_E_ARG, "landing_kinodyn_pattern: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_pattern: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_pattern")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  const int nx = landing::kd_nx(N), ng = landing::kd_ng(N), NW = landing::KD_NW, NR = landing::KD_ROWS;
  landing_kinodyn_params prm;
  memset(&prm, 0, sizeof(prm));
  for (int k = 0; k < N; ++k) prm.dt[k] = 0.02 + 0.001 * k;
  prm.mass = 8.25; prm.mu = 0.7; prm.Ib[0] = 0.06; prm.Ib[1] = 0.23; prm.Ib[2] = 0.28; prm.Ib_inv[0] = 17.0; prm.Ib_inv[1] = 4.3; prm.Ib_inv[2] = 3.6;
  const int T = 3;
  std::vector<double> x((size_t)T * nx), lam((size_t)T * ng);
  unsigned long long sd = 88172645463325252ull;
  auto rnd = [&]() { sd ^= sd << 13; sd ^= sd >> 7; sd ^= sd << 17; return (double)(sd >> 11) / 9007199254740992.0 - 0.5; };
  for (auto& v : x) v = 0.8 * rnd() + 0.05;
  for (auto& v : lam) v = rnd() + 0.01;
  const size_t no = (size_t)T * N * (which ? NW * NW : NR * NW);
  std::vector<double> out(no);
  {
    Staging st(nullptr);
    const double* d_x = st.in(x.data(), x.size()); const double* d_l = st.in(lam.data(), lam.size());
    double* d_o = st.out(out.data(), no);
    HIP_TRY(st.error());
    HIP_TRY(hipMemset(d_o, 0, no * sizeof(double)));
    const int rc = which ? landing_kinodyn_nlp_hess(ctx, T, N, d_x, &prm, d_l, d_o, nullptr) : landing_kinodyn_nlp_eval(ctx, T, N, d_x, &prm, nullptr, d_o, nullptr);
    if (rc) return rc;
    HIP_TRY(st.fetch());
  }
  std::vector<std::set<long long>> cols(nx);
  if (!which) {
    const int oU = 12 * (N + 1) + 12 * N;
    for (int i = 0; i < 12; ++i) { cols[i].insert(i); cols[oU + i].insert(12 + i); }
    for (int i = 0; i < 6; ++i) { cols[12 * N + i].insert(24 + i); cols[12 * N + i].insert(30 + i); cols[12 * N + 6 + i].insert(36 + i); cols[12 * N + 6 + i].insert(42 + i); }
    for (int k = 0; k < N; ++k) {
      const int nr = k == N - 1 ? landing::KD_ROWS_LAST : NR;
      for (int r = 0; r < nr; ++r) for (int j = 0; j < NW; ++j) {
        const int xi = landing::kd_w_index(N, k, j); if (xi < 0) continue;
        bool nz = false;
        for (int t = 0; t < T; ++t) nz = nz || out[(((size_t)t * N + k) * NR + r) * NW + j] != 0.0;
        if (nz) cols[xi].insert(landing::KD_BND + (long long)k * NR + r);
      }
    }
  } else {
    for (int i = 0; i < 12; ++i) cols[12 * N + i].insert(12 * N + i);      /* terminal cost 2 QN on X(:, N+1) (entries with QN = 0 are structural too: QN is a parameter) */
    for (int k = 0; k < N; ++k) for (int a = 0; a < NW; ++a) for (int b2 = 0; b2 < NW; ++b2) {
      const int xa = landing::kd_w_index(N, k, a), xb = landing::kd_w_index(N, k, b2); if (xa < 0 || xb < 0) continue;
      bool nz = false;
      for (int t = 0; t < T; ++t) nz = nz || out[(((size_t)t * N + k) * NW + a) * NW + b2] != 0.0;
      if (nz) { const int lo = xa < xb ? xa : xb, hi = xa < xb ? xb : xa; cols[hi].insert(lo); }
    }
  }
  long long n = 0;
  for (int c = 0; c < nx; ++c) { colind[c] = n; for (long long r : cols[c]) { if (row) row[n] = r; ++n; } }
  colind[nx] = n; *nnz = n;
  return 0;
}


int landing_kinodyn_block_nonzeros(landing_ctx* ctx, int* nnz_mid, int* nnz_last, unsigned char* entries) {
  if (!ctx || !nnz_mid || !nnz_last) return fail(LANDING_E_ARG, "landing_kinodyn_block_nonzeros: bad argument");
  if (!ctx->d_rbd) return fail(LANDING_E_ARG, "landing_kinodyn_block_nonzeros: no model (landing_rbd_set_model)");
  if (const int rc = rbd_need_legs(ctx, "landing_kinodyn_block_nonzeros")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lock(ctx->mu);
  { const int rc = kd_ensure_jpat(ctx); if (rc) return rc; }
  *nnz_mid = ctx->kd_jpat_nnz[0]; *nnz_last = ctx->kd_jpat_nnz[1];
  if (entries) {
    std::vector<landing::KdJPat> T(1);
    HIP_TRY(hipMemcpy(T.data(), ctx->d_kd_jpat.get(), sizeof(landing::KdJPat), hipMemcpyDeviceToHost));
    size_t n = 0;
    for (int lp = 0; lp < 2; ++lp) {
      const int nrow = (lp ? landing::KD_ROWS_LAST : landing::KD_ROWS) - 12;
      for (int j = 0; j < nrow; ++j) for (int t = T[0].rp[lp][j]; t < T[0].rp[lp][j + 1]; ++t) { entries[n++] = T[0].perm[lp][j]; entries[n++] = T[0].cl[lp][t]; }
    }
  }
  return 0;
}

// ---- diagnostics: a read-only view of a member's block of the refinement solver's workspace (landing_nlp.h) ----------------------------
int landing_debug_kd_workspace(landing_ctx* ctx, double** d_ws, unsigned long long* stride, int* N, int* members) {
  if (!ctx || !d_ws || !stride) return fail(LANDING_E_ARG, "landing_debug_kd_workspace: bad argument");
  if (!ctx->d_kd_ws || ctx->kd_ws_N < 2) return fail(LANDING_E_ARG, "landing_debug_kd_workspace: no kinodynamic solve has run in this context");
  *d_ws = ctx->d_kd_ws.get(); *stride = (unsigned long long)landing::kd_ws_stride(ctx->kd_ws_N);
  if (N) *N = ctx->kd_ws_N;
  if (members) *members = ctx->kd_ws_B;
  return 0;
}

int landing_debug_kd_layout(int N, unsigned long long* offsets, unsigned long long* state_offset, unsigned long long* stride) {
  if (N < 2 || N > 64 || !offsets) return fail(LANDING_E_ARG, "landing_debug_kd_layout: bad argument");
  // kd_carve itself over a host block of one member's size (never read or written): the one statement of the layout
  std::vector<double> block(landing::kd_ws_stride(N));
  double* const base = block.data();
  const landing::KdMem M = landing::kd_carve(N, base);
  const double* const arr[LANDING_KD_LAYOUT_N] = {M.x, M.dx, M.g, M.s, M.ds, M.zL, M.zU, M.y, M.yn, M.sig, M.rho, M.gc, M.en, M.ep, M.wn, M.wp};
  for (int i = 0; i < LANDING_KD_LAYOUT_N; ++i) offsets[i] = (unsigned long long)(arr[i] - base);
  if (state_offset) *state_offset = (unsigned long long)(reinterpret_cast<const double*>(M.st) - base);
  if (stride) *stride = (unsigned long long)landing::kd_ws_stride(N);
  return 0;
}

int landing_debug_kd_state(landing_ctx* ctx, int member, double* out) {
  if (!ctx || !out || member < 0) return fail(LANDING_E_ARG, "landing_debug_kd_state: bad argument");
  if (!ctx->d_kd_ws || ctx->kd_ws_N < 2) return fail(LANDING_E_ARG, "landing_debug_kd_state: no kinodynamic solve has run in this context");
  if (member >= ctx->kd_ws_B) return fail(LANDING_E_ARG, "landing_debug_kd_state: no such member in the last solve");
  HIP_TRY(hipSetDevice(ctx->device));
  const landing::KdMem M = landing::kd_carve(ctx->kd_ws_N, ctx->d_kd_ws.get() + (size_t)member * landing::kd_ws_stride(ctx->kd_ws_N));
  landing::KdState K;
  HIP_TRY(hipMemcpy(&K, M.st, sizeof(K), hipMemcpyDeviceToHost));      // (synchronises with the solve that wrote it)
  const double v[LANDING_KD_STATE_N] = {K.mu, K.delta, K.delta_last, K.alpha, K.a_du, (double)K.it, (double)K.nfact, (double)K.nreset, (double)K.last_reset_it, (double)K.feas,
                                        (double)K.status, (double)K.pending, K.omt, K.s_corr, (double)K.done, (double)K.reg_it};
  for (int i = 0; i < LANDING_KD_STATE_N; ++i) out[i] = v[i];
  return 0;
}

/* The contexts behind the one-call entry points (landing_solve_kinodyn_24_on*, landing_pipeline_21_on): one per (N, device) with the 'mc3D' model, shared by
 * all of them, built at the first call and kept until the process ends.  (Calls on one context from several host threads are serialised by the context.) */
static int cached_mc3d_ctx(int N, int device, landing_ctx** out) {
  static std::mutex cache_mu; static std::map<std::pair<int, int>, landing_ctx*> cache;
  std::lock_guard<std::mutex> lock(cache_mu);
  auto it = cache.find({N, device});
  if (it == cache.end()) {
    landing_ctx* ctx = landing_create(N, device, nullptr);
    if (!ctx) return LANDING_E_ARG;
    landing_rbd_model mdl; landing_rbd_model_mc3d(&mdl);
    const int rc = landing_rbd_set_model(ctx, &mdl);
    if (rc) { landing_destroy(ctx); return rc; }
    it = cache.emplace(std::make_pair(N, device), ctx).first;
  }
  *out = it->second;
  return 0;
}

/* One-call form for FFI stubs (matlab/landing_refine_mex.c): a context per (N, device) with the 'mc3D' model is cached inside the library. */
int landing_solve_kinodyn_24_on_form(int device, int N, int B, const landing_kinodyn_form* form, const double* Xref, const double* Uref, const double* dt,
                                     const double* q_min, const double* q_max, const double* qd_min, const double* qd_max, const double* q_init, const double* qd_init,
                                     const double* c_init, const double* q_term_min, const double* q_term_max, const double* qd_term_min, const double* qd_term_max,
                                     const double* QN, const double* x0, const double* jpos_min, const double* jpos_max, const double* kin_box, const double* mu,
                                     const double* l_leg_max, const double* mass, const double* Ib, const double* Ib_inv, const landing_solver_opts* opts,
                                     double* x_star, double* f_star, double* lam_g, int* status, int* iters, double* kkt) {
  landing_ctx* ctx;
  if (const int rc = cached_mc3d_ctx(N, device, &ctx)) return rc;
  return landing_solve_kinodyn_24(ctx, N, B, form, Xref, Uref, dt, q_min, q_max, qd_min, qd_max, q_init, qd_init, c_init, q_term_min, q_term_max, qd_term_min,
                                  qd_term_max, QN, x0, jpos_min, jpos_max, kin_box, mu, l_leg_max, mass, Ib, Ib_inv, opts, x_star, f_star, lam_g, status, iters, kkt);
}
int landing_solve_kinodyn_24_on(int device, int N, int B, const double* Xref, const double* Uref, const double* dt, const double* q_min, const double* q_max,
                                const double* qd_min, const double* qd_max, const double* q_init, const double* qd_init, const double* c_init,
                                const double* q_term_min, const double* q_term_max, const double* qd_term_min, const double* qd_term_max, const double* QN,
                                const double* x0, const double* jpos_min, const double* jpos_max, const double* kin_box, const double* mu, const double* l_leg_max,
                                const double* mass, const double* Ib, const double* Ib_inv, const landing_solver_opts* opts,
                                double* x_star, double* f_star, double* lam_g, int* status, int* iters, double* kkt) {
  return landing_solve_kinodyn_24_on_form(device, N, B, nullptr, Xref, Uref, dt, q_min, q_max, qd_min, qd_max, q_init, qd_init, c_init, q_term_min, q_term_max,
                                          qd_term_min, qd_term_max, QN, x0, jpos_min, jpos_max, kin_box, mu, l_leg_max, mass, Ib, Ib_inv, opts, x_star, f_star,
                                          lam_g, status, iters, kkt);
}

}  // extern "C"
