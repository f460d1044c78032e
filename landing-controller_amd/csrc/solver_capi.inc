// solver_capi.inc -- host side of landing_solve_batch (included by capi.hip): assembly tables built
// from the CCS patterns, workspace management, launch.  No CPU solve path exists here.
//
// Assembly tables.  The solver kernel consumes the SAME CCS nonzeros the function layer emits
// (casadi_s5 / casadi_s4 order).  For every stage k the host precomputes, from the patterns, how the
// stage's nonzeros combine into the condensed stage block
//     G_k = H_k + J_d^T Sigma J_d   (48x48 over w = [X_k(12) c_k(12) f_k(12) c_{k+1}(12)])
// the barrier gradient gamma_k = J_d^T rho and the dynamics block A^ = -dg_dyn/d(X_k,c_k,f_k) (12x36, rows in
// state order), and, for the whole horizon, the records of the row products J_d dx.  Stages with identical tables
// share one (first / middle / penultimate / last stage), so the table data stays L1/L2 resident.

namespace {

constexpr int NTH = landing::SOLVER_THREADS;

// What the solver kernel reads (SolveArgs): everything in lists interleaved over the 256 threads, entry j of thread t at [j * 256 + t]
struct SolverTables {
  std::vector<unsigned long long> ctab, ccomb;      // per stage type: terms [c_ml][256] (landing::aterm_pack), destinations summed from partial slots [256] (landing::acomb_pack)
  std::vector<int> ctype;                           // type of every stage, numbered as first seen
  int c_ml = 0, c_mid = 0;                          // terms per thread; the most frequent type
  std::vector<unsigned long long> rterm;            // row products [rlen][256]: jac index | x index << 16 | row << 32 | closes the row << 48 | valid << 49
  int rlen = 0;
};

// One entry of G (upper triangle, elimination order), of gamma or of A^: its byte offset inside the kernel's LDS block (`ah`: inside Lds::Ah,
// whose two copies alternate between stages) and the terms summed into it, each a product of three entries of the LDS array cx
struct AsmDest {
  int d; bool ah;
  std::vector<std::array<int, 3>> terms;      // positions in cx
  bool operator==(const AsmDest& o) const { return d == o.d && ah == o.ah && terms == o.terms; }
};

// w-index of global variable c relative to stage k, or -1 (X_{k+1} / unrelated)
int w_index(const Layout& L, int k, long long c) {
  const int N = L.N;
  if (c >= L.x_X(k) && c < L.x_X(k) + 12) return (int)(c - L.x_X(k));
  if (c >= L.x_U(k) && c < L.x_U(k) + 24) { const int j = (int)(c - L.x_U(k)); return j < 12 ? 12 + j : 24 + (j - 12); }
  if (k < N - 1 && c >= L.x_U(k + 1) && c < L.x_U(k + 1) + 12) return 36 + (int)(c - L.x_U(k + 1));
  return -1;
}
// position in cx of entry `off` of segment `seg` of the stage's nonzeros (asm_copy: J X_k | J U_k | J U_{k+1} | H X_k | H U_k | H U_{k+1} | running-cost
// constants, one load per thread and segment), or -1 when the segment does not hold it
int seg_pos(int seg, long long off) { return off >= 0 && off < landing::ASM_SEG_LEN[seg] ? landing::ASM_SEG_POS[seg] + (int)off : -1; }
// ... of Jacobian nonzero idx (column c) of stage k, or -1
int jpos(const Layout& L, int k, long long c, long long idx) {
  if (c >= L.x_X(k) && c < L.x_X(k) + 12) return seg_pos(0, idx - L.jx(k));
  if (c >= L.x_U(k) && c < L.x_U(k) + 24) return seg_pos(1, idx - L.ju(k));
  if (k < L.N - 1 && c >= L.x_U(k + 1) && c < L.x_U(k + 1) + 12) return seg_pos(2, idx - L.ju(k + 1));
  return -1;
}

struct Patterns {
  std::vector<std::vector<std::pair<long long, long long>>> rows;      // row-major view of J: (col, idx)
  std::vector<long long> hci, hr;                                      // CCS of the Hessian
};

// Destinations of stage k in table order -- the entries of G by (a, b), a <= b indices into w; gamma 0..47, a structural zero included; A^ in the
// order of the dynamics rows -- with their terms in the order they are summed in.  Appends the stage's row-product records to `rrec`.
int stage_dests(const Layout& L, int k, const Patterns& pat, std::vector<AsmDest>& dests, std::vector<unsigned long long>& rrec) {
  using namespace landing;
  const int oG = (int)offsetof(Lds, G), oAh = (int)offsetof(Lds, Ah);
  // G in elimination order, the same for every stage type: (sigma, f, c+) -> rows / columns (f, c+, sigma); gamma is its spare column
  auto gpos = [](int a) { return a < 24 ? a + 24 : a - 24; };
  const bool last = (k == L.N - 1);
  const int nr = L.rows(k), g0 = L.g_stage(k);
  if (nr > 104) return -9;      // sigma and rho of a stage's rows: 104 entries each in cx
  std::map<std::pair<int, int>, std::vector<std::array<int, 3>>> tg;
  std::vector<std::vector<std::array<int, 3>>> gm(48);
  std::vector<AsmDest> ah;
  // --- Jacobian rows ---
  for (int q = 0; q < nr; ++q) {
    std::vector<std::array<int, 2>> ent;   // (w index, position)
    const size_t r0 = rrec.size();
    for (auto& ci : pat.rows[g0 + q]) {
      const int a = w_index(L, k, ci.first);
      if (a < 0) continue;                 // X_{k+1} identity
      const int pos = jpos(L, k, ci.first, ci.second);
      if (pos < 0) return -2;
      ent.push_back({a, pos});
      if (q < 12) continue;
      if (ci.second > 0xffff || ci.first > 0xffff || g0 + q > 0xffff) return -18;      // the 16-bit fields of a record
      rrec.push_back((unsigned long long)ci.second | ((unsigned long long)ci.first << 16) | (1ull << 49));
    }
    if (rrec.size() > r0) rrec.back() |= ((unsigned long long)(g0 + q) << 32) | (1ull << 48);
    if (q < 12) {                          // dynamics rows -> A^ (state order)
      const int sr = q < 6 ? q : (q < 9 ? q + 3 : q - 3);
      for (auto& e : ent) { if (e[0] >= 36) return -3; ah.push_back({oAh + 8 * (sr * YS + e[0]), true, {{e[1], CX_ONE, CX_MONE}}}); }
    } else {                               // inequality rows: sigma_q J_qa J_qb into G, rho_q J_qa into gamma
      for (size_t i = 0; i < ent.size(); ++i) {
        gm[ent[i][0]].push_back({ent[i][1], CX_ONE, CX_SR + 104 + q});
        for (size_t j = i; j < ent.size(); ++j) {
          int a = ent[i][0], b = ent[j][0], pa = ent[i][1], pb = ent[j][1];
          if (a > b) { std::swap(a, b); std::swap(pa, pb); }
          tg[{a, b}].push_back({pa, pb, CX_SR + q});
        }
      }
    }
  }
  // --- Hessian nonzeros owned by stage k ---
  auto add_h = [&](long long r, long long c, int pos) {
    int a = w_index(L, k, r), b = w_index(L, k, c);
    if (a < 0 || b < 0 || pos < 0) return false;
    if (a > b) std::swap(a, b);
    tg[{a, b}].push_back({pos, CX_ONE, CX_ONE});
    return true;
  };
  const auto& hci = pat.hci; const auto& hr = pat.hr;
  for (long long c = L.x_X(k); c < L.x_X(k) + 12; ++c)
    for (long long i = hci[c]; i < hci[c + 1]; ++i) if (!add_h(hr[i], c, seg_pos(3, i - L.hx(k)))) return -4;
  for (long long c = L.x_U(k); c < L.x_U(k) + 24; ++c)
    for (long long i = hci[c]; i < hci[c + 1]; ++i) {
      if (k > 0 && hr[i] >= L.x_U(k - 1) && hr[i] < L.x_U(k - 1) + 24) continue;   // (f_z of stage k-1, c_k): owned by stage k-1
      if (!add_h(hr[i], c, seg_pos(4, i - L.hu(k)))) return -5;
    }
  if (!last)
    for (long long c = L.x_U(k + 1); c < L.x_U(k + 1) + 12; ++c)
      for (long long i = hci[c]; i < hci[c + 1]; ++i)
        if (hr[i] >= L.x_U(k) && hr[i] < L.x_U(k) + 24) { if (!add_h(hr[i], c, seg_pos(5, i - L.hu(k + 1)))) return -6; }
  // --- constant Hessian entries of the running cost (segment 6 of cx, layout: RUNC) ---
  if (L.run_cost) {
    auto add_c = [&](int a, int b, int j) { tg[{a, b}].push_back({seg_pos(6, j), CX_ONE, CX_ONE}); };
    for (int i = 0; i < 12; ++i) add_c(i, i, i);                                  // (X_i, X_i)
    for (int l = 0; l < 4; ++l) for (int a = 0; a < 3; ++a) add_c(a, 12 + 3 * l + a, 12 + 3 * l + a);   // (pos_a, c_leg,a)
    for (int j = 0; j < 12; ++j) add_c(12 + j, 12 + j, 24 + j);                  // (c, c)
    for (int j = 0; j < 12; ++j) add_c(24 + j, 24 + j, 36 + j);                  // (f, f)
  }
  for (auto& kv : tg) {      // upper triangle (block_eliminate's tile fetch)
    const int ga = gpos(kv.first.first), gb = gpos(kv.first.second);
    dests.push_back({oG + 8 * (std::min(ga, gb) * GS + std::max(ga, gb)), false, kv.second});
  }
  for (int a = 0; a < 48; ++a) {
    if (gm[a].empty()) gm[a].push_back({0, CX_ONE, CX_ZERO});      // structural zero
    dests.push_back({oG + 8 * (gpos(a) * GS + G_GAMMA), false, gm[a]});
  }
  dests.insert(dests.end(), ah.begin(), ah.end());
  return 0;
}

// The tables of a horizon.  Assembly (ctab, read by asm_terms of the backward sweep): the terms of a stage type, destination behind destination, are cut into
// PIECES at every ch-th term (ch = ceil(n / 256) terms, the same for every type: where the 256 equal chunks of rounds 1-4 cut them).  A destination of one
// piece is summed and stored by one thread; the pieces of a longer one go to consecutive partial-sum slots and thread j adds up the slots of the j-th
// such destination (ccomb, asm_combine) -- every sum keeps the association it had, results stay bit-identical to the earlier kernels.  Pieces are
// spread over the 256 threads by longest-processing-time assignment, the lists padded with terms that add 0 to a closed sum to a multiple of ATAB_TB.
// Row products (rterm, read by row_products): the records of all inequality rows in row order, in 256 chunks of equal length moved to the next row border.
int build_tables(const Layout& L, SolverTables& T) {
  using namespace landing;
  const int N = L.N;
  Patterns pat;
  std::vector<long long> jci(L.nx + 1), jr(L.nnz_jac);
  pat.hci.resize(L.nx + 1); pat.hr.resize(L.nnz_hess); pat.rows.resize(L.ng);
  if (landing_pattern_jac(N, jci.data(), jr.data()) || landing_pattern_hess(N, pat.hci.data(), pat.hr.data())) return -1;
  for (long long c = 0; c < L.nx; ++c) for (long long i = jci[c]; i < jci[c + 1]; ++i) pat.rows[jr[i]].push_back({c, i});
  std::vector<std::vector<AsmDest>> types;
  std::vector<std::set<int>> where(N);      // structural nonzeros of G and A^ per stage, by their place
  std::vector<unsigned long long> rrec;
  T.ctype.assign(N, 0);
  for (int k = 0; k < N; ++k) {
    std::vector<AsmDest> dests;
    if (const int rc = stage_dests(L, k, pat, dests, rrec)) return rc;
    for (const AsmDest& D : dests) where[k].insert(D.d);
    const size_t id = std::find(types.begin(), types.end(), dests) - types.begin();
    if (id == types.size()) types.push_back(dests);
    T.ctype[k] = (int)id;
  }
  // the backward sweep visits k = N-1 .. 0 and only overwrites structural nonzeros in LDS: that needs the pattern of
  // stage k to contain the one of stage k+1 (true for this NLP: the last stage lacks the c+ block, all others agree)
  for (int k = N - 2; k >= 0; --k)
    if (!std::includes(where[k].begin(), where[k].end(), where[k + 1].begin(), where[k + 1].end())) return -8;
  std::vector<int> cnt(types.size(), 0);
  for (int id : T.ctype) cnt[id]++;
  T.c_mid = (int)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());

  const int oCx = (int)offsetof(Lds, jhl), oCarry = (int)offsetof(Lds, carry), oDump = (int)offsetof(Lds, dump);
  auto cx = [&](int pos) { return oCx + 8 * pos; };
  int ch = 0;
  for (const auto& dests : types) {
    size_t n = 0;
    for (const AsmDest& D : dests) n += D.terms.size();
    ch = std::max(ch, ((int)n + NTH - 1) / NTH);
  }
  struct Piece { std::vector<std::array<int, 3>> ops; int d = 0; bool ah = false; };
  std::vector<std::vector<std::vector<unsigned long long>>> lists(types.size(), std::vector<std::vector<unsigned long long>>(NTH));
  T.ccomb.assign(types.size() * (size_t)NTH, 0ull);
  for (size_t u = 0; u < types.size(); ++u) {
    std::vector<Piece> pieces;
    int nslot = 0, ncomb = 0, i = 0;
    for (const AsmDest& D : types[u]) {
      std::vector<Piece> cur(1);      // pieces of this destination
      for (const auto& t : D.terms) {
        if (i++ % ch == 0 && !cur.back().ops.empty()) cur.emplace_back();
        cur.back().ops.push_back(t);
      }
      if (cur.size() == 1) { cur[0].d = D.d; cur[0].ah = D.ah; pieces.push_back(cur[0]); continue; }
      if (cur.size() > 7 || nslot + (int)cur.size() > ASM_NSLOT || ncomb >= NTH) return -13;
      T.ccomb[u * NTH + ncomb++] = acomb_pack((int)cur.size(), oCarry + 8 * nslot, D.d, D.ah);
      for (auto& q : cur) { q.d = oCarry + 8 * nslot++; pieces.push_back(q); }
    }
    std::vector<int> order(pieces.size());
    for (size_t j = 0; j < order.size(); ++j) order[j] = (int)j;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return pieces[x].ops.size() > pieces[y].ops.size(); });
    std::vector<int> load(NTH, 0);
    for (int di : order) {
      const int l = (int)(std::min_element(load.begin(), load.end()) - load.begin());
      const Piece& q = pieces[di];
      for (size_t j = 0; j < q.ops.size(); ++j) {
        const bool lastt = j + 1 == q.ops.size();
        lists[u][l].push_back(aterm_pack(cx(q.ops[j][0]), cx(q.ops[j][1]), cx(q.ops[j][2]), lastt ? q.d : oDump + 8 * (l & 63), !lastt, lastt && q.ah));
      }
      load[l] += (int)q.ops.size();
    }
    T.c_ml = std::max(T.c_ml, *std::max_element(load.begin(), load.end()));
  }
  T.c_ml = (T.c_ml + ATAB_TB - 1) / ATAB_TB * ATAB_TB;
  if (T.c_ml > ATAB_LTMAX) return -10;
  T.ctab.assign(types.size() * (size_t)T.c_ml * NTH, 0ull);
  for (size_t u = 0; u < types.size(); ++u)
    for (int l = 0; l < NTH; ++l)
      for (int j = 0; j < T.c_ml; ++j)
        T.ctab[(u * T.c_ml + j) * NTH + l] = j < (int)lists[u][l].size() ? lists[u][l][j] : aterm_pack(cx(CX_ZERO), cx(CX_ONE), cx(CX_ONE), oDump + 8 * (l & 63), true, false);

  // row products: thread t takes the records [start[t], start[t + 1]), cut where a row closes
  const int n = (int)rrec.size();
  std::vector<int> start(NTH + 1, n);
  start[0] = 0;
  for (int t = 1; t < NTH; ++t) {
    int want = std::max((int)((long long)n * t / NTH), start[t - 1]);
    while (want < n && want > 0 && !((rrec[want - 1] >> 48) & 1ull)) ++want;
    start[t] = want;
  }
  for (int t = 0; t < NTH; ++t) T.rlen = std::max(T.rlen, start[t + 1] - start[t]);
  T.rterm.assign((size_t)T.rlen * NTH, 0ull);      // (0: not valid)
  for (int t = 0; t < NTH; ++t) for (int e = start[t]; e < start[t + 1]; ++e) T.rterm[(size_t)(e - start[t]) * NTH + t] = rrec[e];
  return 0;
}

}  // namespace

namespace landing {
// One solve is in flight per context at any time: the workspace (1.3 MB per member) and the tables belong to the context,
// not to a stream.  `done` is recorded behind every launch; the next launch makes ITS stream wait for it, and the
// workspace is only re-allocated after the event has completed.  Callers who want several batches in flight use one
// context per stream (tools/bench_pipeline.py).
int SolverWorkspace::ensure(const Layout& L, int B, hipStream_t stream) {
  if (!done && hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess) return -100;
  if (!d_ctab) {
    SolverTables T;
    const int rc = build_tables(L, T);
    if (rc) return rc;
    auto up = [](auto& dst, const auto& v) {
      if (dst.alloc(v.size()) != hipSuccess) return -100;
      if (hipMemcpy(dst.get(), v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice) != hipSuccess) return -101;
      return 0;
    };
    DevBuf<int> ctype;      // all filled before any is moved in: a failure leaves the workspace as it was
    DevBuf<unsigned long long> rterm, ctab, ccomb;
    int e = up(rterm, T.rterm);
    if (!e) e = up(ctype, T.ctype);
    if (!e) e = up(ctab, T.ctab);
    if (!e) e = up(ccomb, T.ccomb);
    if (e) return e;
    rlen = T.rlen; c_ml = T.c_ml; c_mid = T.c_mid;
    d_rterm = std::move(rterm); d_ctype = std::move(ctype); d_ccomb = std::move(ccomb);
    d_ctab = std::move(ctab);   // set last: d_ctab set <=> all tables are resident
  }
  const size_t need = (size_t)B * member_stride(L);
  if (buf.size() < need) {
    // an earlier launch (possibly on another stream) may still be using the old buffer
    if (hipEventSynchronize(done) != hipSuccess) return -102;
    if (buf.grow(need) != hipSuccess) return -100;
  }
  if (d_order.size() < (size_t)B) {
    if (hipEventSynchronize(done) != hipSuccess) return -102;
    if (d_order.grow((size_t)B) != hipSuccess) return -100;
  }
  // the previous solve of this context must have finished before this one touches the workspace
  if (hipStreamWaitEvent(stream, done, 0) != hipSuccess) return -102;
  return 0;
}
void SolverWorkspace::release() {      // (the blocks free themselves with the context)
  if (done) { (void)hipEventSynchronize(done); (void)hipEventDestroy(done); done = nullptr; }
}
}  // namespace landing

extern "C" {

// diagnostic: device pointer and member stride (in doubles) of the solver workspace of the last landing_solve_batch call
int landing_debug_workspace(landing_ctx* ctx, double** d_ws, unsigned long long* stride) {
  if (!ctx || !d_ws || !stride) return LANDING_E_ARG;
  *d_ws = ctx->ws.buf.get(); *stride = (unsigned long long)landing::member_stride(ctx->L);
  return 0;
}

// diagnostic: the tables the solver kernel reads, built (without a solve) when the context has none yet
int landing_debug_solver_tables(landing_ctx* ctx, int which, void* host_out, unsigned long long* n_bytes) {
  if (!ctx || which < 0 || which > 4 || !n_bytes) return fail(LANDING_E_ARG, "landing_debug_solver_tables: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lock(ctx->mu);
  landing::SolverWorkspace& ws = ctx->ws;
  const int rc = ws.ensure(ctx->L, 0, nullptr);
  if (rc) return fail(rc <= -100 ? LANDING_E_HIP : LANDING_E_ARG, "landing_debug_solver_tables: table setup failed (" + std::to_string(rc) + ")");
  const int scal[3] = {ws.c_ml, ws.c_mid, ws.rlen};
  const void* src[5] = {ws.d_ctab.get(), ws.d_ccomb.get(), ws.d_ctype.get(), ws.d_rterm.get(), scal};
  const size_t len[5] = {ws.d_ctab.size() * sizeof(*ws.d_ctab.get()), ws.d_ccomb.size() * sizeof(*ws.d_ccomb.get()), ws.d_ctype.size() * sizeof(*ws.d_ctype.get()),
                         ws.d_rterm.size() * sizeof(*ws.d_rterm.get()), sizeof(scal)};
  *n_bytes = len[which];
  if (host_out && which == 4) memcpy(host_out, scal, sizeof(scal));
  else if (host_out) HIP_TRY(hipMemcpy(host_out, src[which], len[which], hipMemcpyDeviceToHost));
  return 0;
}

int landing_solve_batch(landing_ctx* ctx, int B, const double* d_p, const double* d_x0, const landing_solver_opts* opts,
                        double* d_x, double* d_f, double* d_lam_g, int* d_status, int* d_iters, double* d_kkt, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || !d_p || !d_x0 || !d_x) return fail(LANDING_E_ARG, "landing_solve_batch: bad argument");
  if (ctx->L.N > landing::SOLVER_NMAX) return fail(LANDING_E_ARG, "landing_solve_batch: N <= 96 supported (the states of the forward sweep of one member live in LDS)");
  HIP_TRY(hipSetDevice(ctx->device));
  landing_solver_opts o;
  if (opts) o = *opts; else landing_solver_opts_default(&o);
  if (o.factor_fp32) {   // retired in round 5 (slower than the fp64 factor on every measurement): callers of rounds 2-4 that still set it keep working -- the fp64 factor runs, said once
    static std::atomic<bool> said{false};
    if (!said.exchange(true)) fprintf(stderr, "landing_solve_batch: factor_fp32 is retired (round 5); the fp64 factor runs instead\n");
  }
  if (!(o.kappa_eps > 0.0)) o.kappa_eps = ctx->L.run_cost ? 10.0 : 120.0;     // automatic choice by formulation (landing_nlp.h)
  if (!(o.theta_mu > 0.0)) o.theta_mu = ctx->L.run_cost ? 1.5 : 1.8;
  if (!(o.mu_init > 0.0)) o.mu_init = ctx->L.run_cost ? 0.1 : 0.5;           // likewise
  if (!(o.bound_push > 0.0)) o.bound_push = ctx->L.run_cost ? 0.5 : 1.0;
  std::lock_guard<std::mutex> lock(ctx->mu);      // contexts may be shared between host threads; launches are serialised
  const int rc = ctx->ws.ensure(ctx->L, B, (hipStream_t)stream);
  if (rc) return fail(rc <= -100 ? LANDING_E_HIP : LANDING_E_ARG, "landing_solve_batch: workspace/table setup failed (" + std::to_string(rc) + ")");
  landing::SolveArgs A;
  A.L = ctx->L; A.B = B; A.o = o; A.p = d_p; A.x0 = d_x0; A.x_out = d_x; A.f_out = d_f; A.lam_out = d_lam_g;
  A.status = d_status; A.iters = d_iters; A.kkt = d_kkt; A.ws = ctx->ws.buf.get(); A.ws_stride = landing::member_stride(ctx->L);
  A.ctab = ctx->ws.d_ctab.get(); A.ctype = ctx->ws.d_ctype.get(); A.c_ml = ctx->ws.c_ml; A.c_mid = ctx->ws.c_mid; A.ccomb = ctx->ws.d_ccomb.get();
  A.rterm = ctx->ws.d_rterm.get(); A.rlen = ctx->ws.rlen;
  A.prof = ctx->d_prof; A.iter_cap = ctx->iter_cap;
  A.edge_map = ctx->d_edge_map.get();
  A.order = nullptr;
  // hard-first order: pointless while every member is resident from the start (2 workgroups on each of the 256 CUs), and the
  // all-pairs ranking kernel is O(B^2) -- skipped for the huge batches of a data-generation job (ADVICE r2)
  if (o.dispatch_order && B > 512 && B <= 16384) {
    hipLaunchKernelGGL(landing::landing_order_kernel, dim3((B + landing::ORDER_THREADS - 1) / landing::ORDER_THREADS), dim3(landing::ORDER_THREADS), 0, (hipStream_t)stream, ctx->L, B, d_p, ctx->ws.d_order.get());
    A.order = ctx->ws.d_order.get();
  }
  hipLaunchKernelGGL(landing::landing_ipm_kernel, dim3(B), dim3(landing::SOLVER_THREADS), 0, (hipStream_t)stream, A);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(ctx->ws.done, (hipStream_t)stream));
  return 0;
}

// development aid: per-member phase timers [B][16] (see PH_* in solver_kernels.hip); pass NULL to disable
int landing_set_profile_buffer(landing_ctx* ctx, double* d_prof) {
  if (!ctx) return fail(LANDING_E_ARG, "landing_set_profile_buffer: bad argument");
  ctx->d_prof = d_prof;
  return 0;
}

// development aid: total iteration cap of every later solve of the context (SRBM and kinodynamic, phases included); 0 = the default
int landing_debug_iter_cap(landing_ctx* ctx, int cap) {
  if (!ctx || cap < 0) return fail(LANDING_E_ARG, "landing_debug_iter_cap: bad argument");
  std::lock_guard<std::mutex> lock(ctx->mu);
  ctx->iter_cap = cap;
  return 0;
}

int landing_solve_batch_host(landing_ctx* ctx, int B, const double* p, const double* x0, const landing_solver_opts* opts,
                             double* x, double* f, double* lam_g, int* status, int* iters, double* kkt) {
  if (!ctx || B <= 0 || !p || !x0 || !x) return fail(LANDING_E_ARG, "landing_solve_batch_host: bad argument");
  const Layout& L = ctx->L;
  HIP_TRY(hipSetDevice(ctx->device));
  // large host batches (what the mex gateway and the 21 / 25-argument entry points hand over in a data-generation job) go through the library's own stream:
  // chunks of 1024 on two lanes, copies under the solves, a workspace of 2 x 1024 members instead of B (stream_capi.inc; same results bit for bit)
  if (B > 2048 && !ctx->d_prof) return landing_solve_stream_host(ctx, B, 1024, 2, p, x0, opts, x, f, lam_g, status, iters, kkt);
  // copies and the launch go to a stream of the context (non-blocking: no implicit ordering against the null stream), so that
  // host threads driving different contexts -- also two contexts on ONE device, landing_multi_* -- really overlap
  { std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->host_stream) HIP_TRY(hipStreamCreateWithFlags(&ctx->host_stream, hipStreamNonBlocking)); }
  hipStream_t hs = ctx->host_stream;
  const size_t b = (size_t)B;
  Staging st(hs);
  const double* dp = st.in(p, b * L.np); const double* dx0 = st.in(x0, b * L.nx);
  double* dx = st.out(x, b * L.nx); double* df = st.out_always(f, b); double* dl = st.out_always(lam_g, b * L.ng); double* dk = st.out_always(kkt, b * 3);
  int* ds = st.out_always(status, b); int* di = st.out_always(iters, b);
  HIP_TRY(st.error());
  if (const int rc = landing_solve_batch(ctx, B, dp, dx0, opts, dx, df, dl, ds, di, dk, hs)) return rc;      // (st drains the stream before its blocks go)
  HIP_TRY(st.fetch());
  return 0;
}

// ---- the reference's 21-argument solver function (generate_landingCtrller_IPOPT.m:323-327), batched ------------------
int landing_pack_args21(int N, int B, const landing_args21* a, double* p) {
  if (N < 2 || B < 0 || !a || !p) return fail(LANDING_E_ARG, "landing_pack_args21: bad argument");
  const double* six[10] = {a->q_min, a->q_max, a->qd_min, a->qd_max, a->q_init, a->qd_init, a->q_term_min, a->q_term_max, a->qd_term_min, a->qd_term_max};
  const double* one[4] = {a->mu, a->l_leg_max, a->f_max, a->mass};
  if (!a->Xref || !a->dt || !a->QN || !a->Ib || !a->Ib_inv) return fail(LANDING_E_ARG, "landing_pack_args21: NULL argument");
  for (const double* q : six) if (!q) return fail(LANDING_E_ARG, "landing_pack_args21: NULL argument");
  for (const double* q : one) if (!q) return fail(LANDING_E_ARG, "landing_pack_args21: NULL argument");
  const Layout L = landing::make_layout(N);
  const size_t nX = 12 * (size_t)(N + 1);
  for (int b = 0; b < B; ++b) {       // Opti's order of the ACTIVE parameters (declaration order :51-75 without Uref; SURVEY row a2)
    double* q = p + (size_t)b * L.np;
    memcpy(q, a->Xref + b * nX, nX * sizeof(double));
    memcpy(q + L.o_dt, a->dt + (size_t)b * N, N * sizeof(double));
    for (int i = 0; i < 10; ++i) memcpy(q + L.o_q_min + 6 * i, six[i] + (size_t)b * 6, 6 * sizeof(double));
    memcpy(q + L.o_QN, a->QN + (size_t)b * 12, 12 * sizeof(double));
    q[L.o_mu] = a->mu[b]; q[L.o_l_leg_max] = a->l_leg_max[b]; q[L.o_f_max] = a->f_max[b]; q[L.o_mass] = a->mass[b];
    memcpy(q + L.o_Ib, a->Ib + (size_t)b * 3, 3 * sizeof(double));
    memcpy(q + L.o_Ib_inv, a->Ib_inv + (size_t)b * 3, 3 * sizeof(double));
  }
  return 0;
}

// ---- the 25-argument solver function of the reference's N=41 script (generate_quadruped_SRBM_CCC.m; call site analysis/eval_SRBM_CCC.m:72-78)
int landing_pack_args25(int N, int B, const landing_args25* a, double* p) {
  if (N < 2 || B < 0 || !a || !p) return fail(LANDING_E_ARG, "landing_pack_args25: bad argument");
  const double* six[10] = {a->q_min, a->q_max, a->qd_min, a->qd_max, a->q_init, a->qd_init, a->q_term_min, a->q_term_max, a->qd_term_min, a->qd_term_max};
  const double* one[4] = {a->mu, a->l_leg_max, a->f_max, a->mass};
  if (!a->Xref || !a->Uref || !a->dt || !a->QX || !a->QN || !a->Qc || !a->Qf || !a->Ib || !a->Ib_inv) return fail(LANDING_E_ARG, "landing_pack_args25: NULL argument");
  for (const double* q : six) if (!q) return fail(LANDING_E_ARG, "landing_pack_args25: NULL argument");
  for (const double* q : one) if (!q) return fail(LANDING_E_ARG, "landing_pack_args25: NULL argument");
  Layout L = landing::make_layout(N);
  landing::layout_ccc_params(L);
  const size_t nX = 12 * (size_t)(N + 1), nU = 24 * (size_t)N;
  for (int b = 0; b < B; ++b) {       // Opti's order of the ACTIVE parameters (declaration order :49-71 without c_init)
    double* q = p + (size_t)b * L.np;
    memcpy(q, a->Xref + b * nX, nX * sizeof(double));
    memcpy(q + L.o_Uref, a->Uref + b * nU, nU * sizeof(double));
    memcpy(q + L.o_dt, a->dt + (size_t)b * N, N * sizeof(double));
    for (int i = 0; i < 10; ++i) memcpy(q + L.o_q_min + 6 * i, six[i] + (size_t)b * 6, 6 * sizeof(double));
    memcpy(q + L.o_QX, a->QX + (size_t)b * 12, 12 * sizeof(double));
    memcpy(q + L.o_QN, a->QN + (size_t)b * 12, 12 * sizeof(double));
    memcpy(q + L.o_Qc, a->Qc + (size_t)b * 3, 3 * sizeof(double));
    memcpy(q + L.o_Qf, a->Qf + (size_t)b * 3, 3 * sizeof(double));
    q[L.o_mu] = a->mu[b]; q[L.o_l_leg_max] = a->l_leg_max[b]; q[L.o_f_max] = a->f_max[b]; q[L.o_mass] = a->mass[b];
    memcpy(q + L.o_Ib, a->Ib + (size_t)b * 3, 3 * sizeof(double));
    memcpy(q + L.o_Ib_inv, a->Ib_inv + (size_t)b * 3, 3 * sizeof(double));
  }
  return 0;
}

int landing_solve_args25(landing_ctx* ctx, int B, const landing_args25* a, const landing_solver_opts* opts,
                         double* x_star, double* f_star, double* lam_g, int* status, int* iters, double* kkt) {
  if (!ctx || B <= 0 || !a || !a->x0 || !x_star) return fail(LANDING_E_ARG, "landing_solve_args25: bad argument");
  if (ctx->L.run_cost != 2) return fail(LANDING_E_ARG, "landing_solve_args25: the context must be created with landing_form.run_cost = 2 (the N=41 script's parameter vector)");
  std::vector<double> p((size_t)B * ctx->L.np);
  const int rc = landing_pack_args25(ctx->L.N, B, a, p.data());
  if (rc) return rc;
  return landing_solve_batch_host(ctx, B, p.data(), a->x0, opts, x_star, f_star, lam_g, status, iters, kkt);
}

int landing_solve_args21(landing_ctx* ctx, int B, const landing_args21* a, const landing_solver_opts* opts,
                         double* x_star, double* f_star, int* status, int* iters, double* kkt) {
  if (!ctx || B <= 0 || !a || !a->x0 || !x_star) return fail(LANDING_E_ARG, "landing_solve_args21: bad argument");
  if (ctx->L.run_cost == 2) return fail(LANDING_E_ARG, "landing_solve_args21: this context takes the N=41 script's 25 arguments (landing_solve_args25)");
  std::vector<double> p((size_t)B * ctx->L.np);
  const int rc = landing_pack_args21(ctx->L.N, B, a, p.data());
  if (rc) return rc;
  return landing_solve_batch_host(ctx, B, p.data(), a->x0, opts, x_star, f_star, nullptr, status, iters, kkt);
}

int landing_solve_21(landing_ctx* ctx, int B, const double* Xref, const double* Uref, const double* dt,
                     const double* q_min, const double* q_max, const double* qd_min, const double* qd_max,
                     const double* q_init, const double* qd_init, const double* q_term_min, const double* q_term_max,
                     const double* qd_term_min, const double* qd_term_max, const double* QN, const double* x0,
                     const double* mu, const double* l_leg_max, const double* f_max, const double* mass,
                     const double* Ib, const double* Ib_inv, const landing_solver_opts* opts,
                     double* x_star, double* f_star, int* status, int* iters, double* kkt) {
  const landing_args21 a = {Xref, Uref, dt, q_min, q_max, qd_min, qd_max, q_init, qd_init, q_term_min, q_term_max,
                            qd_term_min, qd_term_max, QN, x0, mu, l_leg_max, f_max, mass, Ib, Ib_inv};
  return landing_solve_args21(ctx, B, &a, opts, x_star, f_star, status, iters, kkt);
}

// ---- SRBM variational linearisation + Riccati tracking gains (vbl_kernels.hip) ----------------------------------------
// the model and weight arguments the Riccati entry points share: checked, and the inertia, its inverse (adjugate) and 1/mass put into a.C
static int vbl_model(const char* who, const double* Ib3x3, double mass, const double* Q, const double* r_diag, landing::RdeArgs& a) {
  if (!Ib3x3 || !(mass > 0.0) || !Q || !r_diag) return fail(LANDING_E_ARG, std::string(who) + ": bad argument");
  const double* I = Ib3x3; double* J = a.C.Ibi;
  const double det = I[0] * (I[4] * I[8] - I[5] * I[7]) - I[1] * (I[3] * I[8] - I[5] * I[6]) + I[2] * (I[3] * I[7] - I[4] * I[6]);
  if (!(fabs(det) > 0.0)) return fail(LANDING_E_ARG, std::string(who) + ": singular inertia");
  J[0] = (I[4] * I[8] - I[5] * I[7]) / det; J[1] = (I[2] * I[7] - I[1] * I[8]) / det; J[2] = (I[1] * I[5] - I[2] * I[4]) / det;
  J[3] = (I[5] * I[6] - I[3] * I[8]) / det; J[4] = (I[0] * I[8] - I[2] * I[6]) / det; J[5] = (I[2] * I[3] - I[0] * I[5]) / det;
  J[6] = (I[3] * I[7] - I[4] * I[6]) / det; J[7] = (I[1] * I[6] - I[0] * I[7]) / det; J[8] = (I[0] * I[4] - I[1] * I[3]) / det;
  for (int i = 0; i < 9; ++i) a.C.Ib[i] = I[i];
  a.C.inv_m = 1.0 / mass;
  for (int i = 0; i < 12; ++i) if (!(r_diag[i] > 0.0)) return fail(LANDING_E_ARG, std::string(who) + ": R must be positive");
  return 0;
}

// uploads the weights and launches landing_rde_kernel on `stream`.  Call with ctx->mu held and the device selected; `a` is complete but for Q / F / rinv.
static int vbl_launch(landing_ctx* ctx, landing::RdeArgs& a, const double* Q, const double* r_diag, const double* F, hipStream_t stream) {
  constexpr size_t VBL_N = 576 + 576 + 12;
  if (!ctx->d_vbl) HIP_TRY(ctx->d_vbl.alloc(VBL_N));
  // The weights travel through a PINNED staging block owned by the context, so the upload is a true asynchronous copy and the call returns
  // without blocking the caller's stream (VERDICT r3 item 11: a stack buffer forced a hipStreamSynchronize here).  The block is re-written
  // by the next call only after the copy that read it has completed: `vbl_copied` is recorded behind the copy and waited for on the HOST
  // (normally long past -- the copy is 9 KB), never the kernel.
  if (!ctx->h_vbl) {      // event first, block second: a failure leaves the context as it was (h_vbl set <=> both exist)
    if (!ctx->vbl_copied) HIP_TRY(hipEventCreateWithFlags(&ctx->vbl_copied, hipEventDisableTiming));
    HIP_TRY(hipHostMalloc((void**)&ctx->h_vbl, VBL_N * sizeof(double), hipHostMallocDefault));
  } else HIP_TRY(hipEventSynchronize(ctx->vbl_copied));
  double* host = ctx->h_vbl;
  for (int i = 0; i < 576; ++i) { host[i] = Q[i]; host[576 + i] = F ? F[i] : 0.0; }
  for (int i = 0; i < 12; ++i) host[1152 + i] = 1.0 / r_diag[i];
  HIP_TRY(scratch_acquire(ctx, stream));      // the previous call's kernel (any stream) still reads Q / F / 1/R from the device block
  HIP_TRY(hipMemcpyAsync(ctx->d_vbl.get(), host, VBL_N * sizeof(double), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipEventRecord(ctx->vbl_copied, stream));
  a.Q = ctx->d_vbl.get(); a.F = a.Q + 576; a.rinv = a.Q + 1152;
  hipLaunchKernelGGL(landing::landing_rde_kernel, dim3(a.B), dim3(256), 0, stream, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(scratch_release(ctx, stream));
  return 0;
}

int landing_riccati_gains_batch(landing_ctx* ctx, int B, int n, const double* d_xref, const double* d_fref,
                                const double* Ib3x3, double mass, const double* Q, const double* r_diag, const double* F,
                                double dt, int rk4, double* d_P, double* d_K, double* d_A, double* d_B, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || n < 1 || !d_xref || !d_fref) return fail(LANDING_E_ARG, "landing_riccati_gains_batch: bad argument");
  landing::RdeArgs a;
  a.B = B; a.n = n; a.rk4 = rk4 ? 1 : 0; a.dt = dt; a.xref = d_xref; a.fref = d_fref; a.P = d_P; a.K = d_K; a.Aout = d_A; a.Bout = d_B;
  if (const int rc = vbl_model("landing_riccati_gains_batch", Ib3x3, mass, Q, r_diag, a)) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  std::lock_guard<std::mutex> lock(ctx->mu);
  return vbl_launch(ctx, a, Q, r_diag, F, (hipStream_t)stream);
}

// ---- receding-horizon shift of a solved batch (landing_mpc_shift_kernel) ---------------------------------------------------
int landing_mpc_shift(landing_ctx* ctx, int B, const double* d_x_prev, const double* d_state, double* d_p, double* d_x0, void* stream) {
  if (ctx && B == 0) return 0;
  if (!ctx || B < 0 || !d_x_prev || !d_state || !d_p || !d_x0 || d_x_prev == d_x0) return fail(LANDING_E_ARG, "landing_mpc_shift: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t n = (size_t)B * ctx->L.nx;
  hipLaunchKernelGGL(landing::landing_mpc_shift_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctx->L, B, d_x_prev, d_state, d_p, d_x0);
  HIP_TRY(hipGetLastError());
  return 0;
}

}  // extern "C"
