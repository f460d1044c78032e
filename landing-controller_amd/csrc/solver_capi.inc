// solver_capi.inc -- host side of landing_solve_batch (included by capi.hip): assembly tables built
// from the CCS patterns, workspace management, launch.  No CPU solve path exists here.
//
// Assembly tables.  The solver kernel consumes the SAME CCS nonzeros the function layer emits
// (casadi_s5 / casadi_s4 order).  For every stage k the host precomputes, from the patterns, how the
// stage's nonzeros combine into the condensed stage block
//     G_k = H_k + J_d^T Sigma J_d   (48x48 over w = [X_k(12) c_k(12) f_k(12) c_{k+1}(12)])
// the barrier gradient gamma_k = J_d^T rho, the dynamics block A^ = -dg_dyn/d(X_k,c_k,f_k) (12x36, rows in
// state order) and the row-major products J_d w.  Identical tables are de-duplicated (first / middle /
// penultimate / last stage), so the table data stays L1/L2 resident.

namespace {

struct StageTab {
  std::vector<int> tg_ab, tg_start, tg_term, gm_start, gm_term, a_term, r_start, r_term;
  int nu;
  // not part of the de-duplicated table: member-global flat term lists (see build_tables)
  std::vector<std::array<int, 4>> cterm;   // {row (global; -1: Hessian entry; -2: negated Jacobian entry), i1, i2 (-1: rho term), dst}
  std::vector<std::array<int, 4>> rterm;   // {jac index, x index, dst row (-1: more terms follow), 0}
  std::vector<unsigned long long> cloc;    // condensation terms in stage-local packed form (landing::cterm_pack); identical for stages of one type
  bool operator==(const StageTab& o) const {
    return nu == o.nu && tg_ab == o.tg_ab && tg_start == o.tg_start && tg_term == o.tg_term && gm_start == o.gm_start &&
           gm_term == o.gm_term && a_term == o.a_term && r_start == o.r_start && r_term == o.r_term && cloc == o.cloc;
  }
};

// w-index of global variable c relative to stage k, or -1 (X_{k+1} / unrelated)
int w_index(const Layout& L, int k, long long c) {
  const int N = L.N;
  if (c >= L.x_X(k) && c < L.x_X(k) + 12) return (int)(c - L.x_X(k));
  if (c >= L.x_U(k) && c < L.x_U(k) + 24) { const int j = (int)(c - L.x_U(k)); return j < 12 ? 12 + j : 24 + (j - 12); }
  if (k < N - 1 && c >= L.x_U(k + 1) && c < L.x_U(k + 1) + 12) return 36 + (int)(c - L.x_U(k + 1));
  return -1;
}
// position of Jacobian nonzero idx (column c) in the stage-k staging buffer, or -1
int jpos(const Layout& L, int k, long long c, long long idx) {
  if (c >= L.x_X(k) && c < L.x_X(k) + 12) return landing::NZ_JX + (int)(idx - L.jx(k));
  if (c >= L.x_U(k) && c < L.x_U(k) + 24) return landing::NZ_JU + (int)(idx - L.ju(k));
  if (k < L.N - 1 && c >= L.x_U(k + 1) && c < L.x_U(k + 1) + 12) return landing::NZ_JUN + (int)(idx - L.ju(k + 1));
  return -1;
}

// stage-local encoding of an index into the member's [J | H | Hc] array: segment (landing::SEG_*) and offset inside it
bool encode_jh(const Layout& L, int k, int idx, int& seg, int& off) {
  const int nj = L.nnz_jac, nh = L.nnz_hess, N = L.N;
  struct R { int base, len; };
  const R r[7] = {{L.jx(k), 157}, {L.ju(k), L.ju_len(k)}, {k < N - 1 ? L.ju(k + 1) : -1, k < N - 1 ? L.ju_len(k + 1) : 0},
                  {nj + L.hx(k), 29}, {nj + L.hu(k), k == 0 ? 148 : 160}, {k < N - 1 ? nj + L.hu(k + 1) : -1, k < N - 1 ? 160 : 0},
                  {nj + nh + k * landing::RUNC, landing::RUNC}};
  for (int q = 0; q < 7; ++q) if (r[q].base >= 0 && idx >= r[q].base && idx < r[q].base + r[q].len) { seg = q; off = idx - r[q].base; return off < 256; }
  return false;
}

int build_tables(const Layout& L, std::vector<int>& data, std::vector<int>& stage_tab,
                 std::vector<int>& rterms, std::vector<int>& rstart,
                 std::vector<unsigned long long>& ctab, std::vector<unsigned long long>& ccomb, std::vector<int>& ctype, int& c_ml, int& c_mid) {
  const int N = L.N;
  std::vector<long long> jci(L.nx + 1), jr(L.nnz_jac), hci(L.nx + 1), hr(L.nnz_hess);
  if (landing_pattern_jac(N, jci.data(), jr.data()) || landing_pattern_hess(N, hci.data(), hr.data())) return -1;
  // row-major view of J
  std::vector<std::vector<std::pair<long long, long long>>> rows(L.ng);  // (col, idx)
  for (long long c = 0; c < L.nx; ++c) for (long long i = jci[c]; i < jci[c + 1]; ++i) rows[jr[i]].push_back({c, i});
  std::vector<StageTab> uniq;
  stage_tab.assign(N, 0);
  std::vector<int> which(N);
  std::vector<std::set<int>> pat_g(N), pat_a(N);   // structural nonzeros of the condensed G / of A^ per stage
  for (int k = 0; k < N; ++k) {
    StageTab T;
    const bool last = (k == N - 1);
    T.nu = last ? 12 : 24;
    const int nr = L.rows(k), g0 = L.g_stage(k);
    std::map<std::pair<int, int>, std::vector<std::array<int, 3>>> tg;   // (a,b) -> terms
    std::map<int, int> pos2idx;            // staging position -> index into the member's [J | H] nonzeros
    std::vector<std::vector<std::array<int, 2>>> gm(48);
    T.r_start.assign(105, 0);
    // --- Jacobian rows ---
    for (int q = 0; q < nr; ++q) {
      std::vector<std::array<int, 2>> ent;   // (w index, pos)
      std::vector<std::array<int, 2>> entg;  // (global jac index, global x index), same order
      for (auto& ci : rows[g0 + q]) {
        const int a = w_index(L, k, ci.first), pos = jpos(L, k, ci.first, ci.second);
        if (a < 0) continue;                 // X_{k+1} identity
        if (pos < 0) return -2;
        ent.push_back({a, pos});
        entg.push_back({(int)ci.second, (int)ci.first});
        pos2idx[pos] = (int)ci.second;
      }
      if (q >= 12) for (size_t i = 0; i < entg.size(); ++i)
        T.rterm.push_back({entg[i][0], entg[i][1], i + 1 == entg.size() ? g0 + q : -1, 0});
      if (q < 12) {                          // dynamics rows -> A^ (state order)
        const int sr = q < 6 ? q : (q < 9 ? q + 3 : q - 3);
        for (auto& e : ent) { if (e[0] >= 36) return -3; T.a_term.push_back(e[1]); T.a_term.push_back(sr); T.a_term.push_back(e[0]); }
      } else {                               // inequality rows
        for (size_t i = 0; i < ent.size(); ++i) {
          gm[ent[i][0]].push_back({q, ent[i][1]});
          T.r_term.push_back(ent[i][1]); T.r_term.push_back(ent[i][0]);
          for (size_t j = i; j < ent.size(); ++j) {
            int a = ent[i][0], b = ent[j][0], pa = ent[i][1], pb = ent[j][1];
            if (a > b) { std::swap(a, b); std::swap(pa, pb); }
            tg[{a, b}].push_back({q, pa, pb});
          }
        }
      }
      T.r_start[q + 1] = (int)T.r_term.size() / 2;
    }
    for (int q = nr; q < 104; ++q) T.r_start[q + 1] = T.r_start[nr];
    // --- Hessian nonzeros owned by stage k ---
    auto add_h = [&](long long r, long long c, long long idx, int pos) {
      int a = w_index(L, k, r), b = w_index(L, k, c);
      if (a < 0 || b < 0) return false;
      if (a > b) std::swap(a, b);
      tg[{a, b}].push_back({-1, pos, 0});
      pos2idx[pos] = L.nnz_jac + (int)idx;
      return true;
    };
    for (long long c = L.x_X(k); c < L.x_X(k) + 12; ++c)
      for (long long i = hci[c]; i < hci[c + 1]; ++i) if (!add_h(hr[i], c, i, landing::NZ_HX + (int)(i - L.hx(k)))) return -4;
    for (long long c = L.x_U(k); c < L.x_U(k) + 24; ++c)
      for (long long i = hci[c]; i < hci[c + 1]; ++i) {
        if (k > 0 && hr[i] >= L.x_U(k - 1) && hr[i] < L.x_U(k - 1) + 24) continue;   // (f_z of stage k-1, c_k): owned by stage k-1
        if (!add_h(hr[i], c, i, landing::NZ_HU + (int)(i - L.hu(k)))) return -5;
      }
    if (!last)
      for (long long c = L.x_U(k + 1); c < L.x_U(k + 1) + 12; ++c)
        for (long long i = hci[c]; i < hci[c + 1]; ++i)
          if (hr[i] >= L.x_U(k) && hr[i] < L.x_U(k) + 24) { if (!add_h(hr[i], c, i, landing::NZ_HUN + (int)(i - L.hu(k + 1)))) return -6; }
    // --- constant Hessian entries of the running cost (stored behind the Hessian nonzeros, RUNC per stage) ---
    if (L.run_cost) {
      auto add_c = [&](int a, int b, int j) {
        const int pos = 100000 + j;
        tg[{a, b}].push_back({-1, pos, 0});
        pos2idx[pos] = L.nnz_jac + L.nnz_hess + k * landing::RUNC + j;
      };
      for (int i = 0; i < 12; ++i) add_c(i, i, i);                                  // (X_i, X_i)
      for (int l = 0; l < 4; ++l) for (int a = 0; a < 3; ++a) add_c(a, 12 + 3 * l + a, 12 + 3 * l + a);   // (pos_a, c_leg,a)
      for (int j = 0; j < 12; ++j) add_c(12 + j, 12 + j, 24 + j);                  // (c, c)
      for (int j = 0; j < 12; ++j) add_c(24 + j, 24 + j, 36 + j);                  // (f, f)
    }
    // --- flatten ---
    T.tg_start.push_back(0);
    for (auto& kv : tg) {
      T.tg_ab.push_back(kv.first.first | (kv.first.second << 8));
      for (auto& t : kv.second) { T.tg_term.push_back(t[0]); T.tg_term.push_back(t[1]); T.tg_term.push_back(t[2]); }
      T.tg_start.push_back((int)T.tg_term.size() / 3);
    }
    T.gm_start.push_back(0);
    for (int a = 0; a < 48; ++a) {
      for (auto& t : gm[a]) { T.gm_term.push_back(t[0]); T.gm_term.push_back(t[1]); }
      T.gm_start.push_back((int)T.gm_term.size() / 2);
    }
    // member-global condensation terms of this stage: targets, gamma, A^ (destinations k*COND_STRIDE + slot)
    {
      const int base = k * landing::COND_STRIDE;
      if ((int)T.tg_ab.size() > landing::COND_GAM || (int)T.a_term.size() / 3 > landing::COND_STRIDE - landing::COND_AH) return -7;
      int slot = 0;
      for (auto& kv : tg) {
        for (size_t i = 0; i < kv.second.size(); ++i) {
          const auto& t = kv.second[i];
          const int dst = (i + 1 == kv.second.size()) ? base + slot : -1;
          if (t[0] < 0) T.cterm.push_back({-1, pos2idx.at(t[1]), -1, dst});
          else T.cterm.push_back({g0 + t[0], pos2idx.at(t[1]), pos2idx.at(t[2]), dst});
        }
        ++slot;
      }
      for (int a = 0; a < 48; ++a) {
        if (gm[a].empty()) { T.cterm.push_back({-3, 0, -1, base + landing::COND_GAM + a}); continue; }   // structural zero
        for (size_t i = 0; i < gm[a].size(); ++i)
          T.cterm.push_back({g0 + gm[a][i][0], pos2idx.at(gm[a][i][1]), -1, (i + 1 == gm[a].size()) ? base + landing::COND_GAM + a : -1});
      }
      for (size_t i = 0; i < T.a_term.size() / 3; ++i) T.cterm.push_back({-2, pos2idx.at(T.a_term[3 * i]), -1, base + landing::COND_AH + (int)i});
    }
    for (auto& t : T.cterm) {   // stage-local packed form of the same terms
      int sa = 0, oa = 0, sb = 0, ob = 0;
      const bool has_b = t[2] >= 0;
      if (t[0] != -3 && !encode_jh(L, k, t[1], sa, oa)) return -9;
      if (has_b && !encode_jh(L, k, t[2], sb, ob)) return -9;
      const int rtype = t[0] >= 0 ? 0 : (t[0] == -1 ? 1 : (t[0] == -2 ? 2 : 3));
      const int rowq = t[0] >= 0 ? t[0] - g0 : 0;
      if (rowq < 0 || rowq >= 128) return -9;
      const int dstl = t[3] >= 0 ? t[3] - k * landing::COND_STRIDE : 0;
      if (dstl < 0 || dstl >= 1024) return -9;
      T.cloc.push_back(landing::cterm_pack(sa, oa, sb, ob, has_b, rowq, rtype, dstl, t[3] >= 0));
    }
    for (int ab : T.tg_ab) pat_g[k].insert(ab);
    for (size_t i = 0; i < T.a_term.size() / 3; ++i) pat_a[k].insert(T.a_term[3 * i + 1] * 64 + T.a_term[3 * i + 2]);
    for (auto& t : T.rterm) { rterms.push_back(t[0]); rterms.push_back(t[1]); rterms.push_back(t[2]); rterms.push_back(t[3]); }
    T.cterm.clear(); T.rterm.clear();
    int id = -1;
    for (size_t u = 0; u < uniq.size(); ++u) if (uniq[u] == T) { id = (int)u; break; }
    if (id < 0) { id = (int)uniq.size(); uniq.push_back(T); }
    which[k] = id;
  }
  // the backward sweep visits k = N-1 .. 0 and only overwrites structural nonzeros in LDS: that needs the pattern of
  // stage k to contain the one of stage k+1 (true for this NLP: the last stage lacks the c+ block, all others agree)
  int zero_each = 0;
  for (int k = N - 2; k >= 0; --k)
    if (!std::includes(pat_g[k].begin(), pat_g[k].end(), pat_g[k + 1].begin(), pat_g[k + 1].end()) ||
        !std::includes(pat_a[k].begin(), pat_a[k].end(), pat_a[k + 1].begin(), pat_a[k + 1].end())) zero_each = 1;
  if (zero_each) return -8;     // cannot happen for this NLP family; the kernel relies on the nesting
  // --- serialise: header of 16 ints per table, then the arrays ---
  data.clear();
  std::vector<int> off(uniq.size());
  for (size_t u = 0; u < uniq.size(); ++u) {
    const StageTab& T = uniq[u];
    off[u] = (int)data.size();
    const int h = (int)data.size();
    data.resize(data.size() + 16, 0);
    auto put = [&](const std::vector<int>& v) { const int o = (int)data.size(); data.insert(data.end(), v.begin(), v.end()); return o; };
    data[h + 0] = (int)T.tg_ab.size();
    data[h + 1] = put(T.tg_ab); data[h + 2] = put(T.tg_start); data[h + 3] = put(T.tg_term);
    data[h + 4] = put(T.gm_start); data[h + 5] = put(T.gm_term);
    data[h + 6] = (int)T.a_term.size() / 3; data[h + 7] = put(T.a_term);
    data[h + 8] = put(T.r_start); data[h + 9] = put(T.r_term);
    data[h + 10] = T.nu;
    data[h + 11] = zero_each;
  }
  for (int k = 0; k < N; ++k) stage_tab[k] = off[which[k]];
  // Assembly tables, one per stage type (landing::aterm_pack, read by asm_terms of the backward sweep), every place given as a byte
  // offset inside the kernel's LDS block.  The terms of a destination are cut into PIECES where the 256 equal chunks of rounds 1-4
  // cut them (chunk = ceil(n / 256) terms, the same for every type): a destination of one piece is summed and stored by one thread;
  // the pieces of a longer one go to consecutive partial-sum slots and thread j adds up the slots of the j-th such destination
  // (landing::acomb_pack, asm_combine) -- every sum keeps the association it had, results stay bit-identical to the earlier kernels.
  // Pieces are spread over the 256 threads by longest-processing-time assignment; list [entry j][thread], padded with terms that add
  // 0 to a closed sum; the length is a multiple of ATAB_TB.
  {
    using landing::Lds;
    const int NTH = landing::SOLVER_THREADS;
    const int oG = (int)offsetof(Lds, G), oAh = (int)offsetof(Lds, Ah), oCx = (int)offsetof(Lds, jhl), oCarry = (int)offsetof(Lds, carry), oDump = (int)offsetof(Lds, dump);
    auto cx = [&](int pos) { return oCx + 8 * pos; };
    // G in elimination order, the same for every stage type: (sigma, f, c+) -> rows / columns (f, c+, sigma); gamma is its spare column
    auto gpos = [](int a) { return a < 24 ? a + 24 : a - 24; };
    int ch = 0;
    for (size_t u = 0; u < uniq.size(); ++u) ch = std::max(ch, ((int)uniq[u].cloc.size() + NTH - 1) / NTH);
    struct Piece { std::vector<std::array<int, 3>> ops; int d; bool ah; };
    std::vector<std::vector<std::vector<unsigned long long>>> lists(uniq.size(), std::vector<std::vector<unsigned long long>>(NTH));
    ccomb.assign(uniq.size() * (size_t)NTH, 0ull);
    c_ml = 0;
    for (size_t u = 0; u < uniq.size(); ++u) {
      const StageTab& T = uniq[u];
      const auto& v = T.cloc; const int n = (int)v.size();
      if (n == 0 || !landing::cterm_closes(v[n - 1])) return -11;
      std::vector<Piece> pieces, cur;      // all pieces; pieces of the open destination
      int nslot = 0, ncomb = 0;
      Piece pc_; pc_.d = 0; pc_.ah = false;
      for (int i = 0; i < n; ++i) {
        const unsigned lo = (unsigned)v[i], hi = (unsigned)(v[i] >> 32);
        const int pa = (int)(lo & 2047u), pb0 = (int)((lo >> 11) & 2047u), rowq = (int)((lo >> 23) & 127u), rtype = (int)(lo >> 30), dst = (int)(hi & 1023u);
        const bool has_b = (lo >> 22) & 1u, closes = landing::cterm_closes(v[i]);
        const int pb = has_b ? pb0 : landing::CX_ONE;
        const int pc = rtype == 0 ? landing::CX_SR + rowq + (has_b ? 0 : 104) : (rtype == 1 ? landing::CX_ONE : (rtype == 2 ? landing::CX_MONE : landing::CX_ZERO));
        if (i % ch == 0 && !pc_.ops.empty()) { cur.push_back(pc_); pc_.ops.clear(); }      // chunk border inside a destination
        pc_.ops.push_back({cx(pa), cx(pb), cx(pc)});
        if (!closes) continue;
        int d; bool ah = false;
        if (dst < landing::COND_GAM) {
          if (dst >= (int)T.tg_ab.size()) return -12;
          const int a0 = T.tg_ab[dst] & 255, b0 = T.tg_ab[dst] >> 8;
          if (a0 >= 48 || b0 >= 48) return -12;
          d = oG + 8 * (std::min(gpos(a0), gpos(b0)) * landing::GS + std::max(gpos(a0), gpos(b0)));      // upper triangle (block_eliminate's tile fetch)
        } else if (dst < landing::COND_AH) d = oG + 8 * (gpos(dst - landing::COND_GAM) * landing::GS + landing::G_GAMMA);
        else {
          const int q = dst - landing::COND_AH;
          if (3 * q + 2 >= (int)T.a_term.size()) return -12;
          d = oAh + 8 * (T.a_term[3 * q + 1] * landing::YS + T.a_term[3 * q + 2]); ah = true;
        }
        cur.push_back(pc_); pc_.ops.clear();
        if (cur.size() == 1) { cur[0].d = d; cur[0].ah = ah; pieces.push_back(cur[0]); }
        else {
          if (cur.size() > 7 || nslot + (int)cur.size() > landing::ASM_NSLOT || ncomb >= NTH) return -13;
          ccomb[u * NTH + ncomb++] = landing::acomb_pack((int)cur.size(), oCarry + 8 * nslot, d, ah);
          for (auto& q : cur) { q.d = oCarry + 8 * nslot; q.ah = false; ++nslot; pieces.push_back(q); }
        }
        cur.clear();
      }
      std::vector<int> order(pieces.size());
      for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
      std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return pieces[x].ops.size() > pieces[y].ops.size(); });
      std::vector<int> load(NTH, 0);
      for (int di : order) {
        const int l = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        const Piece& q = pieces[di];
        for (size_t i = 0; i < q.ops.size(); ++i) {
          const bool lastt = i + 1 == q.ops.size();
          lists[u][l].push_back(landing::aterm_pack(q.ops[i][0], q.ops[i][1], q.ops[i][2], lastt ? q.d : oDump + 8 * (l & 63), !lastt, lastt && q.ah));
        }
        load[l] += (int)q.ops.size();
      }
      c_ml = std::max(c_ml, *std::max_element(load.begin(), load.end()));
    }
    c_ml = (c_ml + landing::ATAB_TB - 1) / landing::ATAB_TB * landing::ATAB_TB;
    if (c_ml > landing::ATAB_LTMAX) return -10;
    ctab.assign(uniq.size() * (size_t)c_ml * NTH, 0ull);
    for (size_t u = 0; u < uniq.size(); ++u)
      for (int l = 0; l < NTH; ++l)
        for (int j = 0; j < c_ml; ++j)
          ctab[(u * c_ml + j) * NTH + l] = j < (int)lists[u][l].size() ? lists[u][l][j]
                                           : landing::aterm_pack(cx(landing::CX_ZERO), cx(landing::CX_ONE), cx(landing::CX_ONE), oDump + 8 * (l & 63), true, false);
    ctype.assign(N, 0);
    std::vector<int> cnt(uniq.size(), 0);
    for (int k = 0; k < N; ++k) { ctype[k] = which[k]; cnt[which[k]]++; }
    c_mid = (int)(std::max_element(cnt.begin(), cnt.end()) - cnt.begin());
  }
  // contiguous per-thread chunks of the flat term lists, cut at destination boundaries
  auto chunk_at = [](const std::vector<int>& terms, int dstcol, std::vector<int>& start) {
    const int n = (int)terms.size() / 4, NTH = landing::SOLVER_THREADS;
    start.assign(NTH + 1, n);
    start[0] = 0;
    for (int t = 1; t < NTH; ++t) {
      int want = (int)((long long)n * t / NTH);
      if (want < start[t - 1]) want = start[t - 1];
      while (want < n && want > 0 && terms[4 * (want - 1) + dstcol] < 0) ++want;   // previous term must close its destination
      start[t] = want;
    }
  };
  chunk_at(rterms, 2, rstart);
  // interleave: entry j of thread t at [j * NTH + t] (coalesced 16-byte loads), padded to the longest chunk
  auto interleave = [](std::vector<int>& terms, std::vector<int>& start, const std::array<int, 4>& pad) {
    const int NTH = landing::SOLVER_THREADS;
    int maxlen = 0;
    for (int t = 0; t < NTH; ++t) maxlen = std::max(maxlen, start[t + 1] - start[t]);
    std::vector<int> out((size_t)maxlen * NTH * 4);
    for (int j = 0; j < maxlen; ++j) for (int t = 0; t < NTH; ++t) {
      const int e = start[t] + j;
      for (int q = 0; q < 4; ++q) out[((size_t)j * NTH + t) * 4 + q] = (e < start[t + 1]) ? terms[4 * (size_t)e + q] : pad[q];
    }
    terms.swap(out);
    start.assign(1, maxlen);
  };
  for (size_t i = 0; i < rterms.size() / 4; ++i) rterms[4 * i + 3] = 1;      // valid flag
  interleave(rterms, rstart, {0, 0, -1, 0});
  {   // pack the interleaved records into 8 bytes: jac index | x index << 16 | dst row << 32 | closes << 48 | valid << 49
    const size_t n = rterms.size() / 4;
    std::vector<int> packed(2 * n);
    for (size_t i = 0; i < n; ++i) {
      const int ij = rterms[4 * i], ix = rterms[4 * i + 1], ir = rterms[4 * i + 2], valid = rterms[4 * i + 3];
      if (ij < 0 || ij > 0xffff || ix < 0 || ix > 0xffff || ir > 0xffff) return -18;
      const unsigned long long rec = (unsigned long long)ij | ((unsigned long long)ix << 16) | ((unsigned long long)(ir >= 0 ? ir : 0) << 32) |
                                     ((unsigned long long)(ir >= 0 ? 1 : 0) << 48) | ((unsigned long long)(valid ? 1 : 0) << 49);
      memcpy(&packed[2 * i], &rec, 8);
    }
    rterms.swap(packed);
  }
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
  if (!d_tab) {
    std::vector<int> data, st, rt, rs, cty;
    std::vector<unsigned long long> ctb, ccb;
    const int rc = build_tables(L, data, st, rt, rs, ctb, ccb, cty, c_ml, c_mid);
    if (rc) return rc;
    n_tab = (int)data.size();
    rlen = rs[0];
    auto up = [](auto& dst, const auto& v) {
      if (dst.alloc(v.size()) != hipSuccess) return -100;
      if (hipMemcpy(dst.get(), v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice) != hipSuccess) return -101;
      return 0;
    };
    DevBuf<int> rterm, stage_tab, ctype, tab;      // all filled before any is moved in: a failure leaves the workspace as it was
    DevBuf<unsigned long long> ctab, ccomb;
    int e = up(rterm, rt);
    if (!e) e = up(stage_tab, st);
    if (!e) e = up(ctype, cty);
    if (!e) e = up(ctab, ctb);
    if (!e) e = up(ccomb, ccb);
    if (!e) e = up(tab, data);
    if (e) return e;
    d_rterm = std::move(rterm); d_stage_tab = std::move(stage_tab); d_ctype = std::move(ctype); d_ctab = std::move(ctab); d_ccomb = std::move(ccomb);
    d_tab = std::move(tab);   // set last: d_tab set <=> all tables are resident
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
  A.rterm = (const unsigned long long*)ctx->ws.d_rterm.get(); A.rlen = ctx->ws.rlen;
  A.prof = ctx->d_prof;
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
  DevBuf<double> dp, dx0, dx, df, dl, dk;
  DevBuf<int> dsi;          // status | iters
  HIP_TRY(dp.alloc(b * L.np)); HIP_TRY(dx0.alloc(b * L.nx)); HIP_TRY(dx.alloc(b * L.nx)); HIP_TRY(df.alloc(b));
  HIP_TRY(dl.alloc(b * L.ng)); HIP_TRY(dk.alloc(b * 3)); HIP_TRY(dsi.alloc(2 * b));
  int* ds = dsi.get(); int* di = ds + b;
  HIP_TRY(hipMemcpyAsync(dp.get(), p, b * L.np * 8, hipMemcpyHostToDevice, hs));
  HIP_TRY(hipMemcpyAsync(dx0.get(), x0, b * L.nx * 8, hipMemcpyHostToDevice, hs));
  int rc = landing_solve_batch(ctx, B, dp.get(), dx0.get(), opts, dx.get(), df.get(), dl.get(), ds, di, dk.get(), hs);
  if (rc == 0 && hipStreamSynchronize(hs) != hipSuccess) rc = fail(LANDING_E_HIP, "landing_solve_batch_host: kernel failed");
  if (rc) { (void)hipStreamSynchronize(hs); return rc; }
  HIP_TRY(hipMemcpyAsync(x, dx.get(), b * L.nx * 8, hipMemcpyDeviceToHost, hs));
  if (f) HIP_TRY(hipMemcpyAsync(f, df.get(), b * 8, hipMemcpyDeviceToHost, hs));
  if (lam_g) HIP_TRY(hipMemcpyAsync(lam_g, dl.get(), b * L.ng * 8, hipMemcpyDeviceToHost, hs));
  if (status) HIP_TRY(hipMemcpyAsync(status, ds, b * sizeof(int), hipMemcpyDeviceToHost, hs));
  if (iters) HIP_TRY(hipMemcpyAsync(iters, di, b * sizeof(int), hipMemcpyDeviceToHost, hs));
  if (kkt) HIP_TRY(hipMemcpyAsync(kkt, dk.get(), b * 3 * 8, hipMemcpyDeviceToHost, hs));
  HIP_TRY(hipStreamSynchronize(hs));
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
  HIP_TRY(hipSetDevice(ctx->device));
  landing::KdNlpArgs a;
  a.sx = a.sg = a.sj = a.sh = 0; a.skip = nullptr;
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N; a.x = d_x; a.g = d_g; a.jac = d_jac; a.lam = nullptr; a.hess = nullptr;
  for (int k = 0; k < 64; ++k) a.P.dt[k] = k < N ? prm->dt[k] : 0.0;
  a.P.mass = prm->mass; a.P.mu = prm->mu; a.P.std_base = ctx->rbd_std_base;
  for (int i = 0; i < 3; ++i) { a.P.Ib[i] = prm->Ib[i]; a.P.Ibi[i] = prm->Ib_inv[i]; }
  if (d_g) {
    const long long n = (long long)B * N;
    hipLaunchKernelGGL(landing::landing_kinodyn_nlp_g_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, a);
  }
  if (d_jac) {
    const long long n = (long long)B * N * landing::KD_NW;
    kd_launch_jac(ctx, a, B, N, (hipStream_t)stream);
  }
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
static int kd_ensure_pairs(landing_ctx* ctx, const landing::KdNlpParams& P) {
  if (ctx->d_kd_pairs) return 0;
  const int NP = landing::KD_NPAIR;
  unsigned char host[2 * landing::KD_NPAIR];
  if (landing::kd_pair_list(host, host + NP) != NP) return fail(LANDING_E_ARG, "kinodynamic NLP: internal pair table");
  const int B = 6, N = 3, NW = landing::KD_NW;
  const size_t nx = (size_t)landing::kd_nx(N), ng = (size_t)landing::kd_ng(N), nh = (size_t)B * N * NW * NW;
  std::vector<double> hx(B * nx), hl(B * ng), hh(nh);
  unsigned long long sdd = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { sdd = sdd * 6364136223846793005ull + 1442695040888963407ull; return (double)((sdd >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0; };      // [0, 1)
  for (auto& v : hx) v = rnd() - 0.5;
  for (auto& v : hl) v = (0.5 + rnd()) * (rnd() < 0.5 ? -1.0 : 1.0);
  DevBuf<unsigned char> d_full; DevBuf<double> d_x, d_l, d_h;
  HIP_TRY(d_full.alloc(sizeof(host))); HIP_TRY(hipMemcpy(d_full.get(), host, sizeof(host), hipMemcpyHostToDevice));
  HIP_TRY(d_x.alloc(hx.size())); HIP_TRY(hipMemcpy(d_x.get(), hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(d_l.alloc(hl.size())); HIP_TRY(hipMemcpy(d_l.get(), hl.data(), hl.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(d_h.alloc(nh)); HIP_TRY(hipMemset(d_h.get(), 0, nh * sizeof(double)));
  landing::KdNlpArgs a;
  a.sx = a.sg = a.sj = a.sh = 0; a.skip = nullptr;
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N; a.x = d_x.get(); a.g = nullptr; a.jac = nullptr; a.lam = d_l.get(); a.hess = d_h.get(); a.P = P;
  // The structure must not depend on the caller's parameter VALUES (ADVICE r5: with Ib = (0.03, 0.03, 0.03) the omega-omega entries of omega x I omega vanish and a later
  // call with the real inertia got 36 wrong zeros): the probe runs with fixed generic constants -- distinct inertias, mu > 0, unit mass, a uniform grid -- so that only the model
  // (landing_rbd_set_model invalidates the table) and the formulation decide which pairs are kept.
  for (int k = 0; k < 64; ++k) a.P.dt[k] = k < N ? 0.03 : 0.0;
  a.P.mass = 1.0; a.P.mu = 0.7; a.P.Ib[0] = 0.05; a.P.Ib[1] = 0.2; a.P.Ib[2] = 0.3; a.P.Ibi[0] = 17.0; a.P.Ibi[1] = 4.3; a.P.Ibi[2] = 3.6;
  const long long n = (long long)B * N * NP;
  kd_launch_hess(ctx, a, B, N, d_full.get(), d_full.get() + NP, NP, (hipStream_t)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(hh.data(), d_h.get(), nh * sizeof(double), hipMemcpyDeviceToHost));
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
  unsigned long long sdd = 0x2545F4914F6CDD1Dull;
  auto rnd = [&]() { sdd = sdd * 6364136223846793005ull + 1442695040888963407ull; return (double)((sdd >> 11) & 0xFFFFFFFFFFFFFull) / 4503599627370496.0; };      // [0, 1)
  for (auto& v : hx) v = rnd() - 0.4;
  DevBuf<double> d_x, d_j;
  HIP_TRY(d_x.alloc(hx.size())); HIP_TRY(hipMemcpy(d_x.get(), hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(d_j.alloc(nj)); HIP_TRY(hipMemset(d_j.get(), 0, nj * sizeof(double)));
  landing::KdNlpArgs a;
  a.sx = a.sg = a.sj = a.sh = 0; a.skip = nullptr;
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N; a.x = d_x.get(); a.g = nullptr; a.jac = d_j.get(); a.lam = nullptr; a.hess = nullptr;
  for (int k = 0; k < 64; ++k) a.P.dt[k] = k < N ? 0.03 : 0.0;
  a.P.mass = 1.0; a.P.mu = 0.7; a.P.Ib[0] = 0.05; a.P.Ib[1] = 0.2; a.P.Ib[2] = 0.3; a.P.Ibi[0] = 17.0; a.P.Ibi[1] = 4.3; a.P.Ibi[2] = 3.6; a.P.std_base = ctx->rbd_std_base;
  kd_launch_jac(ctx, a, B, N, (hipStream_t)nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(hj.data(), d_j.get(), nj * sizeof(double), hipMemcpyDeviceToHost));
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
  HIP_TRY(hipSetDevice(ctx->device));
  landing::KdNlpArgs a;
  a.sx = a.sg = a.sj = a.sh = 0; a.skip = nullptr;
  a.model = ctx->d_rbd.get(); a.B = B; a.N = N; a.x = d_x; a.g = nullptr; a.jac = nullptr; a.lam = d_lam_g; a.hess = d_hess;
  for (int k = 0; k < 64; ++k) a.P.dt[k] = k < N ? prm->dt[k] : 0.0;
  a.P.mass = prm->mass; a.P.mu = prm->mu; a.P.std_base = ctx->rbd_std_base;
  for (int i = 0; i < 3; ++i) { a.P.Ib[i] = prm->Ib[i]; a.P.Ibi[i] = prm->Ib_inv[i]; }
  std::lock_guard<std::mutex> lock(ctx->mu);      // (the lazily built table below, like every other lazily created resource of the context)
  { const int rc = kd_ensure_pairs(ctx, a.P); if (rc) return rc; }      // the list of structurally non-zero pairs of a block, built once per context
  const long long n = (long long)B * N * ctx->kd_npair;
  if (n > 0x7fffffffLL * 64) return fail(LANDING_E_ARG, "landing_kinodyn_nlp_hess: batch too large for one launch");
  HIP_TRY(hipMemsetAsync(d_hess, 0, (size_t)B * N * landing::KD_NW * landing::KD_NW * sizeof(double), (hipStream_t)stream));
  kd_launch_hess(ctx, a, B, N, ctx->d_kd_pairs.get(), ctx->d_kd_pairs.get() + ctx->kd_npair, ctx->kd_npair, (hipStream_t)stream);
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

}  // extern "C"
