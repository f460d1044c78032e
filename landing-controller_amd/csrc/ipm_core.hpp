// ipm_core.hpp -- what the two batched interior-point solvers share: landing_ipm_kernel (solver_kernels.hip, SRBM NLP) and
// landing_kd_head_kernel / landing_kd_iter_kernel (kd_solver_kernels.hip, kinodynamic refinement NLP).
//
// Both run the same primal-dual iteration (slacks with bound multipliers on every inequality row, monotone barrier update, inertia
// correction by delta_w, filter line search with second-order slack correction and watchdog, restarts, feasibility phase on the elastic
// problem: landing_nlp.h).  Their stage linear algebra differs; the scalar control logic and the per-row barrier / elastic arithmetic
// live here, once.  The scalar rules run on ONE lane, inside the solvers' KS_BEGIN / KD_BEGIN blocks, on the control state IpmCtl; the
// per-row functions are called by every lane from the solvers' own row loops, which keep the bound storage and the reductions.
// Nothing here branches on which solver calls it: what differs is passed in (number of fixed rows, proximal floor, ...).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/landing_nlp.h"

namespace landing {

// ---- block-wide reductions through LDS (deterministic order), K values at once ----------------------
enum { RSUM = 0, RMAX = 1, RMIN = 2 };
__device__ __forceinline__ double red_op(double a, double b, int op) { return op == RSUM ? a + b : (op == RMAX ? fmax(a, b) : fmin(a, b)); }
template <int K>
__device__ __forceinline__ void block_reduce(double (&v)[K], const int (&op)[K], double* red) {
  const int tid = threadIdx.x, nwave = (blockDim.x + 63) >> 6;
  for (int i = 0; i < K; ++i) {
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) v[i] = red_op(v[i], __shfl_xor(v[i], mask), op[i]);   // butterfly: every lane gets the wave result
  }
  if ((tid & 63) == 0) for (int i = 0; i < K; ++i) red[(tid >> 6) * K + i] = v[i];
  __syncthreads();
  for (int i = 0; i < K; ++i) {
    double r = red[i];
    for (int w = 1; w < nwave; ++w) r = red_op(r, red[w * K + i], op[i]);
    v[i] = r;
  }
  __syncthreads();
}
__device__ __forceinline__ double block_reduce1(double v, int op, double* red) {
  double a[1] = {v}; const int o[1] = {op};
  block_reduce<1>(a, o, red);
  return a[0];
}

// The four largest of a set of values spread over the block (clip_k rule of the primal step length): every thread keeps
// a sorted quadruple t[0] >= .. >= t[3]; the merge is a max-type operation, hence independent of the order.
__device__ __forceinline__ void top4_push(double (&t)[4], double v) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { const double hi = fmax(t[i], v); v = fmin(t[i], v); t[i] = hi; }
}
__device__ __forceinline__ void block_top4(double (&t)[4], double* red) {
  const int tid = threadIdx.x, nwave = (blockDim.x + 63) >> 6;
#pragma unroll
  for (int mask = 32; mask >= 1; mask >>= 1) {
    double o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = __shfl_xor(t[i], mask);
#pragma unroll
    for (int i = 0; i < 4; ++i) top4_push(t, o[i]);
  }
  if ((tid & 63) == 0) for (int i = 0; i < 4; ++i) red[(tid >> 6) * 4 + i] = t[i];
  __syncthreads();
  for (int i = 0; i < 4; ++i) t[i] = red[i];
  for (int w = 1; w < nwave; ++w) for (int i = 0; i < 4; ++i) top4_push(t, red[w * 4 + i]);
  __syncthreads();
}

// ---- sum over an aligned group of 8 lanes, valid in the group's FIRST lane only (the other lanes end with partial sums) ------------------
// The first lane adds what the butterfly v += xor 1, v += xor 2, v += xor 4 adds there, in the same order.  On the device the partners share
// a 16-lane row, so the values travel by DPP inside the vector ALU (two 32-bit moves per double): quad_perm for distance 1 and 2, a row shift
// by 4 for the last level, which only the first lane needs.  __shfl_xor is ds_bpermute: address, issue and a wait on the LDS counter per
// level.  The host emulation keeps __shfl_xor.  (The butterflies of block_reduce / block_top4 above were moved to DPP the same way and
// measured 0.5 % SLOWER on the headline, dual and line-search phases up by 0.001 ms each: they stay as they are)
#if defined(__HIP_DEVICE_COMPILE__)
template <int CTRL>
__device__ __forceinline__ double dpp_move(double v) {      // (lanes whose source lies outside the row keep their own value)
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(v), __double2loint(v), CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(v), __double2hiint(v), CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
enum { DPP_QUAD_XOR1 = 0xb1, DPP_QUAD_XOR2 = 0x4e, DPP_ROW_SHL4 = 0x104 };      // quad_perm:[1,0,3,2], quad_perm:[2,3,0,1], row_shl:4 (lane i reads lane i + 4)
#endif
__device__ __forceinline__ double lane_sum8_head(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  v += dpp_move<DPP_QUAD_XOR1>(v); v += dpp_move<DPP_QUAD_XOR2>(v);
  return v + dpp_move<DPP_ROW_SHL4>(v);
#else
  v += __shfl_xor(v, 1); v += __shfl_xor(v, 2);
  return v + __shfl_xor(v, 4);
#endif
}

// fp64 matrix-core accumulator tile (v_mfma_f64_16x16x4: 4 doubles per lane)
typedef double f64x4 __attribute__((vector_size(32)));

#if defined(__HIP_DEVICE_COMPILE__)
typedef const double __attribute__((address_space(1)))* landing_gptr;    // global address space: global_load, not flat_load
#else                                                                     // (a flat load also ties up the LDS counter)
typedef const double* landing_gptr;
#endif

// ---- feasibility (restoration) phase: one side of an elastic inequality row ------------------------------------------------------
// The row  lb <= s  becomes  a = s - lb + n >= 0,  n >= 0  with the price rho_pen * n  (upper side: b = ub + q - s, q >= 0); multipliers
// z (of a >= 0) and w (of n >= 0), stationarity  rho_pen - z - w = 0.  Eliminating (dn, dw) from the primal-dual Newton system leaves
//   dz = c - sd * (z / D) ds,   D = a + z n / w,   c = (mu - a z - z (mu - n w + n (z + w - rho_pen)) / w) / D
// (sd = +1 lower side, -1 upper side: d(dist) = sd ds + dn), i.e. the row enters the condensed system with sigma = z / D exactly like
// a plain slack row with sigma = z / d -- condensation, Riccati sweep and forward sweep are those of the normal iteration.
struct ElStep { double dz, dw, dn, da; };
__device__ __forceinline__ ElStep el_step(double sd, double a, double n, double z, double w, double mu, double rho_pen, double ds) {
  ElStep e;
  const double D = a + z * n / w, rn = z + w - rho_pen;
  e.dz = (mu - a * z - z * (mu - n * w + n * rn) / w - sd * z * ds) / D;
  e.dw = -e.dz - rn;
  e.dn = (mu - n * w - n * e.dw) / w;
  e.da = sd * ds + e.dn;
  return e;
}

// ---- scalar state of the iteration ---------------------------------------------------------------------------------------------
// The fields both solvers keep.  Written by one lane only, between barriers (KS_BEGIN / KD_BEGIN); every lane reads it in place.
struct IpmCtl {
  double mu, delta_last, th_max, c_pr, c_co, c_cm, c_ys, c_zs, c_nz, e_pr, e_du, e_co;
  double tau, omt, a_pr, a_du, th0, ph0, dphi, alpha, s_corr, delta, ft;      // omt > 0: clip_k rule in force (slacks stop at omt of their distance)
  long long tp;      // development aid: wall_clock64 tick of the last phase mark
  int nfilt, it, status, need_reg_streak, nreset, last_reset_it, ncrawl, clip_k_cur, last_mu_it, cutstreak, wd_count, first_failed, force_step;
  int accepted, armijo_step, fact_ok, skipped_zero, attempt;
  int stag, full_prev;      // stag_relief (landing_nlp.h): full steps of the last barrier problem that did not halve the error
  double e_prev;
  int flag, fresh, ls_done, need_corr, fallback;
  // feasibility (restoration) phase, landing_nlp.h: 1 while the elastic problem is being solved; lim = iteration limit in force
  int feas, feas_used, lim;
  int fjam, fstat; double v1_ref;      // feas_jam / feas_stat (landing_nlp.h): leaky count of iterations with a tiny accepted step; iterations with a stationary violation, its reference value
  double c_rn, f_vmax, f_v1;      // |z + w - rho|_inf of the elastic rows; max-norm and 1-norm violation of the inequality rows at x
  // landing_nlp.h feas_max, feas_back, feas_resume, feas_polish: entries into the phase so far; 1 once a stalled phase has handed its point back (or the
  // line search jammed with no entry left); 1 once the regularisation was dropped at a stationary violation; violation at the entry point (1-norm, equality rows
  // included) and 1-norm residual of the equality rows at x; iteration count nothing runs beyond; 1: the entry pass of the phase has to record th_entry
  int n_feas, stalled, polished, hard_lim, want_entry; double th_entry, f_theq;
  double fdc;      // factor between the regularisation of the last iteration and the first one tried in this one inside the phase (feas_delta_dec, adapted: squared after an
                   // iteration whose first factorisation succeeded, square root (<= 0.7) after one that needed more)
};
// what the stop test decides (ipm_decide)
enum { ACT_GO = 0, ACT_STOP = 1, ACT_RESET = 2, ACT_FEAS = 3, ACT_BACK = 4 };

__host__ __device__ __forceinline__ void ipm_init(IpmCtl& K, const landing_solver_opts& o) {
  K = IpmCtl{};
  K.mu = o.mu_init; K.c_nz = 1.0; K.omt = -1.0; K.e_prev = 1e300;
  K.status = LANDING_MAX_ITER; K.clip_k_cur = o.clip_k; K.lim = o.max_iter; K.hard_lim = o.max_iter > 0 ? 3 * o.max_iter : 0;
  K.fdc = o.feas_delta_dec > 0.0 ? o.feas_delta_dec : o.delta_dec;
}

// errors of the current iterate (du = |grad L|_inf over the free variables) and the stag_relief count
__host__ __device__ __forceinline__ void ipm_errors(IpmCtl& K, const landing_solver_opts& o, double du) {
  const double pr = K.c_pr, co = K.c_co;
  if (K.feas) du = fmax(du, K.c_rn);      // the elastic problem has the extra stationarity rows rho_pen - z - w = 0
  K.e_pr = pr; K.e_du = du; K.e_co = co;
  if (o.stag_relief > 0) {      // full Newton steps in the last barrier problem that do not halve the error: the proximal term is what holds them back
    const double E = fmax(pr, du);
    K.stag = (!K.feas && K.mu <= o.tol / 10.0 * 1.0000001 && K.full_prev && E > 0.5 * K.e_prev) ? K.stag + 1 : 0;
    K.e_prev = E;
  }
}

// into the feasibility phase (the row data are the solver's: el_init_row)
__host__ __device__ __forceinline__ void ipm_enter_phase(IpmCtl& K, const landing_solver_opts& o) {
  const int it = K.it;
  K.feas = 1; K.n_feas++; K.feas_used = K.n_feas >= o.feas_max ? 1 : 0; K.status = LANDING_MAX_ITER; K.lim = it + o.max_iter; if (K.lim > K.hard_lim) K.lim = K.hard_lim; K.fstat = -1; K.fjam = 0; K.want_entry = 1; K.fdc = o.feas_delta_dec > 0.0 ? o.feas_delta_dec : o.delta_dec;
  K.mu = o.mu_init; K.nfilt = 0; K.th_max = 0.0; K.delta_last = 0.0; K.need_reg_streak = 0; K.cutstreak = 0; K.force_step = 0; K.wd_count = 0;
  K.it = it + 1;
}

// back from the feasibility phase: the interior-point solve restarts from its point (slacks: ipm_init_row with back = true when feas_ret_push > 0)
__host__ __device__ __forceinline__ void ipm_leave_phase(IpmCtl& K, const landing_solver_opts& o) {
  const int it = K.it;
  K.feas = 0; K.lim = it + (o.max_iter > 1 ? o.max_iter : 1); if (K.lim > K.hard_lim) K.lim = K.hard_lim; K.status = LANDING_MAX_ITER;
  K.mu = (o.feas_ret_push > 0.0 && o.feas_ret_mu > 0.0) ? o.feas_ret_mu : o.mu_init; K.fjam = 0; K.nfilt = 0; K.delta_last = 0.0; K.need_reg_streak = 0; K.wd_count = 0; K.th_max = 0.0; K.nreset = 0; K.last_reset_it = it; K.ncrawl = 0;
  K.cutstreak = 0; K.force_step = 0;
  K.it = it + 1;
}

// restart: slacks, multipliers, barrier parameter and filter are re-initialised at the current x or (K.fresh) at the caller's initial guess
// with the step rule clip_k = 2 (landing_nlp.h fresh_restart)
__host__ __device__ __forceinline__ void ipm_restart(IpmCtl& K, const landing_solver_opts& o, bool stalled, bool lost) {
  const int it = K.it, nreset = K.nreset;
  K.last_reset_it = it;
  if (stalled) K.ncrawl++;
  K.nreset = nreset + 1;
  // the restart in place did not help (second restart) or the iterate is jammed: back to the caller's initial guess with
  // another step rule (landing_nlp.h: the members that fail from it with clip_k = 4 solve with clip_k = 2)
  K.fresh = (((o.fresh_restart & 2) && nreset + 1 == 2) || ((o.fresh_restart & 1) && nreset + 1 == 1 && !stalled && !lost)) ? 1 : 0;
  if (K.fresh) { if (K.clip_k_cur > 1) K.clip_k_cur = 2; K.th_max = 0.0; }
  K.mu = o.mu_init; K.nfilt = 0; K.delta_last = 0.0; K.need_reg_streak = 0; K.wd_count = 0;
  K.it = it + 1;
}

// What happens with this iterate (errors from ipm_errors): stop, restart, into or out of the feasibility phase, or another iteration.
// failed: no regularisation made the last step computable (the solve ends NUMERICAL, or enters the phase).
__host__ __device__ __forceinline__ int ipm_decide(IpmCtl& K, const landing_solver_opts& o, bool failed) {
  const double pr = K.e_pr, du = K.e_du, co = K.e_co, mu = K.mu;
  const int it = K.it, nreset = K.nreset;
  int act = ACT_GO;
  bool give_up = false;
  if (K.feas) {
    // feasibility phase: a feasible point (or an elastic KKT point with negligible violation) restarts the solve from here, an elastic
    // KKT point with positive violation is the certificate of local infeasibility
    const bool conv = fmax(du, fmax(pr, co)) <= o.tol;
    if (!(du < 1e300) || !(pr < 1e300) || !(co < 1e300)) { K.status = LANDING_NUMERICAL; act = ACT_STOP; }
    else if (K.f_vmax <= 1e-9 && pr <= o.tol) act = ACT_BACK;
    else if (conv && K.f_v1 > o.feas_cert) { K.status = LANDING_INFEASIBLE; act = ACT_STOP; }      // KKT point of the elastic problem with positive violation: the certificate
    else if (conv) act = ACT_BACK;
    else if (o.feas_back > 0.0 && !K.feas_used && K.f_v1 + K.f_theq <= o.feas_back * K.th_entry) act = ACT_BACK;      // the violation has come down: IPOPT leaves its restoration phase here
    else if (o.feas_stat > 0) {      // stationary violation (landing_nlp.h): NOT a certificate
      const double v1 = K.f_v1;
      if (K.fstat < 0 || !(fabs(v1 - K.v1_ref) <= 0.05 * K.v1_ref)) { K.v1_ref = v1; K.fstat = 0; } else K.fstat++;
      if (K.fstat >= o.feas_stat && mu <= 1e-4 && pr <= 1e-3) {
        if (v1 <= o.feas_cert) act = ACT_BACK;
        else if (o.feas_polish > 0.0 && !K.polished) {      // once: the regularisation drops -- a stationary point is then a few Newton steps from the elastic KKT point
          K.polished = 1; K.fstat = -1; K.delta_last = o.feas_polish / (o.feas_delta_dec > 0.0 ? o.feas_delta_dec : o.delta_dec); K.need_reg_streak = 2;
        }
        else if (o.feas_resume && !K.stalled) { K.stalled = 1; K.feas_used = 1; act = ACT_BACK; }      // the interior-point iteration resumes from this point, once
        else { K.status = LANDING_STALLED; act = ACT_STOP; }
      }
    }
    if (act == ACT_GO && it >= K.lim) act = ACT_STOP;      // (status MAX_ITER, set at the entry)
    if (act == ACT_BACK) ipm_leave_phase(K, o);
  }
  else if (failed) { K.status = LANDING_NUMERICAL; give_up = true; }
  else if (!(du < 1e300) || !(pr < 1e300) || !(co < 1e300)) { K.status = LANDING_NUMERICAL; give_up = true; }
  else if (fmax(du, fmax(pr, co)) <= o.tol) { K.status = LANDING_CONVERGED; act = ACT_STOP; }
  else if (it >= K.lim) give_up = true;      // (>=: K.it runs ahead of a limit set from a max_iter < 1; status MAX_ITER)
  else if (du > o.reset_du && nreset >= o.max_resets && o.max_resets > 0) { K.status = LANDING_NUMERICAL; give_up = true; }   // jammed again: give up
  else if (o.feas_jam > 0 && K.fjam >= o.feas_jam && pr > 1e-3 && o.feas_phase) { give_up = true; if (K.feas_used) K.stalled = 1; }      // jammed line search: the feasibility phase starts now (landing_nlp.h); no entry left: the solve ends here, status 4
  else {
    // jammed iterate (multipliers blown up) -- the role IPOPT's restoration phase plays on this problem class;
    // crawling: still in the first barrier problem (mu never decreased) restart_period iterations after the last (re)start
    const bool jam = du > o.reset_du && nreset < o.max_resets;
    const bool stalled = o.restart_period > 0 && it - K.last_reset_it >= o.restart_period && mu >= o.mu_init && nreset < o.max_resets && K.ncrawl < ((o.fresh_restart & 4) ? 2 : 1);
    const bool overreg = o.reset_delta > 0.0 && K.delta_last > o.reset_delta && nreset < o.max_resets;
    // a LATER barrier problem not solved 2 restart_period iterations after it began has wandered off (the dual infeasibility stays
    // far below reset_du, nothing else catches it): restarted in place like a crawling iterate
    const bool lost = (o.fresh_restart & 8) && o.restart_period > 0 && mu < o.mu_init && pr > 1e-3 && nreset < o.max_resets &&
                      ((it - K.last_mu_it >= 2 * o.restart_period && it - K.last_reset_it >= o.restart_period) || K.wd_count >= 3);     // ... or crawls on although the watchdog has fired three times
    if (jam || stalled || overreg || lost) { act = ACT_RESET; ipm_restart(K, o, stalled, lost); }
  }
  if (give_up) {
    // the solve would end here as NUMERICAL / MAX_ITER: enter the feasibility phase once (landing_solver_opts::feas_phase)
    if (K.stalled) K.status = LANDING_STALLED;      // the point a stalled phase handed back did not lead anywhere either
    if (o.feas_phase && !K.feas_used && o.max_iter > 0 && it < K.hard_lim) {      // (max_iter < 1: the caller asked for no iteration at all, the phase would get none either)
      act = ACT_FEAS;
      ipm_enter_phase(K, o);
    } else act = ACT_STOP;
  }
  return act;
}

// Monotone barrier update (IPOPT's scaling of the optimality error in the barrier-subproblem test when barrier_smax > 0; nfree = rows
// that are not fixed by the initial conditions): true when mu was decreased -- the caller then recomputes the row quantities and asks again.
__host__ __device__ __forceinline__ bool ipm_barrier_update(IpmCtl& K, const landing_solver_opts& o, int nfree) {
  double sd = 1.0, sc = 1.0;
  if (o.barrier_smax > 0.0) {
    sd = fmax(o.barrier_smax, (K.c_ys + K.c_zs) / ((double)nfree + K.c_nz)) / o.barrier_smax;
    sc = fmax(o.barrier_smax, K.c_zs / K.c_nz) / o.barrier_smax;
  }
  const double mu = K.mu;
  if (fmax(K.e_du / sd, fmax(K.c_pr, K.c_cm / sc)) <= o.kappa_eps * mu && mu > o.tol / 10.0) {
    K.mu = fmax(o.tol / 10.0, fmin(o.kappa_mu * mu, pow(mu, o.theta_mu)));
    K.nfilt = 0; K.last_mu_it = K.it; K.wd_count = 0;
    return true;
  }
  K.tau = fmax(o.tau_min, 1.0 - mu);
  return false;
}

// ---- inertia correction: IPOPT's schedule (delta_w = 0 first, then max(1e-20, delta_last * delta_dec), then x delta_inc_first / x delta_inc),
// except that an iteration following a regularised one starts from delta_last * delta_dec directly when the unregularised attempt failed twice
// in a row (saves one full factorisation in nonconvex phases).  Inside the phase the decrease factor is the adapted K.fdc (landing_nlp.h feas_delta_dec).
__host__ __device__ __forceinline__ double ipm_delta_dec(const IpmCtl& K, const landing_solver_opts& o) { return (K.feas && o.feas_delta_dec > 0.0) ? K.fdc : o.delta_dec; }

// delta_w of the first attempt: dec = factor on delta_last (ipm_delta_dec), floor = proximal term (landing_nlp.h delta_floor: 0 where the
// form has none or inside the phase), a tenth of it per stagnating iteration (stag_relief)
__host__ __device__ __forceinline__ void ipm_first_delta(IpmCtl& K, const landing_solver_opts& o, double dec, double floor) {
  const double dl = K.delta_last;
  K.delta = (K.need_reg_streak >= 2 && dl > 0.0) ? fmax(1e-20, dl * dec) : 0.0;
  if (o.stag_relief > 0 && K.stag >= o.stag_relief) {
    for (int e = K.stag - o.stag_relief; e >= 0 && floor >= 1e-12; --e) floor *= 0.1;
    if (floor < 1e-12) floor = 0.0;
  }
  K.delta = fmax(K.delta, floor);
  K.skipped_zero = K.delta > 0.0;
  K.fact_ok = 0; K.attempt = 0; K.flag = 1;
}

// The factorisation with K.delta has been tried (ok = right inertia).  True: try again with the next regularisation, left in K.delta.
// cont > 0: a regularisation to continue from at the first failure when it is above the next step of the schedule (0: none).
__host__ __device__ __forceinline__ bool ipm_next_delta(IpmCtl& K, const landing_solver_opts& o, bool ok, double cont) {
  K.fact_ok = ok ? 1 : 0;
  if (K.attempt == 0) K.first_failed = (K.skipped_zero && !ok) ? 1 : 0;
  K.attempt++;
  if (ok || K.attempt >= 60) return false;
  double d = K.delta; const double dl = K.delta_last;
  if (d == 0.0) d = (dl == 0.0) ? o.delta_init : fmax(1e-20, dl * ipm_delta_dec(K, o));
  else if (K.feas && o.feas_delta_dec > 0.0 && K.attempt == 1 && d < dl) d = dl;      // inside the phase: the regularisation of the last iteration is the best guess of what this one needs
  else if (K.attempt == 1 && cont > d * o.delta_inc) d = cont;
  else d *= (dl == 0.0 ? o.delta_inc_first : o.delta_inc);
  if (d > 1e40) return false;
  K.delta = d;
  return true;
}

// After the successful factorisation: adapt K.fdc inside the phase, remember a regularisation above `floor`.  True when K.delta counts as one.
__host__ __device__ __forceinline__ bool ipm_commit_delta(IpmCtl& K, const landing_solver_opts& o, double floor) {
  const bool adapt = K.feas && o.feas_delta_dec > 0.0;
  if (adapt) K.fdc = K.attempt <= 1 ? fmax(o.feas_delta_dec, K.fdc * K.fdc) : fmin(0.7, sqrt(K.fdc));      // (attempt counts the factorisations of this iteration)
  const bool reg = K.delta > floor;
  if (reg) { K.delta_last = K.delta; K.need_reg_streak++; } else K.need_reg_streak = 0;
  if (K.need_reg_streak > 8) K.need_reg_streak = adapt ? 2 : 0;      // probe delta = 0 again from time to time (not inside the phase: the elastic problem has no objective)
  return reg;
}

// ---- filter line search (Waechter & Biegler); the filter entries (theta, phi) live with the solver: fth / fph, K.nfilt of them
__host__ __device__ __forceinline__ bool ipm_filter_ok(const IpmCtl& K, const landing_solver_opts& o, double th, double ph, const double* fth, const double* fph) {
  const double th_floor = o.theta_floor * o.tol;      // violations below the tolerance count as equal (landing_nlp.h)
  bool ok = (th <= K.th_max) && (ph < 1e300) && (ph > -1e300);
  for (int e = 0; e < K.nfilt && ok; ++e) if (th >= fmax(fth[e], th_floor) && ph >= fph[e]) ok = false;
  return ok;
}

// trial point at step length K.alpha: violation tht, merit ft + mu bt.  Leaves accepted / ls_done / need_corr, or halves K.alpha
__host__ __device__ __forceinline__ void ipm_ls_test(IpmCtl& K, const landing_solver_opts& o, double tht, double ft, double bt, const double* fth, const double* fph) {
  const double alpha = K.alpha, th_min = 1e-4, th_floor = o.theta_floor * o.tol;
  const double th0 = K.th0, ph0 = K.ph0, dphi = K.dphi;
  const double pht = ft + K.mu * bt;
  const bool ok_f = ipm_filter_ok(K, o, tht, pht, fth, fph) && (tht < 1e300);
  const bool switching = (dphi < 0.0) && (th0 <= th_min) && (alpha * pow(-dphi, 2.3) > 1.0 * pow(th0, 1.1));
  bool accepted = false, done = false;
  if (ok_f) {
    if (switching) {
      if (pht <= ph0 + 1e-8 * alpha * dphi) { accepted = true; K.armijo_step = 1; }
    } else if (tht <= fmax((1.0 - 1e-5) * th0, th_floor) || pht <= ph0 - 1e-8 * th0) {
      accepted = true;
    }
  }
  if (K.force_step && ok_f) { accepted = true; K.nfilt = 0; done = true; }      // watchdog (landing_nlp.h): the step to the boundary is taken without the sufficient-decrease / switching tests;
                                                                                // it must still pass theta <= theta_max and must not be dominated by a filter entry (ok_f), then the filter restarts
  if (accepted) done = true;
  K.need_corr = 0;
  if (!done) {
    if (o.slack_corr > 0.0 && !K.feas && alpha == K.a_pr && tht >= th0) { K.need_corr = 1; K.ft = ft; }
    else { K.alpha = alpha * 0.5; if (!(K.alpha > 1e-10)) done = true; }
  }
  K.accepted = accepted ? 1 : 0;
  K.ls_done = done ? 1 : 0;
}

// the same trial point with the inequality slacks moved to g(x_trial) (landing_nlp.h slack_corr): violation tht2, merit K.ft + mu bt2
__host__ __device__ __forceinline__ void ipm_ls_corr_test(IpmCtl& K, const landing_solver_opts& o, double tht2, double bt2, const double* fth, const double* fph) {
  const double alpha = K.alpha, th_floor = o.theta_floor * o.tol, th0 = K.th0, ph0 = K.ph0;
  const double pht2 = K.ft + K.mu * bt2;
  if (ipm_filter_ok(K, o, tht2, pht2, fth, fph) && (tht2 <= fmax((1.0 - 1e-5) * th0, th_floor) || pht2 <= ph0 - 1e-8 * th0)) { K.accepted = 1; K.s_corr = o.slack_corr; K.ls_done = 1; }
  else { K.alpha = alpha * 0.5; if (!(K.alpha > 1e-10)) K.ls_done = 1; }
}

// End of the line search: watchdog, fallback step (K.fallback: x + alpha dx has to be evaluated), filter update (cap entries at most),
// dual step cap, feas_jam count, full-step flag of stag_relief
__host__ __device__ __forceinline__ void ipm_ls_end(IpmCtl& K, const landing_solver_opts& o, double* fth, double* fph, int cap) {
  const double a_pr = K.a_pr;
  K.force_step = 0;
  if (o.watchdog > 0 && !K.feas) {      // successive iterations with step lengths <= 1/16 of the step to the boundary arm the watchdog
    if (K.accepted && K.alpha <= 0.0625 * a_pr) { if (++K.cutstreak >= o.watchdog) { K.force_step = 1; K.cutstreak = 0; K.wd_count++; } }
    else K.cutstreak = 0;
  }
  K.fallback = 0;
  if (!K.accepted) {
    // no acceptable step: take a short step along the Newton direction and restart the filter
    K.nfilt = 0;
    K.alpha = fmin(a_pr, o.alpha_fallback);
    K.fallback = 1;
  } else if (!K.armijo_step) {
    int nfilt = K.nfilt;
    if (nfilt == cap) {     // drop the oldest entry (serial, rare)
      for (int e = 0; e + 1 < cap; ++e) { fth[e] = fth[e + 1]; fph[e] = fph[e + 1]; }
      nfilt = cap - 1;
    }
    fth[nfilt] = (1.0 - 1e-5) * K.th0; fph[nfilt] = K.ph0 - 1e-8 * K.th0;
    K.nfilt = nfilt + 1;
  }
  if (o.dual_step_cap > 0.0) K.a_du = fmin(K.a_du, o.dual_step_cap * K.alpha);      // the multipliers do not run ahead of a blocked primal step (landing_nlp.h)
  if (o.feas_jam > 0) K.fjam = (!K.feas && K.alpha < 1e-2) ? K.fjam + 1 : (K.fjam > 2 ? K.fjam - 2 : 0);
  K.full_prev = (K.accepted && K.alpha == 1.0 && K.a_du == 1.0 && K.attempt <= 1) ? 1 : 0;
}

// ---- per-row functions.  Mem = the solver's view of a member's workspace (MemberMem / KdMem: arrays g, y, s, zL, zU, en, ep, wn, wp of ng rows);
// lb, ub = the row's bounds.  The callers run them over their non-fixed rows.

// Slack of an inequality row pushed into the interior (IPOPT's bound_push / bound_frac), multipliers of its finite bounds 1, y = zU - zL.
// back (return from the feasibility phase, landing_nlp.h feas_ret_push): pushed only feas_ret_push off the bounds, multipliers mu / distance --
// what the phase gained in feasibility is kept.  Not an inequality row (slack = false): all zero.
template <class Mem>
__host__ __device__ __forceinline__ void ipm_init_row(const Mem& M, int r, bool slack, double lb, double ub, const landing_solver_opts& o, bool back, double mu) {
  const double push = back ? o.feas_ret_push : o.bound_push, frac = back ? o.feas_ret_push : o.bound_frac;
  double sv = 0.0, zl = 0.0, zu = 0.0;
  if (slack) {
    const bool hL = lb > -INFINITY, hU = ub < INFINITY;
    sv = M.g[r];
    double pl, pu;
    if (hL && hU) { pl = fmin(push * fmax(1.0, fabs(lb)), frac * (ub - lb)); pu = fmin(push * fmax(1.0, fabs(ub)), frac * (ub - lb)); }
    else { pl = push * fmax(1.0, hL ? fabs(lb) : 0.0); pu = push * fmax(1.0, hU ? fabs(ub) : 0.0); }
    if (hL) sv = fmax(sv, lb + pl);
    if (hU) sv = fmin(sv, ub - pu);
    if (back) { zl = hL ? fmin(fmax(mu / (sv - lb), 1e-8), 1e3) : 0.0; zu = hU ? fmin(fmax(mu / (ub - sv), 1e-8), 1e3) : 0.0; }
    else { zl = hL ? 1.0 : 0.0; zu = hU ? 1.0 : 0.0; }
  }
  M.s[r] = sv; M.zL[r] = zl; M.zU[r] = zu; M.y[r] = zu - zl;
}

// Entry into the feasibility phase: slack on the row value, violation variables sized so that both distances start at a comfortable value
// (mu0 = the phase's first barrier parameter, frho = rho_pen); the multipliers of equality rows start at 0
template <class Mem>
__host__ __device__ __forceinline__ void el_init_row(const Mem& M, int r, double lb, double ub, double mu0, double frho) {
  const double g = M.g[r];
  if (lb == ub) { M.y[r] = 0.0; return; }
  double zl = 0.0, zu = 0.0, n0 = 0.0, q0 = 0.0, wl = 0.0, wu = 0.0;
  if (lb > -INFINITY) { const double v = lb - g; n0 = fmax(v, 0.0) + fmax(1e-2, 0.1 * fabs(v)); zl = fmin(mu0 / (g - lb + n0), 0.5 * frho); wl = frho - zl; }
  if (ub < INFINITY) { const double v = g - ub; q0 = fmax(v, 0.0) + fmax(1e-2, 0.1 * fabs(v)); zu = fmin(mu0 / (ub + q0 - g), 0.5 * frho); wu = frho - zu; }
  M.s[r] = g; M.en[r] = n0; M.ep[r] = q0; M.zL[r] = zl; M.zU[r] = zu; M.wn[r] = wl; M.wp[r] = wu; M.y[r] = zu - zl;
}

// Errors of the elastic problem at the current point (one lane's share; el_point_finish reduces them): primal error, complementarity,
// its deviation from mu, |y|_1, |z|_1, number of bound multipliers, |z + w - rho_pen|_inf, violation of the inequality rows at x
// (max norm, 1-norm), 1-norm residual of the equality rows
struct ElAcc { double pr, co, cm, ys, zs, nz, rn, vmax, v1, teq; };

// one side of an elastic row (sd = +1 lower, -1 upper; a = distance + violation variable n): errors into e, its part of Sigma / rho into sg / rh
__host__ __device__ __forceinline__ void el_point_side(ElAcc& e, double sd, double a, double n, double z, double w, double mu, double frho, double& sg, double& rh) {
  const double D = a + z * n / w;
  const double c = (mu - a * z - z * (mu - n * w + n * (z + w - frho)) / w) / D;
  e.co = fmax(e.co, fmax(a * z, n * w)); e.cm = fmax(e.cm, fmax(fabs(a * z - mu), fabs(n * w - mu))); e.rn = fmax(e.rn, fabs(z + w - frho));
  sg += z / D; rh -= sd * (z + c); e.zs += z; e.nz += 1.0;
}

// one row at barrier parameter mu: errors into e, Sigma and rho of the row returned (the row enters the condensed system like a slack row)
template <class Mem>
__host__ __device__ __forceinline__ void el_point_row(ElAcc& e, const Mem& M, int r, double lb, double ub, double mu, double frho, double& sg, double& rh) {
  const double g = M.g[r];
  e.ys += fabs(M.y[r]);
  if (lb == ub) { e.pr = fmax(e.pr, fabs(g - lb)); e.teq += fabs(g - lb); return; }
  const double s = M.s[r], v = fmax(fmax(lb - g, g - ub), 0.0);
  e.pr = fmax(e.pr, fabs(g - s)); e.vmax = fmax(e.vmax, v); e.v1 += v;
  if (lb > -INFINITY) { const double n = M.en[r]; el_point_side(e, 1.0, s - lb + n, n, M.zL[r], M.wn[r], mu, frho, sg, rh); }
  if (ub < INFINITY) { const double q = M.ep[r]; el_point_side(e, -1.0, ub + q - s, q, M.zU[r], M.wp[r], mu, frho, sg, rh); }
  rh += sg * (g - s);
}

// block reduction of the lanes' ElAcc into K (every thread calls it, in uniform control flow; red = (blockDim / 64) * 6 doubles of LDS)
__device__ __forceinline__ void el_point_finish(IpmCtl& K, const ElAcc& e, double* red) {
  double v[6] = {e.pr, e.co, e.cm, e.ys, e.zs, e.nz}; const int op[6] = {RMAX, RMAX, RMAX, RSUM, RSUM, RSUM};
  block_reduce<6>(v, op, red);
  double u[4] = {e.rn, e.vmax, e.v1, e.teq}; const int op4[4] = {RMAX, RMAX, RSUM, RSUM};
  block_reduce<4>(u, op4, red);
  if (threadIdx.x == 0) {
    K.c_pr = v[0]; K.c_co = v[1]; K.c_cm = v[2]; K.c_ys = v[3]; K.c_zs = v[4]; K.c_nz = fmax(v[5], 1.0); K.c_rn = u[0]; K.f_vmax = u[1]; K.f_v1 = u[2]; K.f_theq = u[3];
    if (K.want_entry) { K.th_entry = u[2] + u[3]; K.want_entry = 0; }      // first pass of a phase: the violation it starts from
  }
  __syncthreads();
}

}  // namespace landing
