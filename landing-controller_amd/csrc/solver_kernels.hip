// solver_kernels.hip -- batched primal-dual interior-point solver for the SRBM landing NLP (gfx950).
//
// ONE WAVEFRONT = ONE NLP, from the initial guess to the KKT point, in a single persistent kernel:
// members never wait for each other (no lock-step batch iterations), the hardware workgroup
// dispatcher is the work queue.  What replaces the reference's CasADi Nlpsol('ipopt') + MA57 path
// (generate_landingCtrller_IPOPT.m:231-264,277,314; casadi/core/nlpsol.cpp:560-640):
//   * the NLP IPOPT sees through the CasADi boundary: every bound lives in g (lbx/ubx = +-inf), so
//     every inequality row gets a slack and a pair of bound multipliers;
//   * monotone barrier update, fraction-to-the-boundary rule, filter line search (Waechter & Biegler);
//   * the KKT system is condensed stage-wise and solved by a Riccati recursion with state
//     (X_k, c_k) and control (f_k, c_{k+1}) -- the no-slip rows couple U_k and U_{k+1}, carrying the
//     feet as state restores the optimal-control sparsity; inertia correction = retry with a larger
//     delta_w when a stage Cholesky meets a non-positive pivot (IPOPT's rule of thumb).
// Function values / derivatives come from the same srbm_stage.hpp code as the function layer, in the
// reference's CCS order; the assembly into stage blocks is table driven (solver_capi.inc).
#include <hip/hip_runtime.h>
#include <math.h>
#include <type_traits>

#include "../../include/landing_nlp.h"
#include "ipm_core.hpp"

// The phase functions of the solver (riccati_backward, forward_pass, row_products, ...) are __noinline__.  Measured round 3, A/B on
// one box: with every phase inlined into landing_ipm_kernel the callee-saved-register traffic disappears (209 -> 192 GB of HBM traffic
// per launch) but the monolithic kernel is allocated and scheduled far worse -- condensation 0.104 -> 0.231 ms, forward sweep
// 0.082 -> 0.146 ms per iteration under load, 96 -> 141 ms per batch.  Out of line it is.

namespace landing {

constexpr int NZ_JX = 0, NZ_JU = 157, NZ_JUN = 385, NZ_HX = 613, NZ_HU = 642, NZ_HUN = 802, NZ_TOT = 962;
constexpr int GS = 49;    // LDS row stride of G (48x48)
constexpr int PS = 25;    // LDS row stride of 24x24 matrices
constexpr int YS = 37;    // LDS row stride of 24x36 / 12x36 matrices
// per-stage Riccati record (doubles): K 24x24 | kappa 24 | A^ 12x36 | b 12 | P_k rows of X (12x24) | p_k X part 12
// stage record: gains K (nu x 24) | kappa (24) | closed-loop state map of the forward sweep X+ = Mt sigma + mv (12 x 24 | 12) |
// state rows of the cost-to-go P (12 x 24) | p (12)
constexpr int RIC_K = 0, RIC_KAP = 576, RIC_MT = 600, RIC_MV = 888, RIC_PX = 900, RIC_PV = 1188, RIC_STRIDE = 1200;
constexpr int RIC_FWD0 = 288, RIC_FWDN = 612;   // forward chain reads rec[288, 900): K rows of c+ | kappa | Mt | mv
constexpr int FILT_CAP = 64;
constexpr int SOLVER_NMAX = 96;   // longest horizon the solver kernel takes: sigma_0..sigma_N of the forward sweep live in the 48 x 49 LDS array, one table row per stage
constexpr int SOLVER_THREADS = 256;
constexpr int RCG = 36;   // per stage in the member's workspace: gradient of the running cost w.r.t. (X_k, c_k, f_k) (forms with a running cost)
// constant Hessian entries of the running cost per stage, stored right behind the Hessian nonzeros so that the
// condensation tables address them like any other entry of [J | H]: X diagonal (12) | (pos_a, c_leg,a) (12) | c diagonal (12) | f diagonal (12)
constexpr int RUNC = 48;

// Assembly of a stage inside the backward sweep (asm_terms): operands of the condensation terms are positions in the LDS array
// cx = [nonzeros of the stage (NZ_TOT + RUNC) | sigma (104) | rho (104) | 1, -1, 0]
constexpr int CX_SR = NZ_TOT + 48, CX_ONE = CX_SR + 208, CX_MONE = CX_ONE + 1, CX_ZERO = CX_ONE + 2, CX_LEN = CX_ONE + 3;
constexpr int ATAB_TB = 6, ATAB_LTMAX = 6;       // terms per batch; longest per-thread list (a multiple of ATAB_TB): the 1 138..1 234 terms of a stage give 5 per thread
constexpr int ASM_NSLOT = 512;                   // partial-sum slots of one stage

// exit record of a member (the last doubles of its block, behind y2; landing_nlp.h landing_debug_workspace): the scalars of the last step that live in
// LDS only -- mu | delta | alpha | a_du | 1 when the second instance of the swapped row arrays is the live one | it | omt | s_corr
constexpr int EXIT_REC = 8;
// doubles of one member's block of the solver workspace (landing::SolverWorkspace, capi.hip)
inline size_t member_stride(const Layout& L) {
  return (size_t)4 * L.nx + (size_t)20 * L.ng + L.nnz_jac + L.nnz_hess + (size_t)L.N * RUNC + (size_t)(L.N + 1) * RIC_STRIDE + (size_t)L.N * RCG + EXIT_REC;
}

// optional per-member phase timers (wall_clock64 ticks, 100 MHz) -- enabled when SolveArgs.prof != nullptr
enum { PH_EVAL = 0, PH_ERR, PH_SIGRHO, PH_BACK, PH_FWD, PH_DUAL, PH_LS, PH_ACCEPT, PH_NFACT, PH_NTRIAL, PH_NITER, PH_NSTAGE_OK, PH_B_ASM, PH_NSTAGE, PH_B_ELIM, PH_B_POST,
       PH_COUNT = 16 };   // 11 / 13: stage eliminations that succeeded / were attempted (stage-0 foot block included)
#define PROF_ADD(slot, tstart) do { if (SH.prof_on) { const long long n_ = (long long)wall_clock64(); if (threadIdx.x == 0) { SH.prof[slot] += (double)(n_ - (tstart)); (tstart) = n_; } } } while (0)

// Host emulation only (the CPU suite's build of this file; the product is compiled by hipcc): how each accepted step of a member came about,
// counted per member of the last launch -- landing_emu_accept_counts().  The tests use it to see that the fused first trial really is the path
// taken by ordinary iterations and is bypassed by the others.
enum { EMU_ACC_FAST = 0, EMU_ACC_FAST_CLIP, EMU_ACC_FIRST_REJECTED, EMU_ACC_BACKTRACK, EMU_ACC_CORR, EMU_ACC_FALLBACK, EMU_ACC_FEAS, EMU_ACC_N };
#ifndef __HIPCC__
constexpr int EMU_ACC_MAXB = 64;
static int emu_acc[EMU_ACC_MAXB][EMU_ACC_N];
#define LANDING_EMU_COUNT(m, what) do { if ((m) < EMU_ACC_MAXB) emu_acc[m][what]++; } while (0)
// 0: the first trial pass is never fused, every step goes through the accept pass over the rows (the path every step took before the fused
// pass existed) -- the tests run members both ways and ask for equal bits
static int emu_fused_on = 1;
#define LANDING_EMU_FUSED_ON (emu_fused_on != 0)
extern "C" void landing_emu_set_fused(int on) { emu_fused_on = on; }
// counts[EMU_ACC_N] of member m: swap accepts (without / with the clip rule in force), first trial points that were not accepted as they stood,
// row-pass accepts behind back-tracking / with the slack correction / of the fallback step, accepts inside the feasibility phase
extern "C" int landing_emu_accept_counts(int m, int* counts) {
  if (m < 0 || m >= EMU_ACC_MAXB || !counts) return -1;
  for (int i = 0; i < EMU_ACC_N; ++i) counts[i] = emu_acc[m][i];
  return 0;
}
// the row algebra of the feasibility phase on its own (ipm_core.hpp): out = dz, dw, dn, da of el_step and the side's sigma, rho of el_point_side -- a unit check holds
// them against a dense solve of the side's three equations at states with z + w != rho_pen, which the solvers' trajectories hardly ever visit
extern "C" void landing_emu_el_row(double sd, double a, double n, double z, double w, double mu, double rho_pen, double ds, double* out) {
  const ElStep e = el_step(sd, a, n, z, w, mu, rho_pen, ds);
  ElAcc acc{}; double sg = 0.0, rh = 0.0;
  el_point_side(acc, sd, a, n, z, w, mu, rho_pen, sg, rh);
  out[0] = e.dz; out[1] = e.dw; out[2] = e.dn; out[3] = e.da; out[4] = sg; out[5] = rh;
}
#else
#define LANDING_EMU_COUNT(m, what) ((void)0)
#define LANDING_EMU_FUSED_ON true
#endif

struct SolveArgs {
  Layout L; int B; landing_solver_opts o; double* prof;
  int iter_cap;      // development aid (landing_debug_iter_cap): > 0 replaces the hard iteration limit
  const double* p; const double* x0;
  double* x_out; double* f_out; double* lam_out; int* status; int* iters; double* kkt;
  double* ws; size_t ws_stride;
  const unsigned long long* rterm; int rlen;                               // row-product records [rlen][256]
  const unsigned long long* ctab; const int* ctype; int c_ml, c_mid;      // packed assembly tables [type][c_ml][256] (aterm_pack), type of every stage
  const unsigned long long* ccomb;                                         // ... and the destinations summed from partial slots [type][256] (acomb_pack)
  const int* edge_map;   // compaction map of the tiled Jacobian write-out (landing_ctx::d_edge_map)
  const int* order;      // dispatch order: workgroup b solves member order[b] (hard-first, see landing_order_kernel); nullptr = identity
};

struct MemberMem {
  double *x, *xt, *dx, *gx;
  double *g, *gt, *s, *ds, *zL, *zU, *y, *yn, *sig, *rho;
  double *J, *H, *Hc, *ric, *cond;
  double *en, *ep, *wn, *wp;      // feasibility phase: violation variables of the lower / upper side of every inequality row and their multipliers
  // shadow instance of the iterate's row arrays: the first trial pass of the line search writes the accepted point's values here, and accepting
  // that point swaps the instances (mem_accept_swap); g / gt and x / xt are pairs of the same kind
  // RULE for every pass that writes row arrays: the entries the fused first-trial pass never writes -- rows 0..11 of y / sigma / rho and s / zL / zU of
  // the equality rows (lb == ub) -- must hold the SAME value in both instances at every swap (they are zero from the start: ipm_init_row, el_init_row);
  // a pass that wrote one of them in the live instance alone would change results after an odd number of swaps.  The emulation build checks this at
  // every swap (landing_ipm_kernel).
  double *sig2, *rho2, *s2, *zL2, *zU2, *y2;
};
constexpr int MEMBER_MEM_PTRS = 29;
static_assert(sizeof(MemberMem) == MEMBER_MEM_PTRS * sizeof(double*) && std::is_standard_layout<MemberMem>::value && std::is_trivially_copyable<MemberMem>::value,
              "live_mem() walks MemberMem as an array of double*: nothing but double* members");

__device__ __forceinline__ MemberMem carve(const Layout& L, double* w) {
  MemberMem M;
  M.x = w; w += L.nx; M.xt = w; w += L.nx; M.dx = w; w += L.nx; M.gx = w; w += L.nx;
  M.g = w; w += L.ng; M.gt = w; w += L.ng; M.s = w; w += L.ng; M.ds = w; w += L.ng;
  M.zL = w; w += L.ng; M.zU = w; w += L.ng;
  M.y = w; w += L.ng; M.yn = w; w += L.ng;
  M.sig = w; w += L.ng; M.rho = w; w += L.ng;
  M.J = w; w += L.nnz_jac; M.H = w; w += L.nnz_hess; M.Hc = w; w += (size_t)L.N * RUNC; M.ric = w; w += (size_t)(L.N + 1) * RIC_STRIDE; M.cond = w; w += (size_t)L.N * RCG;
  M.en = w; w += L.ng; M.ep = w; w += L.ng; M.wn = w; w += L.ng; M.wp = w; w += L.ng;
  M.sig2 = w; w += L.ng; M.rho2 = w; w += L.ng;      // ([sigma | rho] adjacent as in the first instance, and not at the end of the block: asm_issue reads up to 24 doubles behind rho)
  M.s2 = w; w += L.ng; M.zL2 = w; w += L.ng; M.zU2 = w; w += L.ng; M.y2 = w;
  return M;
}

// Accepting the point the fused first-trial pass prepared: the shadow instance of (s, zL, zU, y, sigma, rho) becomes the live one, and so do
// gt and xt.  What that pass does not write is the same in both instances from the start (rows 0..11, s / zL / zU of equality rows: zero).
__host__ __device__ __forceinline__ void mem_accept_swap(MemberMem& M) {
  double* t;
#define LANDING_SWAP(a, b) t = M.a; M.a = M.b; M.b = t
  LANDING_SWAP(s, s2); LANDING_SWAP(zL, zL2); LANDING_SWAP(zU, zU2); LANDING_SWAP(y, y2); LANDING_SWAP(sig, sig2); LANDING_SWAP(rho, rho2);
  LANDING_SWAP(g, gt); LANDING_SWAP(x, xt);
#undef LANDING_SWAP
}

// Scalar state of the interior-point loop, kept in LDS (S.ks: the fields both solvers keep, ipm_core.hpp IpmCtl) and never in registers
// across phases.  Every thread reads it in place; ONLY thread 0 writes it, inside KS_BEGIN / KS_END blocks that are fenced by barriers on
// both sides -- so the scalar control logic of the solver (error test, restarts, barrier update, regularisation schedule, filter, watchdog)
// runs once per workgroup instead of 256 times, and no value is live across a phase.  Round 2 held these ~45 scalars in VGPRs: the kernel
// body alone carried 767 static scratch (private-segment) accesses around its calls, executed every iteration by all 256 threads
// (VERDICT r2 item 8); now 233, none of them on the per-iteration path of the row passes.

// LDS of one member
constexpr int FWD_DXL_NMAX = 64;   // horizons up to this keep a copy of dx in LDS for row_products: 36 N + 12 doubles in [P | A1 | A^]
constexpr int XCH = 112 * 4;    // one exchange buffer of the blocked elimination (4 x 4 pivot blocks): pivot rows [64][4] + pivot columns [48][4]
static_assert(2 * XCH >= 24 * YS, "A1 also holds Y (24 x YS)");
struct Lds {
  double G[48 * GS];
  double P[24 * PS];
  double A1[2 * XCH];          // Y = P(:,0:12)*A^ (24 x YS = 888) while T^T P T is formed, then the exchange buffers of the blocked elimination
  double Ah[2 * 12 * YS];      // A^ of the stage being eliminated and of the one being assembled (copy k & 1 belongs to stage k)
  double gam[48], q[24], sig[24], w[48], dinv[24];      // (gam: the foot block of stage 0 only -- gamma of a stage is column 48 of G, p column 24 of P, b column 36 of A^)
  double red[(SOLVER_THREADS / 64) * 9];      // (the fused first-trial pass reduces 3 line-search sums + 6 quantities of the new point at once)
  double filt_th[FILT_CAP], filt_ph[FILT_CAP];
  double prof[32];
  int flag;
  // member context, written once by every thread with identical values (read back as LDS broadcasts by the
  // __noinline__ phases so that they carry no register state across calls)
  // assembly (asm_issue / asm_copy / asm_terms): term table of the most frequent stage type (the others are read from L2) and, per stage, the
  // bases of the seven [J | H | Hc] segments + the type id (slot 7)
  int segb[SOLVER_NMAX * 8];
  double carry[ASM_NSLOT];          // partial sums of the destinations that are summed by more than one thread
  double rcl[RCG];                  // gradient of the running cost of the stage whose G / gamma are assembled
  double jhl[CX_LEN];               // cx: nonzeros of the stage being assembled, the seven [J | H | Hc] segments side by side (coalesced copy) | sigma | rho of its rows | 1, -1, 0
  double dump[64];                  // where the stores of terms that close nothing go
  const unsigned long long* ctab; const unsigned long long* ccomb; int c_ml, c_mid, rc_on;
  // bounds of the rows: lbg/ubg depend on the row's position inside its stage only (boundary rows | rows of a stage |
  // rows of the last stage, which has another layout), so 244 (lb, ub) pairs in LDS replace two ng-long workspace arrays
  // that every row pass used to stream (6 of ~30 array passes per iteration)
  double bnd_lb[36 + 2 * 104], bnd_ub[36 + 2 * 104];
  MemberMem M; Layout L; const double* p; int prof_on;
  IpmCtl ks;
  // control fields of this solver alone (written like ks): clip_k rule in force; jam_clip (landing_nlp.h): iterations in a row with a tiny step
  // to the boundary; what the stop test decided (ACT_*); no regularisation made the last step computable
  int clip_now, jamrun, action, fact_failed;
  // fused first trial of the line search (interior-point mode): first_trial = the next trial point is the first of its iteration; fast = it was
  // accepted as it stands, so accepting is a swap of instances; nxt = errors / sums of that point (what the accept pass leaves in ks.c_*)
  int first_trial, fast;
  double nxt[6];
  unsigned long long atab_mid[ATAB_LTMAX * SOLVER_THREADS];      // (behind everything the tables address: their offsets are 16 bits)
  unsigned long long acomb_mid[SOLVER_THREADS];
};
// One instance per workgroup (= per NLP).  Namespace scope keeps the LDS address space visible to every
// phase function (ds_* instructions instead of flat_*).
__shared__ Lds SH;
// the derivative phase's copy of the multipliers (landing_ipm_kernel, eval_kernels.hip lam_lds_stage) lies over [G | P | A1 | A^]: horizons up to 44
constexpr int LAM_LDS_ROOM = 48 * GS + 24 * PS + 2 * XCH + 2 * 12 * YS;
constexpr int LAM_LDS_NMAX = (LAM_LDS_ROOM - 36) / LAM_LDS_STRIDE;
static_assert(offsetof(Lds, P) == offsetof(Lds, G) + sizeof(double) * 48 * GS && offsetof(Lds, A1) == offsetof(Lds, P) + sizeof(double) * 24 * PS &&
              offsetof(Lds, Ah) == offsetof(Lds, A1) + sizeof(double) * 2 * XCH && offsetof(Lds, gam) == offsetof(Lds, G) + sizeof(double) * LAM_LDS_ROOM,
              "G, P, A1, A^ are one contiguous range");
static_assert(lam_lds_stage(LAM_LDS_NMAX) <= LAM_LDS_ROOM && LAM_LDS_NMAX == 44, "the copy of the multipliers fits");
// The member's arrays as they are NOW (the accept step swaps instances, so no phase keeps these pointers across iterations): SH.M by value,
// every pointer moved to scalar registers -- they are the same for all lanes, and the row passes then address with scalar base + lane offset.
__device__ __forceinline__ MemberMem live_mem() {
  MemberMem M = SH.M;
#if defined(__HIP_DEVICE_COMPILE__)
  double** q = reinterpret_cast<double**>(&M);
#pragma unroll
  for (int i = 0; i < MEMBER_MEM_PTRS; ++i) {
    const unsigned long long a = (unsigned long long)q[i];
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    q[i] = (double*)((unsigned long long)lo | ((unsigned long long)hi << 32));
  }
#endif
  return M;
}
// Packed terms of the assembly tables, with every place given as a BYTE OFFSET inside the LDS block (the host builds the tables with
// offsetof: solver_capi.inc): value = [pa] * [pb] * [pc], summed into the open PIECE of a destination and stored to [d] (+ the
// distance to the second copy of A^ when `ah` is set and the stage's copy is 1); the sum restarts behind the store unless `keep`
// (the store of a term that closes nothing goes to a per-lane dump slot).  A piece is a whole destination -- an entry of G (upper
// triangle), gamma or A^ -- or one of the partial sums that asm_combine adds up in slot order (pieces are cut where the 256 equal
// chunks of rounds 1-4 were, so every sum keeps its association).
static_assert(36 * FWD_DXL_NMAX + 12 <= 24 * PS + 2 * XCH + 2 * 12 * YS && offsetof(Lds, A1) == offsetof(Lds, P) + sizeof(double) * 24 * PS && offsetof(Lds, Ah) == offsetof(Lds, A1) + sizeof(double) * 2 * XCH,
              "dx (x layout, N <= FWD_DXL_NMAX) fits the adjacent arrays [P | A1 | A^] (forward_pass / row_products)");
static_assert(offsetof(Lds, atab_mid) <= 65528, "the assembly tables address G, A^, gamma, cx, the partial sums and the dump slots with 16-bit byte offsets");
__host__ __device__ inline unsigned long long aterm_pack(int pa, int pb, int pc, int d, bool keep, bool ah) {
  const unsigned lo = (unsigned)pa | ((unsigned)pb << 16);
  const unsigned hi = (unsigned)pc | (((unsigned)d | (keep ? 1u : 0u) | (ah ? 2u : 0u)) << 16);
  return (unsigned long long)lo | ((unsigned long long)hi << 32);
}
// destination made of n partial sums (slots at byte offset s0 onwards, added in that order): lo = n | s0 << 16, hi = d | ah << 1; n = 0: nothing
__host__ __device__ inline unsigned long long acomb_pack(int n, int s0, int d, bool ah) {
  return (unsigned long long)((unsigned)n | ((unsigned)s0 << 16)) | ((unsigned long long)((unsigned)d | (ah ? 2u : 0u)) << 32);
}

// fp64 matrix-core tile: D(16x16) = C + A(16 x 4KT) B(4KT x 16) with v_mfma_f64_16x16x4_f64.  Operand layout
// (cdna_hip_programming.md section 3): lane l supplies A[i = l&15][k = l>>4] and B[k = l>>4][j = l&15]; the accumulator holds
// D[row = (l>>4) + 4r][col = l&15], r = 0..3.  fa(i,k) / fb(k,j) fetch operands (LDS, zero outside the matrix).
template <int KT, class FA, class FB>
__device__ __forceinline__ f64x4 mfma_tile(f64x4 c, FA fa, FB fb) {
  const int l = threadIdx.x & 63, ij = l & 15, kq = l >> 4;
#pragma unroll
  for (int kt = 0; kt < KT; ++kt) c = __builtin_amdgcn_mfma_f64_16x16x4f64(fa(ij, kt * 4 + kq), fb(kt * 4 + kq, ij), c, 0, 0, 0);
  return c;
}

// 1/d by v_rcp_f64 + two Newton steps (<= 1 ulp measured, tools/dev/rcp_prec.hip; the IEEE division sequence is 4x longer).
__device__ __forceinline__ double fast_rcp(double d) {
  double i = __builtin_amdgcn_rcp(d);
  i = fma(i, fma(-d, i, 1.0), i);
  return fma(i, fma(-d, i, 1.0), i);
}

// Broadcast of one lane's fp64 value to the whole wave through the scalar unit (v_readlane_b32 x2; `src` must be
// wave-uniform -- it is a compile-time constant in the unrolled elimination below).
__device__ __forceinline__ double lane_bcast(double v, int src) {
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  return __hiloint2double(hi, lo);
}

// Elimination of the controls of one stage by ONE wavefront, entirely in registers: Gauss-Jordan on
// [G_uu | G_us | gamma_u], lane c owning column c (NU + 24 + 1 <= 49 lanes, NU values each).  The pivot of step j is
// broadcast from lane j, the multipliers from lane j's column; no LDS traffic and no barrier inside the steps.
// Used for the 12 x 12 block of the free feet of stage 0 only (the stages themselves go through stage_eliminate).  On success Kl (LDS, NU x 24, row stride 24) holds
// K = G_uu^-1 G_us and kl the vector kappa = G_uu^-1 gamma_u.  A non-positive / non-finite pivot (wrong inertia)
// is reported through *flag = 0; the caller raises delta_w.
template <int NU>
__device__ __noinline__ void gauss_jordan_wave(const double* G, const double* gam, double* Kl, double* kl, int* flag) {
  const int lane = threadIdx.x;        // called by the first wave only (threadIdx.x < 64)
  double col[NU];
  const bool isUU = lane < NU, isUS = lane >= NU && lane < NU + 24, isG = lane == NU + 24;
  {   // branch-free column fetch: every lane walks its own (base, stride); idle lanes re-read column 0
    const double* src = isG ? gam + 24 : G + 24 * GS + (isUU ? 24 + lane : (isUS ? lane - NU : 0));
    const int stride = isG ? 1 : GS;
#pragma unroll
    for (int i = 0; i < NU; ++i) col[i] = src[i * stride];
  }
  bool ok = true;
  // Rolled pivot loop with a rotating row file: step j finds its pivot row in col[0]; every update writes row i
  // into slot i-1 (the FMA destination differs from its accumulator source, so the rotation costs nothing) and the
  // normalised pivot row goes to the last slot.  After NU steps the rows are back in place.  One small loop body
  // (instruction-cache resident) instead of NU unrolled copies; the lane select of the broadcasts is the loop
  // counter (scalar).
#pragma unroll 1
  for (int j = 0; j < NU; ++j) {
    const double d = lane_bcast(col[0], j);
    if (!(d > 0.0) || !(d < 1e300)) ok = false;        // wave-uniform; keep going (values are discarded)
    double inv = __builtin_amdgcn_rcp(d);               // v_rcp_f64 + two Newton steps instead of the IEEE division
    inv = fma(inv, fma(-d, inv, 1.0), inv);             // sequence: the reciprocal sits on the serial pivot chain
    inv = fma(inv, fma(-d, inv, 1.0), inv);
    const double pj = col[0] * inv;
    // multipliers first (independent scalar broadcasts, back to back), then the row updates
    double m[NU];
#pragma unroll
    for (int i = 1; i < NU; ++i) m[i] = lane_bcast(col[i], j);
    __builtin_amdgcn_sched_barrier(0);      // all broadcasts in flight before the first update consumes one
#pragma unroll
    for (int i = 1; i < NU; ++i) col[i - 1] = fma(-m[i], pj, col[i]);
    col[NU - 1] = pj;
  }
  if (isUS) {
#pragma unroll
    for (int i = 0; i < NU; ++i) Kl[i * 24 + (lane - NU)] = col[i];
  }
  if (isG) {
#pragma unroll
    for (int i = 0; i < NU; ++i) kl[i] = col[i];
  }
  if (lane == 0) *flag = ok ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Backward sweep, round 5: the ASSEMBLY of stage k - 1 rides on the elimination of stage k.
// While the four waves eliminate the controls of stage k on the matrix cores, they copy stage k - 1's CCS nonzeros, sigma / rho of its
// rows and the residual of its dynamics rows from the workspace into LDS (coalesced loads issued behind the first block step), form
// the condensation terms  G = H + J_d^T Sigma J_d, gamma = J_d^T rho, A^ = -dg_dyn/d(X,c,f)  and store them straight into G, gamma
// and the NEXT stage's copy of A^ / b between two later block steps.  Rounds 1-4 ran the condensation as a phase of its own over all
// stages (0.106 ms of the 0.727 ms an iteration took under load) that wrote a 704-double block per stage to the member's workspace,
// which the sweep read back (473 KB per member and iteration, 12 % of the kernel's HBM traffic) and scattered into G between two
// barriers at the head of every stage (0.6-0.9 us of the 7 us a stage took).  The arithmetic and its order are unchanged: results are
// bit-identical to round 4's (tools/dev/emu_ab.py).  Built on the way, measured on the GPU and rejected (profiles/r05_ab_experiments.txt):
//  * the round-4 term tables (segment / offset pairs, destination codes, carries between threads) decoded inside the block steps, operands
//    gathered from the workspace: +2.3 us per stage (60 gather instructions of 64 scattered addresses per stage); operands staged through
//    LDS first: +2.0 us (500 instructions per thread and stage): whatever the four waves execute together is on the chain, so the
//    per-term work has to be a handful of instructions;
//  * an ASSEMBLER WAVE: waves 0..2 eliminate (wave 2 carrying the right-hand-side column as a second tile), wave 3 assembles alone: the
//    elimination itself went from 5.0 to 7.2 us per stage (second tile: 148+ registers, callee-saved spills whose reloads sit in front
//    of every return) and one wave needs 1.1 us more than that for 1 280 terms.
//
// The work is described by packed 8-byte terms (aterm_pack) in stage-LOCAL form: one table per stage type (first / middle /
// penultimate / last), the middle one resident in LDS.  A thread owns whole destinations (balanced on the host: 5-6 terms per
// thread).  Rounds 1-4 cut the term list into 256 equal chunks, one per thread, and a destination whose terms straddled chunk borders
// was finished from per-thread carries in thread order; now a destination is summed by one thread, which restarts the partial sum
// where those borders were (`bnd`), so every sum keeps its association.
constexpr int ASM_SEG_LEN[7] = {NZ_JU - NZ_JX, NZ_JUN - NZ_JU, NZ_HX - NZ_JUN, NZ_HU - NZ_HX, NZ_HUN - NZ_HU, NZ_TOT - NZ_HUN, RUNC};
constexpr int ASM_SEG_POS[7] = {NZ_JX, NZ_JU, NZ_JUN, NZ_HX, NZ_HU, NZ_HUN, NZ_TOT};
static_assert(NZ_JUN - NZ_JU <= SOLVER_THREADS && 2 * 104 <= SOLVER_THREADS, "one load per thread and segment");
// What a sweep reads that is the same for every lane and every stage, fetched from the member context in LDS ONCE per sweep and kept in scalar
// registers from there on (until round 9 the assembly hooks read ctab, c_ml, c_mid, rc_on and the member's pointers back from LDS in every stage)
__device__ __forceinline__ int uni(int v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_readfirstlane(v);
#else
  return v;
#endif
}
template <class P>
__device__ __forceinline__ P uni_ptr(P q) {
  const unsigned long long a = (unsigned long long)q;
  return (P)((unsigned long long)(unsigned)uni((int)(unsigned)a) | ((unsigned long long)(unsigned)uni((int)(unsigned)(a >> 32)) << 32));
}
__device__ __forceinline__ double uni(double v) { return __hiloint2double(uni(__double2hiint(v)), uni(__double2loint(v))); }
#if defined(__HIP_DEVICE_COMPILE__)
typedef const unsigned long long __attribute__((address_space(1)))* landing_gptr_u;
#else
typedef const unsigned long long* landing_gptr_u;
#endif
struct SweepCtx {
  landing_gptr JH, SR, Gr, Cd;      // [J | H | Hc] (contiguous), [sigma | rho] (contiguous), g, gradient of the running cost
  landing_gptr_u ctab, ccomb;       // term and combine tables of the stage types that are not LDS-resident (global_load: a flat load would also count on the LDS counter)
  int c_ml, c_mid, rc_on, ng;
};
__device__ __forceinline__ SweepCtx sweep_ctx() {
  const Lds& S = SH;
  SweepCtx X;
  X.JH = uni_ptr((landing_gptr)S.M.J); X.SR = uni_ptr((landing_gptr)S.M.sig); X.Gr = uni_ptr((landing_gptr)S.M.g); X.Cd = uni_ptr((landing_gptr)S.M.cond);
  X.ctab = uni_ptr((landing_gptr_u)S.ctab); X.ccomb = uni_ptr((landing_gptr_u)S.ccomb);
  X.c_ml = uni(S.c_ml); X.c_mid = uni(S.c_mid); X.rc_on = uni(S.rc_on); X.ng = uni(S.L.ng);
  return X;
}
static_assert(ATAB_LTMAX == ATAB_TB, "a thread's terms of a stage are ONE batch: its words travel in AsmRegs");
struct AsmRegs { double jh[7], sr, g, rc; int tp; unsigned long long tw[ATAB_TB], cw; };      // (tp: the stage's type, uniform; tw, cw: the thread's term words and combine word, live from asm_copy on)
// (1) coalesced loads of stage k's nonzeros (one per segment), sigma / rho of its rows, the residual of its dynamics rows; nothing is consumed here
// (the segment bases and the type of the stage are the one thing the hooks still read from LDS per stage: segb, one round trip)
__device__ __forceinline__ void asm_issue(int k, const SweepCtx& X, AsmRegs& R) {
  const Lds& S = SH;
  const int tid = threadIdx.x, ng = X.ng;
  const int* sb = S.segb + k * 8;
  const int g0 = Layout::g_stage(k);
#pragma unroll
  for (int sgm = 0; sgm < 7; ++sgm) R.jh[sgm] = X.JH[uni(sb[sgm]) + (tid < ASM_SEG_LEN[sgm] ? tid : 0)];
  R.tp = uni(sb[7]);
  R.sr = X.SR[tid < 104 ? g0 + tid : (tid < 208 ? ng + g0 + tid - 104 : 0)];      // (the last stage has 80 rows: the tail reads the workspace behind them, never used)
  R.g = X.Gr[g0 + (tid < 12 ? tid : 0)];
  R.rc = 0.0;
  if (X.rc_on) R.rc = X.Cd[(size_t)k * RCG + (tid < RCG ? tid : 0)];
}
// (2) ... into LDS; a barrier follows before asm_terms.  The thread's packed words of the stage's TYPE (terms: asm_terms, partial-sum slots:
// asm_combine) are fetched here, one block step early, into the registers the copied values leave: they depend on the type alone, and read
// behind the barrier they were a round trip of their own in front of the operand reads, which need them for their addresses
__device__ __forceinline__ void asm_copy(const SweepCtx& X, int nb, AsmRegs& R) {
  Lds& S = SH;
  const int tid = threadIdx.x;
#pragma unroll
  for (int sgm = 0; sgm < 7; ++sgm) if (tid < ASM_SEG_LEN[sgm]) S.jhl[ASM_SEG_POS[sgm] + tid] = R.jh[sgm];
  if (tid < 208) S.jhl[CX_SR + tid] = R.sr;
  // b of copy `nb` (no term writes that column; the copy is the NEXT stage's) and the gradient of the running cost (w order X, c, f: added to gamma
  // when its tile is fetched, which every wave is past): stored here, so that every loaded value has left its register before the words arrive
  if (tid < 12) { const int i = tid; S.Ah[nb * (12 * YS) + (i < 6 ? i : (i < 9 ? i + 3 : i - 3)) * YS + (YS - 1)] = -R.g; }
  if (tid < RCG) S.rcl[tid] = R.rc;
  if (R.tp == X.c_mid) {
#pragma unroll
    for (int u = 0; u < ATAB_TB; ++u) R.tw[u] = S.atab_mid[u * SOLVER_THREADS + tid];
    R.cw = S.acomb_mid[tid];
  } else {
    const landing_gptr_u gt = X.ctab + (size_t)R.tp * X.c_ml * SOLVER_THREADS;
#pragma unroll
    for (int u = 0; u < ATAB_TB; ++u) R.tw[u] = gt[u * SOLVER_THREADS + tid];
    R.cw = X.ccomb[R.tp * SOLVER_THREADS + tid];
  }
}
// (3) products and stores: G and gamma (dead since the tile fetch of the running elimination), A^ / b of copy `nb`.  ATAB_TB terms
// at a time: all operands (the codes came with asm_copy), then the arithmetic and the stores
__device__ __forceinline__ void asm_terms(int nb, const AsmRegs& R) {
  Lds& S = SH;
  char* const lds0 = reinterpret_cast<char*>(&S);
  const unsigned ahoff = nb ? (unsigned)(12 * YS * sizeof(double)) : 0u;
  double acc = 0.0;
  {
    const unsigned long long (&t)[ATAB_TB] = R.tw;
    double a[ATAB_TB], b[ATAB_TB], c[ATAB_TB];
#pragma unroll
    for (int u = 0; u < ATAB_TB; ++u) {
      const unsigned lo = (unsigned)t[u], hi = (unsigned)(t[u] >> 32);
      a[u] = *reinterpret_cast<const double*>(lds0 + (lo & 0xffffu)); b[u] = *reinterpret_cast<const double*>(lds0 + (lo >> 16)); c[u] = *reinterpret_cast<const double*>(lds0 + (hi & 0xffffu));
    }
#pragma unroll
    for (int u = 0; u < ATAB_TB; ++u) {
      const unsigned dd = (unsigned)(t[u] >> 48);
      acc += a[u] * b[u] * c[u];
      *reinterpret_cast<double*>(lds0 + ((dd & 0xfff8u) + ((dd & 2u) ? ahoff : 0u))) = acc;
      acc = (dd & 1u) ? acc : 0.0;
    }
  }
}
// (4) behind the next barrier: the destinations whose terms more than one thread summed
__device__ __forceinline__ void asm_combine(int nb, const AsmRegs& R) {
  Lds& S = SH;
  const unsigned long long code = R.cw;
  const unsigned lo = (unsigned)code, dd = (unsigned)(code >> 32);
  const int n = (int)(lo & 7u);
  if (n > 0) {
    char* const lds0 = reinterpret_cast<char*>(&S);
    const double* sl = reinterpret_cast<const double*>(lds0 + (lo >> 16));
    double tot = 0.0;
    for (int i = 0; i < n; ++i) tot += sl[i];
    *reinterpret_cast<double*>(lds0 + ((dd & 0xfff8u) + ((dd & 2u) ? (nb ? (unsigned)(12 * YS * sizeof(double)) : 0u) : 0u))) = tot;
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
typedef double __attribute__((address_space(1)))* landing_gptr_w;
#else
typedef double* landing_gptr_w;
#endif
// A stage record's base as a global pointer in scalar registers (a __noinline__ phase receives its arguments in vector registers; the
// pointer is the same in every lane): stores through it are global_store with a scalar base and a 32-bit lane offset
__device__ __forceinline__ landing_gptr_w uniform_record(double* rec) { return uni_ptr((landing_gptr_w)rec); }

// Elimination of the controls of one stage on the matrix cores (waves 0..2): blocked Gauss-Jordan with
// 4 x 4 pivot blocks on the (NU + 24) x (NU + 25) array  [G_uu G_us gamma_u ; G_su G_ss gamma_s]  (rows/columns: controls
// first).  After NU/4 block steps the control rows hold [I | K | kappa] and the state rows hold the Schur complement
// [0 | P_k | p_k] -- gains and cost-to-go in one pass.  The array lives in v_mfma_f64_16x16x4 accumulator tiles: wave w
// owns column tile w (16 columns x 48 rows = 3 tiles; with NU = 24 the right-hand side is column 48, the only live column of
// wave 3's tile).  Returns false on a non-positive pivot (at the end of the stage).
//
// One block step (pivot_block_step): the 4 x 4 pivot block at rows / columns [OFF, OFF + 4), OFF = 4 STEP, of the tile array T (wave
// ct owns column tile ct, accumulator layout: T[rt][r] = element (row 16 rt + lk + 4 r, column 16 ct + lj)).  Exchange through LDS
// (buffer STEP & 1 of S.A1): every lane publishes the 4 pivot-row entries of its column, W[c][4]; the 4 lane-columns that hold the
// pivot columns publish them, C[row][4]; one barrier; then every lane solves D r = w for its own column with the pivot block D
// recomputed redundantly from the broadcast copy (no further communication), and the wave applies the rank-4 update T -= C R with ONE
// matrix-core instruction per tile; the pivot rows become R itself (forming them as W - (D - I) R would cancel at the scale of W).
// Rounds 2-4 factored D as L diag(d) L^T with two triangular solves; the 2 x 2 partition below has the shorter serial chain.
// 8 x 8 blocks (3 exchange + barrier rounds per stage instead of 6) were built and measured in round 3 and are
// SLOWER: the redundant per-lane factorisation grows with the cube of the block size -- about 210 fp64 operations per lane and block at
// 4 issue cycles each against 2 x 40 -- which costs more than the three barrier rounds it saves: backward sweep 0.353 instead of
// 0.293 ms per iteration with the CU to itself.
constexpr int G_GAMMA = GS - 1, P_PV = PS - 1, AH_B = YS - 1;
static_assert(G_GAMMA == 48 && P_PV == 24 && AH_B == 36, "spare columns of G / P / A^ hold gamma / p / b");

// What a lane needs to know about itself in a stage elimination: columns, LDS bases (BYTE offsets inside the LDS block) and masks.  All of it
// follows from the thread index and NU alone -- not from the member, the iteration or the stage -- so the sweep forms it once (stage_lanes)
// and every stage of its loop uses it as it stands; until round 9 each of the 40 stages of a sweep worked it out again.  The places inside A^
// are those of copy 0: a stage adds the distance to its own copy (one scalar, k & 1).
template <int NU>
struct StageLanes {
  int ct, lj, lk, c;                   // column tile (= wave, uniform), column inside the tile, lane group, column
  bool isg, live, ym, pm, wr;          // the gamma lane; live column; lanes with an operand in A^ | b / in P | p; lanes that write the stage out
  bool am[3];                          // rows (one per row tile) that have a column of A^
  int gb, cd384, cm;                   // tile fetch: base of the own column of [G | gamma]; 48 * 8 * (position of the column - lk); c - lk
  int yb, pa1, pb, p2, fb, ab[3];      // operands of T^T P T and of the closed-loop map
  int xw, xw0, xcp, xcr;               // exchange buffers of the block steps: own pivot-row entry, own pivot rows, published pivot column, pivot-column operand
  unsigned iK, iM, iP, rs;             // write-out: byte offsets of the lane's first entry of K | kappa, Mt | mv, P_x | p in the record, byte stride of a row
  int sw, pw;                          //            own column of A^ | b and of P | p
};
template <int NU>
__device__ __forceinline__ StageLanes<NU> stage_lanes() {
  constexpr int NR = NU + 24, D = (int)sizeof(double);
  constexpr int oG = (int)offsetof(Lds, G), oP = (int)offsetof(Lds, P), oAh = (int)offsetof(Lds, Ah), oA1 = (int)offsetof(Lds, A1);
  StageLanes<NU> Z;
  const int tid = threadIdx.x, l = tid & 63;
  Z.ct = uni(tid >> 6); Z.lj = l & 15; Z.lk = l >> 4;
  const int ct = Z.ct, lj = Z.lj, lk = Z.lk, c = 16 * ct + lj;
  Z.c = c;
  Z.isg = (c == NR); Z.live = (c <= NR);
  const bool isg = Z.isg, live = Z.live;
  // position of the own column in G; its column of A^ | b (state and force columns, b for gamma); its column of P | p (columns of c+, p for gamma)
  const int cl = c < NR ? c : NR;
  const int cp = NU == 24 ? cl : (cl < NU ? cl : cl + (24 - NU));
  Z.ym = live && (c < 12 || c >= NU);
  int ycol = c < NU ? c + 24 : c - NU;
  ycol = Z.ym ? (isg ? AH_B : ycol) : 0;
  Z.pm = live && c >= 12 && (c < NU || isg);
  const int pcol = Z.pm ? (isg ? P_PV : c) : 0;
  Z.gb = oG + (cp + lk * GS) * D; Z.cd384 = (cp - lk) * ((GS - 1) * D); Z.cm = c - lk;
  Z.yb = oAh + (lk * YS + ycol) * D;
  Z.pa1 = oP + (lj * PS + lk) * D;
  Z.pb = oP + (lk * PS + pcol) * D;
#pragma unroll
  for (int rt = 0; rt < 3; ++rt) {
    const int rho = 16 * rt + lj;
    const int a = rho < NU ? 24 + rho : (rho < NR ? rho - NU : 36);      // column of A^ that belongs to row rho (none for the rows of c+ and the dead rows)
    Z.am[rt] = a < 36;
    Z.ab[rt] = oAh + (lk * YS + (Z.am[rt] ? a : 0)) * D;
  }
  // (A-operand rows 12..15 feed rows 12..15 of the products, which nothing reads: those lanes re-read row 11 instead of a zero)
  Z.p2 = oP + ((12 + (lj < 12 ? lj : 11)) * PS + lk) * D;
  Z.fb = oAh + ((lj < 12 ? lj : 11) * YS + 24 + lk) * D;
  Z.xw = oA1 + (c * 4 + lk) * D; Z.xw0 = oA1 + (c * 4) * D; Z.xcp = oA1 + (64 * 4 + lk * 4 + lj) * D; Z.xcr = oA1 + (64 * 4 + lj * 4 + lk) * D;
  // Which field a row goes to is known per accumulator; a lane differs only in "state column or gamma", which is a base and a row stride of its
  // own (K + sj, stride 24, against kappa, stride 1; alike Mt / mv and P_x / p).  Wave 0 (columns < NU) writes nothing.
  Z.wr = c >= NU && c <= NR;
  const unsigned sj = (unsigned)(c - NU), ulk = (unsigned)lk, rs = isg ? 1u : 24u;
  Z.rs = rs * D;
  Z.iK = ((isg ? (unsigned)RIC_KAP : (unsigned)RIC_K + sj) + ulk * rs) * D; Z.iM = ((isg ? (unsigned)RIC_MV : (unsigned)RIC_MT + sj) + ulk * rs) * D;
  Z.iP = ((isg ? (unsigned)RIC_PV : (unsigned)RIC_PX + sj) + ulk * rs) * D;
  const int scol = isg ? AH_B : (int)sj, pcw = isg ? P_PV : (int)sj;
  Z.sw = oAh + (lk * YS + scol) * D; Z.pw = oP + (lk * PS + pcw) * D;
  return Z;
}
__device__ __forceinline__ double lds_get(int boff) { return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(&SH) + boff); }
__device__ __forceinline__ void lds_put(int boff, double v) { *reinterpret_cast<double*>(reinterpret_cast<char*>(&SH) + boff) = v; }

// Returns the inertia key of the block: the largest of the four biased high words of a00, det A, s00, det S -- the block is accepted when it is
// below PIVOT_KEY_MAX, and a stage when the largest key of its blocks is (one compare per stage; identical in every lane of the workgroup).
constexpr unsigned PIVOT_KEY_MAX = 0x7e37e43cu - 0x00100000u;
template <int STEP, int NU>
__device__ __forceinline__ unsigned pivot_block_step(f64x4 (&T)[3], const StageLanes<NU>& Z) {
  constexpr int OFF = 4 * STEP, D = (int)sizeof(double);
  static_assert((OFF >> 4) == ((OFF + 3) >> 4), "a pivot block lies inside one row tile");
  constexpr int RTB = OFF >> 4, R0 = (OFF & 15) >> 2;
  constexpr int WSZ = 64 * 4;
  static_assert(WSZ + 48 * 4 <= XCH, "exchange buffer");
  constexpr int XB = (STEP & 1) * XCH * D;                               // buffer STEP & 1 of S.A1: W at its head, C behind WSZ doubles
  constexpr int CB = (int)offsetof(Lds, A1) + XB + WSZ * D;
  const bool inblk = (unsigned)(Z.lj - (OFF & 15)) < 4u;                 // lane column inside the pivot block's columns (of its tile)
  lds_put(Z.xw + XB, T[RTB][R0]);
  if (Z.ct == RTB && inblk) {
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) lds_put(Z.xcp + XB + ((16 * rt + 4 * r) * 4 - (OFF & 15)) * D, T[rt][r]);
  }
  __syncthreads();
  // pivot block (uniform reads), pivot rows of the own column, pivot-column operands
  double a[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) a[i][j] = lds_get(CB + ((OFF + i) * 4 + j) * D);
  double w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = lds_get(Z.xw0 + XB + i * D);
  double am[3];
#pragma unroll
  for (int rt = 0; rt < 3; ++rt) { const double cv = lds_get(Z.xcr + XB + 16 * rt * 4 * D); am[rt] = (rt == RTB && inblk) ? 0.0 : cv; }   // pivot rows: no update
  auto recip = [](double d) { double i = __builtin_amdgcn_rcp(d); i = fma(i, fma(-d, i, 1.0), i); return fma(i, fma(-d, i, 1.0), i); };
  // The 4 x 4 pivot block through its 2 x 2 partition  D = [A B^T; B C]:  A^-1 from its determinant, E = B A^-1, Schur complement S = C - E B^T, S^-1 from its
  // determinant, then  r_2 = S^-1 (w_2 - E w_1),  r_1 = A^-1 w_1 - E^T r_2.  Two reciprocals on the serial chain instead of four and ~24 dependent operations
  // instead of ~64 of the LDL^T + two triangular solves (every lane computes this between the barrier and its matrix-core update: it is latency, not
  // throughput).  Inertia: the four leading principal minors a00, det A, det A * s00, det A * det S are positive exactly when the four pivots of the
  // unblocked elimination are (Sylvester), so the test -- a00, det A, s00, det S in (2^-1022, ~1e300) -- accepts the same matrices up to rounding.
  const double a00 = a[0][0], a10 = a[1][0], a11 = a[1][1], a20 = a[2][0], a21 = a[2][1], a22 = a[2][2], a30 = a[3][0], a31 = a[3][1], a32 = a[3][2], a33 = a[3][3];
  const double detA = fma(a00, a11, -a10 * a10), iA = recip(detA);
  const double e00 = fma(a20, a11, -a21 * a10) * iA, e01 = fma(a21, a00, -a20 * a10) * iA, e10 = fma(a30, a11, -a31 * a10) * iA, e11 = fma(a31, a00, -a30 * a10) * iA;
  const double s00 = fma(-e01, a21, fma(-e00, a20, a22)), s10 = fma(-e11, a21, fma(-e10, a20, a32)), s11 = fma(-e11, a31, fma(-e10, a30, a33));
  const double detS = fma(s00, s11, -s10 * s10), iS = recip(detS);
  unsigned hm = 0u;
  { const double piv[4] = {a00, detA, s00, detS};
#pragma unroll
    for (int j = 0; j < 4; ++j) { const unsigned h = (unsigned)__double2hiint(piv[j]) - 0x00100000u; hm = h > hm ? h : hm; } }
  // normalised pivot row of the own column: D r = w, lane group lk keeps r[lk]
  const int lk = Z.lk;
  auto solve = [&](const double (&wv)[4]) {
    const double t2 = fma(-e01, wv[1], fma(-e00, wv[0], wv[2])), t3 = fma(-e11, wv[1], fma(-e10, wv[0], wv[3]));
    const double r2 = fma(s11, t2, -s10 * t3) * iS, r3 = fma(s00, t3, -s10 * t2) * iS;
    const double q0 = fma(a11, wv[0], -a10 * wv[1]) * iA, q1 = fma(a00, wv[1], -a10 * wv[0]) * iA;
    const double r0 = fma(-e10, r3, fma(-e00, r2, q0)), r1 = fma(-e11, r3, fma(-e01, r2, q1));
    return lk == 0 ? r0 : (lk == 1 ? r1 : (lk == 2 ? r2 : r3));
  };
  const double R = solve(w);
  if (16 * Z.ct + 16 > OFF) {                            // (uniform) tiles whose columns are all eliminated already stay as they are
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) T[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(am[rt], -R, T[rt], 0, 0, 0);
    T[RTB][R0] = R;                                      // the pivot rows become the normalised rows, exactly
  }
  return hm;
}

// (`k` = stage, its copy of A^ | b is k & 1; the assembly of stage k - 1 rides along)
//
// Where the operands sit (the host's assembly tables, solver_capi.inc, and the epilogue below write them there):
//  * G holds the condensed stage array in ELIMINATION order -- rows / columns (f, c+, sigma), upper triangle --
//    with gamma in the spare column GS - 1 = 48.  Element (rho, c) of the symmetric array [G | gamma] is therefore
//    G[min(rho, c) * GS + max(rho, c)] = G[48 min(rho, c) + rho + c] for the columns of G AND for the gamma lane (c = 48).  The last
//    stage (no c+) uses the same positions, its rows / columns skip the c+ range: the patterns of the stages still nest along the sweep.
//  * P carries p in its spare column PS - 1 = 24, A^ carries b in its spare column YS - 1 = 36: the gamma lane reads its operands
//    with the formula of the other lanes, at a column of its own.
// Every fetch below is then ONE per-lane base, formed once per sweep from (lj, lk, ct) (stage_lanes), plus a compile-time offset; a lane without an operand
// (dead column, structural zero) loads from a clamped column and drops the value under a lane mask.  Until round 8 every fetch chose
// its index through nested conditions on the lane, which the compiler turned into about 30 instructions of exec-mask branches per load.
// Store to a stage record through its base in scalar registers and a 32-bit BYTE offset of the lane (global_store, scalar base + lane offset)
__device__ __forceinline__ void rec_put(landing_gptr_w rec, unsigned boff, double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef char __attribute__((address_space(1)))* gchar_w;
  *reinterpret_cast<landing_gptr_w>(reinterpret_cast<gchar_w>(rec) + boff) = v;
#else
  *reinterpret_cast<double*>(reinterpret_cast<char*>(rec) + boff) = v;
#endif
}
// `rec`, `delta`, `k` and X are uniform (scalar registers); returns whether every pivot was positive, uniform as well.
template <int NU>
__device__ __forceinline__ bool stage_eliminate(const StageLanes<NU>& Z, const SweepCtx& X, landing_gptr_w rec, double delta, int k) {
  constexpr int NR = NU + 24, D = (int)sizeof(double);          // rows; column NR is gamma
  const int lk = Z.lk;
  const bool isg = Z.isg, live = Z.live, ym = Z.ym, pm = Z.pm;
  const int cb = k & 1;
  const int ah = cb * (12 * YS * D);                             // distance to the stage's copy of A^ | b
  f64x4 T[3];
  {   // tile fetch: every lane walks its own column of [G | gamma]; delta_w on the diagonal
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rb = 16 * rt + 4 * r;                                  // (compile-time after unrolling) row rho = rb + lk
        if (rb < NR) {
          const int rp = NU == 24 ? rb : (rb < NU ? rb : rb + (24 - NU));      // its position in G, less lk
          const int m384 = rp * ((GS - 1) * D) < Z.cd384 ? rp * ((GS - 1) * D) : Z.cd384;      // (GS - 1) * 8 * min(rp, position of the column - lk)
          const double v = lds_get(Z.gb + rp * D + m384) + (Z.cm == rb ? delta : 0.0);
          T[rt][r] = live ? v : 0.0;
        } else T[rt][r] = 0.0;
      }
    if (X.rc_on) {      // (uniform) + gradient of the running cost of the stage's variables (X, c, f) in the column of gamma
      Lds& S = SH;
#pragma unroll
      for (int rt = 0; rt < 3; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rb = 16 * rt + 4 * r;
          if (rb < NR) {
            const int ab = rb < NU ? 24 + rb : rb - NU;                  // index of row rb in the (sigma, f, c+) order of the gradient
            static_assert(RCG % 4 == 0 && NU % 4 == 0, "a group of four rows lies on one side of every border");
            const double g = ab < RCG ? S.rcl[ab + lk] : 0.0;
            T[rt][r] += isg ? g : 0.0;
          }
        }
    }
  }
  {   // + T^T P T and T^T (P b + p) of the next stage's cost-to-go, formed where it is consumed.  With
      // A_ext = [A^ | b] (12 rows) the own column of Y = P(:,0:12) A_ext comes out of the matrix cores in accumulator
      // layout, which IS the B-operand layout of the next product (row 4kt+k of k-step kt sits in lane group k):
      // Y never touches LDS.  Columns of c+ and the p-part of gamma enter P T directly.
    double be[3];
    {
      const int yb = Z.yb + ah;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) { const double v = lds_get(yb + 4 * kt * YS * D); be[kt] = ym ? v : 0.0; }
    }
    double pa1[3], add1[3];
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) pa1[kt] = lds_get(Z.pa1 + 4 * kt * D);
#pragma unroll
    for (int r = 0; r < 3; ++r) { const double v = lds_get(Z.pb + 4 * r * PS * D); add1[r] = pm ? v : 0.0; }
    double av[3][3];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt) {
      const int ab = Z.ab[rt] + ah;
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) { const double v = lds_get(ab + 4 * kt * YS * D); av[rt][kt] = Z.am[rt] ? v : 0.0; }
    }
    double pa2[3], add2[3];
    if (NU == 24) {
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) pa2[kt] = lds_get(Z.p2 + 4 * kt * D);
#pragma unroll
      for (int r = 0; r < 3; ++r) { const double v = lds_get(Z.pb + (12 + 4 * r) * PS * D); add2[r] = pm ? v : 0.0; }
    }
    f64x4 Y1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) Y1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa1[kt], be[kt], Y1, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) Y1[r] += add1[r];
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) T[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[rt][kt], Y1[kt], T[rt], 0, 0, 0);
    if (NU == 24) {   // rows of c+ (control rows 12..23): + rows 12..23 of P T
      f64x4 Y2 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kt = 0; kt < 3; ++kt) Y2 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa2[kt], be[kt], Y2, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 3; ++r) Y2[r] += add2[r];
      T[0][3] += Y2[0]; T[1][0] += Y2[1]; T[1][1] += Y2[2];
    }
  }
  // assembly of stage k - 1 (asm_issue / asm_copy / asm_terms / asm_combine): loads behind the first block step (every wave is past
  // the tile fetch: G and gamma are free), LDS copy before block step SC, whose barrier publishes it, products and stores behind
  // that step, sums of several threads behind the next one.
  // A non-positive pivot does not end the stage early: the sweep is abandoned by the caller, a few block steps later
  static_assert(NU == 12 || NU == 24, "3 or 6 block steps per stage");
  constexpr int SC = NU == 24 ? 3 : 1;
  AsmRegs nxt;
  const bool more = k > 0;                               // (uniform)
#define ASM_HOOK(step) do { if constexpr (SC == (step)) { if (more) asm_copy(X, cb ^ 1, nxt); } if constexpr (SC + 1 == (step)) { if (more) asm_terms(cb ^ 1, nxt); } if constexpr (SC + 2 == (step)) { if (more) asm_combine(cb ^ 1, nxt); } } while (0)
  unsigned key = pivot_block_step<0>(T, Z), kq;
#define KEY_MAX(e) do { kq = (e); key = kq > key ? kq : key; } while (0)
  if (more) asm_issue(k - 1, X, nxt);
  ASM_HOOK(1);
  KEY_MAX(pivot_block_step<1>(T, Z));
  ASM_HOOK(2);
  KEY_MAX(pivot_block_step<2>(T, Z));
  ASM_HOOK(3);
  if constexpr (NU == 24) {
    KEY_MAX(pivot_block_step<3>(T, Z));
    ASM_HOOK(4);
    KEY_MAX(pivot_block_step<4>(T, Z));
    ASM_HOOK(5);
    KEY_MAX(pivot_block_step<5>(T, Z));
  }
#undef KEY_MAX
#undef ASM_HOOK
  if (!((unsigned)uni((int)key) < PIVOT_KEY_MAX)) return false;      // (the key is identical in every lane: a scalar test)
  // closed-loop state map for the forward sweep: X+ = A^_sigma sigma + A^_f f + b with f = -(K_f sigma + kappa_f), i.e.
  // Mt = A^_sigma - A^_f K_f, mv = b - A^_f kappa_f.  K_f / kappa_f are rows 0..11 of the first row tile, already in
  // B-operand layout (k-step kt = accumulator kt).  (Rows 12..15 of the product are not read: their lanes re-read row 11 of A^.)
  f64x4 Mq = {0.0, 0.0, 0.0, 0.0};
  {
    const int fb = Z.fb + ah;
#pragma unroll
    for (int kt = 0; kt < 3; ++kt) Mq = __builtin_amdgcn_mfma_f64_16x16x4f64(lds_get(fb + 4 * kt * D), T[0][kt], Mq, 0, 0, 0);
  }
  // Mt | mv and the gains to the stage record, cost-to-go to LDS (+ its state rows to the record): one store per accumulator under ONE lane
  // mask.  Nothing waits for these stores: the forward sweep is the first to read the record.
  if (Z.wr) {
    const int sw = Z.sw + ah;
#pragma unroll
    for (int r = 0; r < 3; ++r) rec_put(rec, Z.iM + (unsigned)(4 * r) * Z.rs, lds_get(sw + 4 * r * YS * D) - Mq[r]);
#pragma unroll
    for (int rt = 0; rt < 3; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rb = 16 * rt + 4 * r;                                    // (compile-time) row rho = rb + lk
        const double v = T[rt][r];
        if (rb < NU) rec_put(rec, Z.iK + (unsigned)rb * Z.rs, v);
        else if (rb < NR) {
          lds_put(Z.pw + (rb - NU) * PS * D, v);
          if (rb - NU < 12) rec_put(rec, Z.iP + (unsigned)(rb - NU) * Z.rs, v);
        }
      }
  }
  return true;
}

// The last stage (NU = 12: no c+) is eliminated once per sweep, out of line, with lane constants of its own
__device__ __noinline__ bool last_stage_eliminate(double* rec_, double delta_, int k_) {
  const StageLanes<12> Z = stage_lanes<12>();
  const SweepCtx X = sweep_ctx();
  return stage_eliminate<12>(Z, X, uniform_record(rec_), uni(delta_), uni(k_));
}

// The stages N - 2 .. 0 of a sweep (NU = 24: controls (f_k, c_{k+1})): ONE resident loop with the elimination inlined -- no call, no return
// and no wait for the record's stores per stage; the record's base, delta, the context X and the loop condition live in scalar registers,
// the lane constants Z in vector registers.  Two instances: the timed one (profile buffer set) reads the clock around every stage, the
// other carries no trace of the timers.  `n_try` counts the eliminations attempted.
template <bool TIMED>
__device__ __forceinline__ bool stage_loop(const StageLanes<24>& Z, const SweepCtx& X, landing_gptr_w rec, double delta, int k, int& n_try) {
  bool ok = true;
  for (; k >= 0 && ok; --k, rec -= RIC_STRIDE) {
    long long tb_ = 0;
    if (TIMED) tb_ = (long long)wall_clock64();
    ok = stage_eliminate<24>(Z, X, rec, delta, k);
    __syncthreads();
    ++n_try;
    if (TIMED) { const long long n_ = (long long)wall_clock64(); if (threadIdx.x == 0) SH.prof[PH_B_ELIM] += (double)(n_ - tb_); }
  }
  return ok;
}

// One backward Riccati sweep with regularisation delta (terminal cost-to-go, stages N-1..0, free feet of
// stage 0).  false = a pivot was not positive (wrong inertia): the caller raises delta and retries.
__device__ __noinline__ bool riccati_backward(double delta) {
  Lds& S = SH;
  const Layout& L = S.L;
  const MemberMem& M = S.M;
  const double* p = S.p;
  const int N = L.N, lane = threadIdx.x, NT = blockDim.x;
  (void)p; (void)N; (void)lane; (void)NT;
  bool ok = true;
  int n_try = 0;      // stage eliminations attempted in this sweep (all but the last one succeeded, and that one iff ok): counted in S.prof once, at the end
  // terminal cost-to-go on sigma_N = X_N: diagonal (terminal rows are copies of X_N, gen:94-97)
  for (int e = lane; e < 24 * PS; e += NT) S.P[e] = 0.0;
  __syncthreads();
  if (lane < 12) {
    const int i = lane;
    const int ra = i < 6 ? 12 + i : 24 + (i - 6), rb = i < 6 ? 18 + i : 30 + (i - 6);
    const double qn2 = S.ks.feas ? 0.0 : 2.0 * p[L.o_QN + i];      // (the feasibility phase has no objective)
    S.P[i * PS + i] = qn2 + M.sig[ra] + M.sig[rb] + delta;
    S.P[i * PS + P_PV] = qn2 * (M.x[12 * N + i] - p[12 * N + i]) + M.rho[ra] + M.rho[rb];      // p_N in the spare column of P (rows 12..23 stay 0)
    double* rec = M.ric + (size_t)N * RIC_STRIDE;      // record N: P_N (diag), p_N
    for (int j = 0; j < 24; ++j) rec[RIC_PX + i * 24 + j] = (j == i) ? S.P[i * PS + i] : 0.0;
    rec[RIC_PV + i] = S.P[i * PS + P_PV];
  }
  // background of the condensed stage data: the scatter below writes the structural nonzeros only (the patterns
  // of the stages nest along the sweep unless the tables say otherwise), nothing else writes G / A^ any more
  for (int e = lane; e < 48 * GS; e += NT) S.G[e] = 0.0;
  for (int e = lane; e < 2 * 12 * YS; e += NT) S.Ah[e] = 0.0;
  __syncthreads();
  const SweepCtx X = sweep_ctx();
  const bool timed = uni(S.prof_on) != 0;
  {   // the only exposed assembly of the sweep
    AsmRegs first;
    asm_issue(N - 1, X, first);
    asm_copy(X, (N - 1) & 1, first);
    __syncthreads();
    asm_terms((N - 1) & 1, first);
    __syncthreads();
    asm_combine((N - 1) & 1, first);
  }
  __syncthreads();
  // ---- per stage: G + T^T P T, elimination of the controls: P_k, p_k, gains -> record k; the assembly of stage k - 1 rides along
  {
    long long tb_ = timed ? (long long)wall_clock64() : 0;
    ok = uni(last_stage_eliminate(M.ric + (size_t)(N - 1) * RIC_STRIDE, delta, N - 1) ? 1 : 0) != 0;
    __syncthreads();
    ++n_try;
    if (timed) { const long long n_ = (long long)wall_clock64(); if (lane == 0) S.prof[PH_B_ELIM] += (double)(n_ - tb_); }
  }
  if (ok && N > 1) {
    const StageLanes<24> Z = stage_lanes<24>();
    const int Nu = uni(N);
    const landing_gptr_w rec = uniform_record(M.ric) + (size_t)(Nu - 2) * RIC_STRIDE;
    const double du = uni(delta);
    ok = timed ? stage_loop<true>(Z, X, rec, du, Nu - 2, n_try) : stage_loop<false>(Z, X, rec, du, Nu - 2, n_try);
  }
  if (ok) {
    // ---- stage 0: X_0 fixed, feet c_0 free: P_cc dc0 = -(p_c + P_cx dX0), same elimination on a 12x12 block
    if (lane < 12) {
      const int i = lane;
      const double x0i = (i < 6) ? p[L.o_q_init + i] : p[L.o_qd_init + i - 6];
      S.sig[i] = x0i - M.x[i];
    }
    for (int e = lane; e < 144; e += NT) { const int i = e / 12, j = e % 12; S.G[(24 + i) * GS + 24 + j] = S.P[(12 + i) * PS + 12 + j]; }
    __syncthreads();
    if (lane < 12) {
      double v = S.P[(12 + lane) * PS + P_PV];
      for (int t = 0; t < 12; ++t) v += S.P[(12 + lane) * PS + t] * S.sig[t];
      S.gam[24 + lane] = v;
    }
    __syncthreads();
    if (lane < 64) gauss_jordan_wave<12>(S.G, S.gam, S.A1, S.A1 + 24 * 24, &S.flag);
    __syncthreads();
    ok = S.flag != 0;
    ++n_try;
    if (ok) {
      if (lane < 12) S.sig[12 + lane] = -S.A1[24 * 24 + lane];
      __syncthreads();
    }
  }
  if (lane == 0) { S.prof[PH_NSTAGE] += (double)n_try; S.prof[PH_NSTAGE_OK] += (double)(ok ? n_try : n_try - 1); }
  __syncthreads();
  return ok;
}

// Forward sweep: dx of every stage, next states, multipliers of the dynamics rows.
// The serial part is the state recursion alone: sigma_{k+1} = [Mt; -K_c] sigma_k + [mv; -kappa_c] (one 24 x 24
// product and one barrier per stage; the 612 doubles of a stage are prefetched four stages ahead into registers
// and passed on through a double-buffered LDS slot).  The forces f_k = -(K_f sigma_k + kappa_f) and the multipliers
// of the dynamics rows y_k = -(P_{k+1} sigma_{k+1} + p_{k+1})_X do not feed the recursion: they are evaluated for
// all stages at once afterwards.
__device__ __noinline__ void forward_pass() {
  Lds& S = SH;
  const Layout& L = S.L;
  const MemberMem& M = S.M;
  const int N = uni(L.N), tid = threadIdx.x, NT = blockDim.x;
  double* sg = S.G;                    // sigma_k, k = 0..N  at sg[24 k]           (N <= SOLVER_NMAX = 96: 2328 of the 2352 doubles of G)
  double* buf = S.jhl;                 // two stage slots of RIC_FWDN doubles: the assembler's copy of a stage's nonzeros (free here) and A1
  double* buf1 = S.A1;
  static_assert(24 * (SOLVER_NMAX + 1) <= 48 * GS && RIC_FWDN <= NZ_TOT + RUNC && RIC_FWDN <= XCH * 2, "forward scratch fits");
  auto slot = [&](int k) { return (k & 1) ? buf1 : buf; };
  // The record base of the sweep lives in scalar registers (uniform_record, as in riccati_backward): the prefetch address of a stage is scalar
  // arithmetic on it, the member context in LDS is not read inside the loop.  global_load: a flat load would also tie up the LDS counter
  const landing_gptr fwd0 = (landing_gptr)uniform_record(M.ric) + RIC_FWD0;
  int fe[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) { const int e = tid + j * 256; fe[j] = e < RIC_FWDN ? e : RIC_FWDN - 1; }
  auto fetch = [&](int k, double (&r)[3]) {
    const landing_gptr rec = fwd0 + (size_t)(k < N ? k : N - 1) * RIC_STRIDE;
#pragma unroll
    for (int j = 0; j < 3; ++j) r[j] = rec[fe[j]];      // unconditional (clamped): the memory counter stays countable
  };
  auto stash = [&](int k, const double (&r)[3]) {
    double* b = slot(k);
#pragma unroll
    for (int j = 0; j < 3; ++j) { const int e = tid + j * 256; if (k < N && e < RIC_FWDN) b[e] = r[j]; }
  };
  if (tid < 24) sg[tid] = S.sig[tid];
  double r0[3], r1[3], r2[3], r3[3];
  fetch(0, r0); fetch(1, r1); fetch(2, r2); fetch(3, r3);
  stash(0, r0); fetch(4, r0);
  __syncthreads();
  // Lane constants of the recursion: lane (r, j) sums entries 3j..3j+2 of row r of [Mt; -K_c]; a stage reads its row, sigma_k AND the bias of
  // its row in one batch of LDS reads, the 8-lane sum stays in the vector ALU (lane_sum8_head) and the two cases of a row (state row: bias +
  // sum, c+ row: -(bias + sum), 0 behind the last stage) are selects on the loaded value -- one trip through the LDS pipe per stage, not six
  const int fr = tid >> 3, fj = tid & 7;
  const bool frow = tid < 192, fstate = fr < 12, fhead = frow && fj == 0;
  const int f_row = (fstate ? 312 + fr * 24 : (fr - 12) * 24) + 3 * fj;      // slot layout: [0,288) K rows of c+ | [288,312) kappa | [312,600) Mt | [600,612) mv
  const int f_bias = fstate ? 600 + fr : 300 + (fr - 12);
  auto stage = [&](int k, double (&rn)[3]) {
    // rn holds stage k+1 (loaded four stages ago): hand it to LDS, refill it with stage k+5
    if (k < N) {
      const double* b = slot(k);
      const bool lastk = (k == N - 1);
      if (frow) {
        const double* row = b + f_row;
        const double* sk = sg + 24 * k + 3 * fj;
        double bias = b[f_bias];
        double prod = row[0] * sk[0] + row[1] * sk[1] + row[2] * sk[2];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(bias), "+v"(prod));      // the bias arrives with the products: without this the compiler sinks its read behind the sum, into the storing lanes' branch
#endif
        const double acc = lane_sum8_head(prod);
        const double v = bias + acc;
        if (fhead) sg[24 * (k + 1) + fr] = fstate ? v : (lastk ? 0.0 : -v);
      }
    }
    stash(k + 1, rn);
    fetch(k + 5, rn);
    __syncthreads();
  };
  for (int k0 = 0; k0 < N; k0 += 4) {
    stage(k0, r1); stage(k0 + 1, r2); stage(k0 + 2, r3); stage(k0 + 3, r0);
  }
  // ---- everything that hangs off the states, all stages at once.  Round 6: dx also goes to LDS in the x layout ([P | A1 | A^] are free from here to the next backward sweep) for
  // row_products, whose gathers of dx were one of its two remaining global gathers per term (horizons up to FWD_DXL_NMAX; longer ones gather from the workspace as before)
  double* const dxl = S.P;
  const bool use_dxl = N <= FWD_DXL_NMAX;
  for (int e = tid; e < 24 * (N + 1); e += NT) {
    const int k = e / 24, i = e % 24;
    if (i < 12) { M.dx[L.x_X(k) + i] = sg[e]; if (use_dxl) dxl[L.x_X(k) + i] = sg[e]; }
    else if (k < N) { M.dx[L.x_U(k) + (i - 12)] = sg[e]; if (use_dxl) dxl[L.x_U(k) + (i - 12)] = sg[e]; }
  }
  for (int e = tid; e < 24 * N; e += NT) {
    const int k = e / 24, h = e % 24, i = h % 12;
    const double* sk = sg + 24 * (h < 12 ? k : k + 1);
    if (h < 12) {            // forces of stage k
      landing_gptr rec = (landing_gptr)(M.ric + (size_t)k * RIC_STRIDE);
      double acc = rec[RIC_KAP + i];
#pragma unroll
      for (int t = 0; t < 24; ++t) acc += rec[RIC_K + i * 24 + t] * sk[t];
      M.dx[L.x_U(k) + 12 + i] = -acc;
      if (use_dxl) dxl[L.x_U(k) + 12 + i] = -acc;
    } else {                 // multipliers of the dynamics rows of stage k (state order -> row order)
      landing_gptr recn = (landing_gptr)(M.ric + (size_t)(k + 1) * RIC_STRIDE);
      double acc = recn[RIC_PV + i];
#pragma unroll
      for (int t = 0; t < 24; ++t) acc += recn[RIC_PX + i * 24 + t] * sk[t];
      const int q = i < 6 ? i : (i < 9 ? i + 3 : i - 3);
      M.yn[L.g_stage(k) + q] = -acc;
    }
  }
  if (tid < 12) {
    const int i = tid;
    const double v = sg[24 * N + i];
    const int ra = i < 6 ? 12 + i : 24 + (i - 6), rb = i < 6 ? 18 + i : 30 + (i - 6);
    M.ds[ra] = v + (M.g[ra] - M.s[ra]);
    M.ds[rb] = v + (M.g[rb] - M.s[rb]);
  }
  __syncthreads();
}

// ds = J_d dx + (g - s) for every stage inequality row: fixed per-thread term lists over the whole horizon (chunks cut at row
// boundaries), 8-byte records {jac index (16 bits) | x index (16) | dst row (16) | closes (1) | valid (1)}, batches of 8 terms
// with the records of the next batch fetched under the gathers of this one.  (Tried in round 2: the stage-local LDS
// table scheme of condense() -- one term per thread and stage, carries through LDS, a barrier per 4 stages -- is slower
// here, alone 0.065 vs 0.039 ms and under load 0.105 vs 0.091: the list is short, 15 k terms, and latency-bound.)
__device__ __noinline__ void row_products(const unsigned long long* __restrict__ rterm, int rlen) {
  Lds& S = SH;
  const MemberMem& M = S.M;
  const int tid = threadIdx.x, NT = blockDim.x;
  const double* __restrict__ Jn = M.J; const double* __restrict__ dxv = M.dx;
  const double* dxl = S.P; const bool use_dxl = S.L.N <= FWD_DXL_NMAX;      // dx in LDS, x layout (forward_pass)
  double* __restrict__ dsv = M.ds;      // (round 6: the `+ (g - s)` of a row is added by the dual pass, which loads g and s of every row anyway -- two of the four gathers per term are gone)
  double acc = 0.0;
  constexpr int BW = 8;
  unsigned long long tn[BW];
#pragma unroll
  for (int u = 0; u < BW; ++u) tn[u] = (u < rlen) ? rterm[(size_t)u * NT + tid] : 0ull;
  for (int j0 = 0; j0 < rlen; j0 += BW) {
    unsigned long long t[BW];
#pragma unroll
    for (int u = 0; u < BW; ++u) t[u] = tn[u];
#pragma unroll
    for (int u = 0; u < BW; ++u) { const int j = j0 + BW + u; tn[u] = (j < rlen) ? rterm[(size_t)j * NT + tid] : 0ull; }
    double a[BW], b[BW];
#pragma unroll
    for (int u = 0; u < BW; ++u) {
      const int ij = (int)(t[u] & 0xffffu), ix = (int)((t[u] >> 16) & 0xffffu);
      a[u] = Jn[ij]; b[u] = use_dxl ? dxl[ix] : dxv[ix];
    }
#pragma unroll
    for (int u = 0; u < BW; ++u) {
      const bool valid = (t[u] >> 49) & 1ull, closes = (t[u] >> 48) & 1ull;
      acc += valid ? a[u] * b[u] : 0.0;
      if (closes) { dsv[(int)((t[u] >> 32) & 0xffffu)] = acc; acc = 0.0; }
    }
  }
  __syncthreads();
}

// Running-cost pieces of the solver (landing_form.run_cost, generate_quadruped_SRBM_CCC.m:81-89): out of line -- cold for the default
// terminal-cost objective, and their 36-entry gradient arrays stay out of the register allocation of the main loop.
__device__ __noinline__ void rc_init_hc() {      // constant Hessian entries of the running cost (layout: RUNC)
  const Layout& L = SH.L; const double* p = SH.p;
  for (int e = threadIdx.x; e < L.N * RUNC; e += blockDim.x) {
    const int k = e / RUNC, j = e % RUNC, a = j % 3;
    const double dt2 = 2.0 * p[L.o_dt + k];
    double v;
    if (j < 12) v = dt2 * (rc_QX(L, p, j) + (j < 3 ? 4.0 * rc_Qc(L, p, j) : 0.0));
    else if (j < 24) v = -dt2 * rc_Qc(L, p, a);
    else if (j < 36) v = dt2 * rc_Qc(L, p, a);
    else v = dt2 * rc_Qf(L, p, a);
    SH.M.Hc[e] = v;
  }
}
__device__ __noinline__ void rc_add_grad() {     // objective gradient of the stage variables into gx
  const Layout& L = SH.L; const MemberMem& M = SH.M;
  for (int k = threadIdx.x; k < L.N; k += blockDim.x) { double* gU = M.gx + L.x_U(k); (void)run_cost_stage(L, M.x, SH.p, k, M.gx + L.x_X(k), gU, gU + 12); }
}
__device__ __noinline__ void rc_add_gamma() {    // ... and, per stage, for the right-hand sides gamma_k (w order X, c, f): added when the tile of gamma is fetched (stage_eliminate)
  const Layout& L = SH.L; const MemberMem& M = SH.M;
  for (int k = threadIdx.x; k < L.N; k += blockDim.x) {
    double gr[36];
#pragma unroll
    for (int a = 0; a < 36; ++a) gr[a] = 0.0;
    (void)run_cost_stage(L, M.x, SH.p, k, gr, gr + 12, gr + 24);
    double* gm = M.cond + (size_t)k * RCG;
#pragma unroll
    for (int a = 0; a < 36; ++a) gm[a] = gr[a];
  }
}
__device__ __noinline__ void rc_f_dphi(double& f0, double& dphi) {     // running cost at x and its directional derivative along dx (per-thread partial sums)
  const Layout& L = SH.L; const MemberMem& M = SH.M;
  for (int k0 = 0; k0 < L.N; k0 += blockDim.x) {
    const int k = k0 + threadIdx.x;
    if (k >= L.N) continue;
    double gr[36];
#pragma unroll
    for (int a = 0; a < 36; ++a) gr[a] = 0.0;
    f0 += run_cost_stage(L, M.x, SH.p, k, gr, gr + 12, gr + 24);
    const double* dX = M.dx + L.x_X(k); const double* dU = M.dx + L.x_U(k);
#pragma unroll
    for (int a = 0; a < 12; ++a) dphi += gr[a] * dX[a] + gr[12 + a] * dU[a] + gr[24 + a] * dU[12 + a];
  }
}
__device__ __noinline__ double rc_f(const double* x) {                 // running cost at x (per-thread partial sum)
  const Layout& L = SH.L;
  double f = 0.0;
  // (uniform trip count with a lane predicate: a loop whose trip count differs per lane right in front of the block
  // reduction hung the kernel on gfx950 / ROCm 7.2 even with the branch not taken -- bisected, tools/dev)
  for (int k0 = 0; k0 < L.N; k0 += blockDim.x) { const int k = k0 + threadIdx.x; if (k < L.N) f += run_cost_stage(L, x, SH.p, k, nullptr, nullptr, nullptr); }
  return f;
}

// Workgroups per CU the register budget is sized for.  Measured on MI355X (N = 40, end of round 1, IPRA off): 2 per CU
// (256 VGPRs) beats 3 (168) at batch 1024 -- 5220 vs 4760 NLPs/s -- and ties beyond (2048: 5410 vs 5330, 8192: 7080 vs
// 7050); 4 per CU (128 VGPRs, and the 46 KB of LDS would only fit three) is far behind.  Every phase is latency-bound:
// more resident workgroups mostly add contention, and the row passes / derivative phases spill less with 256 registers.
constexpr int SOLVER_MIN_WAVES = 2;
// Receding-horizon shift (SURVEY 8f row N3 / BASELINE configs[4]): the initial guess of the next control tick is the previous
// solution advanced by one stage -- X(:,k) <- X(:,k+1), U(:,k) <- U(:,k+1), the last column held -- with the measured state
// in X(:,0); the parameter vector gets the new q_init / qd_init.  (The reference's warm-start variant re-solves from the stored
// previous solution unshifted, codegen_casadi/test_loadCasadi_ws.m:73-88; the shift is what a 100 Hz loop adds.)
__global__ void landing_mpc_shift_kernel(Layout L, int B, const double* __restrict__ x_prev, const double* __restrict__ state,
                                         double* __restrict__ p, double* __restrict__ x0) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)B * L.nx) return;
  const int m = (int)(idx / L.nx), i = (int)(idx % L.nx), N = L.N, nX = 12 * (N + 1);
  const double* xp = x_prev + (size_t)m * L.nx;
  double v;
  if (i < 12) v = state[(size_t)m * 12 + i];
  else if (i < nX) { const int k = i / 12, r = i % 12; v = xp[12 * (k < N ? k + 1 : N) + r]; }
  else { const int j = i - nX, k = j / 24, r = j % 24; v = xp[nX + 24 * (k < N - 1 ? k + 1 : N - 1) + r]; }
  x0[idx] = v;
  if (i < 6) p[(size_t)m * L.np + L.o_q_init + i] = v;
  else if (i < 12) p[(size_t)m * L.np + L.o_qd_init + (i - 6)] = v;
}

// Dispatch order of a batch: workgroups are handed to the CUs in blockIdx order and a batch larger than the resident
// capacity (2 workgroups per CU) runs in waves, so the batch time is the finishing time of the slowest member -- which
// is much later when that member only starts in the second wave.  Members likely to need many iterations go first.
// Difficulty proxy = initial body height z0 = q_init(3) (it grows with |pitch| and the drop speed through the callers'
// touch-down rule, generate_training_data_automated.m:52-60): correlation 0.65 with the iteration count on the bench
// batches (round-2 measurement), as good as what a 30-iteration probe predicts.  rank = number of members with a larger
// key (ties: lower index first) -- O(B^2) comparisons, deterministic, no atomics.  NaN keys sort last.  The keys lie np doubles apart: a
// workgroup stages them in LDS, ORDER_THREADS at a time, instead of every thread walking the strided column itself.
constexpr int ORDER_THREADS = 256;
__global__ void __launch_bounds__(ORDER_THREADS) landing_order_kernel(Layout L, int B, const double* __restrict__ p, int* __restrict__ order) {
  __shared__ double keys[ORDER_THREADS];
  const int tid = threadIdx.x, m = blockIdx.x * ORDER_THREADS + tid;
  const int off = L.o_q_init + 2;
  double key = m < B ? p[(size_t)m * L.np + off] : 0.0;
  if (!(key == key)) key = -INFINITY;
  int rank = 0;
  for (int j0 = 0; j0 < B; j0 += ORDER_THREADS) {
    double kj = j0 + tid < B ? p[(size_t)(j0 + tid) * L.np + off] : 0.0;
    if (!(kj == kj)) kj = -INFINITY;
    keys[tid] = kj;
    __syncthreads();
    const int n = B - j0 < ORDER_THREADS ? B - j0 : ORDER_THREADS;
    for (int j = 0; j < n; ++j) rank += (keys[j] > key) || (keys[j] == key && j0 + j < m);
    __syncthreads();
  }
  if (m < B) order[rank] = m;
}

__global__ void __launch_bounds__(SOLVER_THREADS, SOLVER_MIN_WAVES) landing_ipm_kernel(SolveArgs A) {
  if ((int)blockIdx.x >= A.B) return;
  const int m = A.order ? A.order[blockIdx.x] : (int)blockIdx.x;
  const Layout& L = A.L;
  const int N = L.N, lane = threadIdx.x, NT = blockDim.x;
  const int nx = L.nx, ng = L.ng;
  const double* p = A.p + (size_t)m * L.np;
  const landing_solver_opts& o = A.o;
  // the layout of the member's block; which instance of a swapped array is live is in S.M alone (mem_accept_swap): the set-up below runs before
  // any swap and uses M directly, everything from the main loop on takes the pointers from live_mem()
  const MemberMem M = carve(L, A.ws + (size_t)m * A.ws_stride);
  Lds& S = SH;
  const double INF = INFINITY;
  auto bidx = [N](int r) { if (r < 36) return r; const int k = (r - 36) / 104, q = (r - 36) - 104 * k; return 36 + (k == N - 1 ? 104 : 0) + q; };
  // the workspace arrays never overlap: tell the compiler so that the row passes can batch their loads
#define ROW_PTRS(M) double* __restrict__ r_g = (M).g; double* __restrict__ r_gt = (M).gt; double* __restrict__ r_s = (M).s; double* __restrict__ r_ds = (M).ds; \
  double* __restrict__ r_zL = (M).zL; double* __restrict__ r_zU = (M).zU; double* __restrict__ r_y = (M).y; double* __restrict__ r_yn = (M).yn; \
  double* __restrict__ r_sig = (M).sig; double* __restrict__ r_rho = (M).rho; \
  (void)r_g; (void)r_gt; (void)r_s; (void)r_ds; (void)r_zL; (void)r_zU; (void)r_y; (void)r_yn; (void)r_sig; (void)r_rho
  S.M = M; S.L = L; S.p = p; S.prof_on = A.prof != nullptr;
  S.ctab = A.ctab; S.ccomb = A.ccomb; S.c_ml = A.c_ml; S.c_mid = A.c_mid; S.rc_on = 0;
  if (lane < SOLVER_THREADS) S.acomb_mid[lane] = A.ccomb[A.c_mid * SOLVER_THREADS + lane];
  for (int e = lane; e < 64; e += NT) S.dump[e] = 0.0;
  for (int e = lane; e < A.c_ml * SOLVER_THREADS; e += NT) S.atab_mid[e] = A.ctab[(size_t)A.c_mid * A.c_ml * SOLVER_THREADS + e];      // term table of the most frequent stage type
  if (lane == 0) { S.jhl[CX_ONE] = 1.0; S.jhl[CX_MONE] = -1.0; S.jhl[CX_ZERO] = 0.0; }
  if (lane < 32) S.prof[lane] = 0.0;
#ifndef __HIPCC__
  if (lane == 0 && m < EMU_ACC_MAXB) for (int i = 0; i < EMU_ACC_N; ++i) emu_acc[m][i] = 0;
#endif
  {   // condensation: segment bases of every stage, packed term table of the most frequent stage type
    const int nj = L.nnz_jac, nh = L.nnz_hess;
    for (int k = lane; k < N; k += NT) {
      int* sb = S.segb + k * 8;
      sb[0] = L.jx(k); sb[1] = L.ju(k); sb[2] = k < N - 1 ? L.ju(k + 1) : 0;
      sb[3] = nj + L.hx(k); sb[4] = nj + L.hu(k); sb[5] = k < N - 1 ? nj + L.hu(k + 1) : 0;
      sb[6] = nj + nh + k * RUNC; sb[7] = A.ctype[k];
    }
  }
  __syncthreads();

  // ------------------------------------------------------------------ initial point
  for (int i = lane; i < nx; i += NT) {
    double v = A.x0[(size_t)m * nx + i];
    if (i < 6) v = p[L.o_q_init + i]; else if (i < 12) v = p[L.o_qd_init + i - 6];   // X(:,1) is fixed (gen:90-91)
    M.x[i] = v;
  }
  for (int e = lane; e < 36 + 2 * 104; e += NT) {
    const int r = e < 36 ? e : (e < 36 + 104 ? L.g_stage(0) + (e - 36) : L.g_stage(N - 1) + (e - 36 - 104));
    double lb = 0.0, ub = 0.0;
    if (r < ng) bound_of(L, p, r, lb, ub);          // (the last stage has 80 rows: the tail of its slot is never addressed)
    S.bnd_lb[e] = lb; S.bnd_ub[e] = ub;
  }
  __syncthreads();
  if (L.run_cost) rc_init_hc();
  __syncthreads();
  member_eval_g_rare(L, M.x, p, M.g);
  __syncthreads();
  // slacks pushed into the interior, z = 1, y = z_U - z_L, y_dyn = 0; back: at the point a feasibility phase hands back (ipm_init_row)
  auto init_slacks = [&](bool back, double mu_) {
    const MemberMem M = live_mem();
    for (int r = lane; r < ng; r += NT) { const double lb = S.bnd_lb[bidx(r)], ub = S.bnd_ub[bidx(r)]; ipm_init_row(M, r, r >= 12 && lb != ub, lb, ub, o, back, mu_); }
    __syncthreads();
  };
  init_slacks(false, 0.0);
  // the shadow instance starts as zeros: rows 0..11 and s / zL / zU of the equality rows, which no pass writes, then agree with the live instance for good
  for (int r = lane; r < ng; r += NT) { M.s2[r] = 0.0; M.zL2[r] = 0.0; M.zU2[r] = 0.0; M.y2[r] = 0.0; M.sig2[r] = 0.0; M.rho2[r] = 0.0; }
  // primal / complementarity errors, Sigma and rho of the CURRENT point for barrier parameter mu_ (one pass over the
  // rows; the accept pass below produces the same quantities for the next iterate, so this runs only at the start,
  // after a multiplier reset and when mu changes)
  IpmCtl& K = S.ks;
  // K is written by thread 0 only, between barriers (all other threads only read it, after the closing barrier)
#define KS_BEGIN() __syncthreads(); if (lane == 0) {
#define KS_BEGIN_SYNCED() if (lane == 0) {      /* directly behind a barrier (block_reduce / block_top4 end with one) */
#define KS_END() } __syncthreads()
  // Row passes: every thread owns the rows lane + NT j.  They are processed RB at a time with ALL loads of a batch issued
  // up-front and unconditionally (every array is fully allocated; out-of-range rows re-read the last row and are masked):
  // one memory round trip per batch instead of two or three dependent ones per row behind the bound-type branches.
  constexpr int RB = 4;
  // primal / complementarity errors, Sigma and rho of the CURRENT point for barrier parameter mu_ (one pass over the
  // rows; the accept pass below produces the same quantities for the next iterate, so this runs only at the start,
  // after a multiplier reset and when mu changes).  Leaves c_pr, c_co, c_cm, |y|_1, |z|_1 and the number of bound multipliers in K.
  // the same for the elastic problem of the feasibility phase (plain row loops: the phase is rare); also leaves the violation of the
  // inequality rows at x (max norm, 1-norm) and |z + w - rho_pen|_inf in K
  auto feas_point_pass = [&](double mu_) {
    const MemberMem M = live_mem();
    ROW_PTRS(M);
    ElAcc e{};
    for (int r = lane; r < ng; r += NT) {
      double sg = 0.0, rh = 0.0;
      if (r >= 12) el_point_row(e, M, r, S.bnd_lb[bidx(r)], S.bnd_ub[bidx(r)], mu_, o.feas_rho, sg, rh);
      r_sig[r] = sg; r_rho[r] = rh;
    }
    el_point_finish(K, e, S.red);
  };
  auto point_pass = [&](double mu_) {
    if (K.feas) { feas_point_pass(mu_); return; }
    const MemberMem M = live_mem();
    ROW_PTRS(M);
    double pr = 0.0, co = 0.0, cm = 0.0, ys = 0.0, zs = 0.0, nz = 0.0;
    for (int rb = lane; rb < ng; rb += NT * RB) {
      double lbv[RB], ubv[RB], gv[RB], sv[RB], zlv[RB], zuv[RB], yv[RB];
#pragma unroll
      for (int j = 0; j < RB; ++j) { const int r = rb + j * NT, rr = r < ng ? r : ng - 1; lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_g[rr]; sv[j] = r_s[rr]; zlv[j] = r_zL[rr]; zuv[j] = r_zU[rr]; yv[j] = r_y[rr]; }
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const int r = rb + j * NT;
        if (r >= ng) continue;
        const double lb = lbv[j], ub = ubv[j];
        double sg = 0.0, rh = 0.0;
        if (r >= 12) {
          const double g = gv[j];
          ys += fabs(yv[j]);
          if (lb == ub) pr = fmax(pr, fabs(g - lb));
          else {
            const double s = sv[j];
            pr = fmax(pr, fabs(g - s));
            if (lb > -INF) { const double d = s - lb, rd = fast_rcp(d), zl = zlv[j]; co = fmax(co, d * zl); cm = fmax(cm, fabs(d * zl - mu_)); sg += zl * rd; rh -= mu_ * rd; zs += zl; nz += 1.0; }
            if (ub < INF) { const double d = ub - s, rd = fast_rcp(d), zu = zuv[j]; co = fmax(co, d * zu); cm = fmax(cm, fabs(d * zu - mu_)); sg += zu * rd; rh += mu_ * rd; zs += zu; nz += 1.0; }
            rh += sg * (g - s);
          }
        }
        r_sig[r] = sg; r_rho[r] = rh;
      }
    }
    double v[6] = {pr, co, cm, ys, zs, nz}; const int op[6] = {RMAX, RMAX, RMAX, RSUM, RSUM, RSUM};
    block_reduce<6>(v, op, S.red);
    KS_BEGIN_SYNCED() K.c_pr = v[0]; K.c_co = v[1]; K.c_cm = v[2]; K.c_ys = v[3]; K.c_zs = v[4]; K.c_nz = fmax(v[5], 1.0); KS_END();
  };

  if (lane == 0) {
    ipm_init(K, o);
    if (A.iter_cap > 0) { K.hard_lim = A.iter_cap; if (K.lim > K.hard_lim) K.lim = K.hard_lim; }      // development aid (landing_debug_iter_cap)
    K.tp = A.prof ? (long long)wall_clock64() : 0;
    S.clip_now = 0; S.jamrun = 0; S.fact_failed = 0; S.first_trial = 0; S.fast = 0;
  }
  __syncthreads();
  // the lane = stage phases are called by the lanes that have work only: the callee-saved registers an out-of-line function touches
  // are saved and restored in scratch memory by every lane that is active at the call
  const int nst = N > 36 ? N : 36;

  for (;;) {
    // ---------------------------------------------------------------- derivatives at (x, y)
    const MemberMem M = live_mem();      // (every block below that runs behind a possible swap or keeps row pointers takes its own)
    if (A.prof && lane == 0) K.tp = (long long)wall_clock64();
    // (round 2: the coalesced tile write-out of landing_sweep_kernel<0> was tried here for the Jacobian task -- eval_task_jac_tiled,
    // tiles in the dead G array -- and is slower: 0.049 vs 0.039 ms alone, 0.094 vs 0.085 under load; every lane then runs the
    // full middle-stage stream and the wave serialises on 24 tile flushes, while the scattered stores of this version drain
    // asynchronously behind the arithmetic of the other two waves)
    // The multipliers the J^T y task and the Hessian tasks read come from LDS: [G | P | A1 | A^] are dead here (riccati_backward clears or rewrites
    // all four before it reads them, row_products was the last reader of the dx copy), and lane = stage reads of the workspace array touch 40 cache
    // lines per instruction.  One coalesced pass, stage k to lam_lds_stage(k); longer horizons read the workspace as before.
    const bool lam_lds = N <= LAM_LDS_NMAX;      // (uniform)
    if (lam_lds) {
      const landing_gptr yg = (landing_gptr)M.y;
      double* const yl = S.G;
      constexpr int YB = 8;
      for (int rb = lane; rb < ng; rb += NT * YB) {
        double yv[YB];
#pragma unroll
        for (int j = 0; j < YB; ++j) { const int r = rb + j * NT; yv[j] = yg[r < ng ? r : ng - 1]; }
#pragma unroll
        for (int j = 0; j < YB; ++j) {
          const int r = rb + j * NT;
          if (r < ng) yl[r < 36 ? r : r + (r - 36) / 104 * (LAM_LDS_STRIDE - 104)] = yv[j];
        }
      }
      __syncthreads();
    }
    if ((lane & 63) < nst) member_eval_jh(L, M.x, p, M.y, M.J, M.H, M.gx, nullptr, nullptr, K.feas ? 0.0 : 1.0, lam_lds, (landing_lds_cptr)S.G);
    __syncthreads();
    if (L.run_cost && !K.feas) { rc_add_grad(); __syncthreads(); }   // objective gradient of the stage variables (the terminal part is in member_eval_jh)
    PROF_ADD(PH_EVAL, K.tp);
    // ---------------------------------------------------------------- optimality error (unscaled)
    if (K.it == 0) point_pass(K.mu);
    {
      double du = 0.0;
      for (int i = lane + 12; i < nx; i += NT) du = fmax(du, fabs(M.gx[i]));
      du = block_reduce1(du, RMAX, S.red);
      KS_BEGIN_SYNCED()      // ---- what happens with this iterate: stop, restart, into / out of the feasibility phase, or another iteration
        ipm_errors(K, o, du);
        S.action = ipm_decide(K, o, S.fact_failed != 0);      // (a failed factorisation hands over through fact_failed: the solve ends NUMERICAL or enters the phase)
        S.fact_failed = 0;
      KS_END();
    }
    if (S.action == ACT_STOP) break;
    if (S.action == ACT_FEAS) {
      // ---- enter the feasibility phase from the current point (from the caller's initial guess when the iterate is not finite)
      double big = 0.0;
      for (int i = lane; i < nx; i += NT) { const double v = fabs(M.x[i]); big = fmax(big, v < 1e6 ? v : 1e300); }
      big = block_reduce1(big, RMAX, S.red);
      if (!(big < 1e6)) {
        for (int i = lane; i < nx; i += NT) {
          double v = A.x0[(size_t)m * nx + i];
          if (i < 6) v = p[L.o_q_init + i]; else if (i < 12) v = p[L.o_qd_init + i - 6];
          M.x[i] = v;
        }
      }
      __syncthreads();
      member_eval_g_rare(L, M.x, p, M.g);
      if (L.run_cost) for (int e = lane; e < N * RUNC; e += NT) M.Hc[e] = 0.0;      // no objective: its constant Hessian entries leave the condensation
      __syncthreads();
      for (int r = lane + 12; r < ng; r += NT) el_init_row(M, r, S.bnd_lb[bidx(r)], S.bnd_ub[bidx(r)], o.mu_init, o.feas_rho);
      __syncthreads();
      point_pass(K.mu);
      continue;
    }
    if (S.action == ACT_BACK) {
      // ---- a feasible point (or negligible violation): the interior-point solve restarts from it
      if (L.run_cost) rc_init_hc();
      for (int r = lane + 12; r < ng; r += NT) if (S.bnd_lb[bidx(r)] == S.bnd_ub[bidx(r)]) M.y[r] = 0.0;
      __syncthreads();
      init_slacks(o.feas_ret_push > 0.0, K.mu);
      point_pass(K.mu);
      continue;
    }
    if (S.action == ACT_RESET) {
      if (K.fresh) {
        for (int i = lane; i < nx; i += NT) {
          double v = A.x0[(size_t)m * nx + i];
          if (i < 6) v = p[L.o_q_init + i]; else if (i < 12) v = p[L.o_qd_init + i - 6];
          M.x[i] = v;
        }
        __syncthreads();
        member_eval_g_rare(L, M.x, p, M.g);
        __syncthreads();
      }
      init_slacks(false, 0.0);
      point_pass(K.mu);
      continue;
    }
    // ---------------------------------------------------------------- barrier parameter (monotone)
    for (;;) {
      KS_BEGIN() K.flag = ipm_barrier_update(K, o, ng - 12) ? 1 : 0; KS_END();
      if (!K.flag) break;
      point_pass(K.mu);                     // complementarity error, Sigma, rho for the new mu
    }
    PROF_ADD(PH_ERR, K.tp);

    // (the condensation G_k = H_k + J_d^T Sigma J_d, gamma_k, A^_k is part of the backward sweep: cond_issue / cond_finish)
    { const int rc = (L.run_cost && !K.feas) ? 1 : 0; if (lane == 0) S.rc_on = rc; if (rc) rc_add_gamma(); __syncthreads(); }   // gradient of the running cost for the stage right-hand sides
    PROF_ADD(PH_SIGRHO, K.tp);
    // ================================================================ Riccati factorisation with inertia correction
    // IPOPT's inertia-correction schedule (ipm_core.hpp); o.sticky_delta = 1: when the first trial of the previous iteration failed, start from delta_last itself
    KS_BEGIN()
      ipm_first_delta(K, o, (o.sticky_delta && K.first_failed) ? 1.0 : ipm_delta_dec(K, o), (!L.run_cost && !K.feas) ? o.delta_floor : 0.0);      // (proximal term of the terminal-cost form, landing_nlp.h)
      S.prof[PH_NFACT] += 1.0;
    KS_END();
    for (;;) {
      const bool ok = riccati_backward(K.delta);
      KS_BEGIN()
        K.flag = ipm_next_delta(K, o, ok, 0.0) ? 1 : 0;
        if (K.flag) S.prof[PH_NFACT] += 1.0;
      KS_END();
      if (!K.flag) break;
    }
    if (!K.fact_ok) {      // the step cannot be computed: give up (status NUMERICAL), or -- once -- continue in the feasibility phase
      KS_BEGIN() K.status = K.stalled ? LANDING_STALLED : LANDING_NUMERICAL; S.fact_failed = (o.feas_phase && !K.feas_used && !K.feas) ? 1 : 0; KS_END();
      if (S.fact_failed) continue;
      break;
    }
    KS_BEGIN() ipm_commit_delta(K, o, 0.0); KS_END();
    PROF_ADD(PH_BACK, K.tp);

    forward_pass();
    row_products(A.rterm, A.rlen);

    PROF_ADD(PH_FWD, K.tp);
    // ================================================================ dual steps, step bounds, merit data
    // fraction-to-the-boundary as tau / max(-ds/d), tau / max(-dz/z): reciprocals instead of divisions in the row
    // loop, one logarithm per row (log of the product of the two distances)
    // clip_k rule (landing_nlp.h): while the point is far from feasible the step length comes from the clip_k-th largest
    // ratio |ds| / distance; the slacks with a larger one stop at (1 - tau) of their distance (omt > 0 in the passes below)
    {
      const MemberMem M = live_mem();
      ROW_PTRS(M);
      const double mu = K.mu;
      const bool feas = K.feas != 0;
      const bool clip_now = !feas && K.clip_k_cur > 1 && (K.c_pr > o.clip_until || (o.jam_clip > 0 && S.jamrun >= o.jam_clip));      // far from feasible, or jammed (landing_nlp.h)
      double top[4] = {0.0, 0.0, 0.0, 0.0};
      double m_pr = 0.0, m_du = 0.0, th0 = 0.0, bar = 0.0, dphi = 0.0;
      double f0 = 0.0;
      if (feas) {      // elastic rows: steps of the eliminated variables, step bounds (a, n, b, q and their multipliers stay positive), merit data
        const double frho = o.feas_rho;
        for (int r = lane + 12; r < ng; r += NT) {
          const double lb = S.bnd_lb[bidx(r)], ub = S.bnd_ub[bidx(r)], g = r_g[r];
          if (lb == ub) { th0 += fabs(g - lb); continue; }
          const double s = r_s[r];
          double ds = r_ds[r];
          if (r >= 36) { ds = ds + (g - s); r_ds[r] = ds; }      // row_products left J_d dx: the row's `+ (g - s)` is added here (the terminal rows 12..35 are complete)
          th0 += fabs(g - s);
          if (lb > -INF) {
            const double n = M.en[r], a = s - lb + n, z = r_zL[r], w = M.wn[r];
            const ElStep e = el_step(1.0, a, n, z, w, mu, frho, ds);
            m_pr = fmax(m_pr, fmax(-e.da / a, -e.dn / n)); m_du = fmax(m_du, fmax(-e.dz / z, -e.dw / w));
            bar -= log(a * n); dphi += frho * e.dn - mu * (e.da / a + e.dn / n); f0 += frho * n;
          }
          if (ub < INF) {
            const double q = M.ep[r], b = ub + q - s, z = r_zU[r], w = M.wp[r];
            const ElStep e = el_step(-1.0, b, q, z, w, mu, frho, ds);
            m_pr = fmax(m_pr, fmax(-e.da / b, -e.dn / q)); m_du = fmax(m_du, fmax(-e.dz / z, -e.dw / w));
            bar -= log(b * q); dphi += frho * e.dn - mu * (e.da / b + e.dn / q); f0 += frho * q;
          }
        }
      } else
      for (int rb = lane + 12; rb < ng; rb += NT * RB) {
        double lbv[RB], ubv[RB], gv[RB], sv[RB], dsv[RB], zlv[RB], zuv[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) { const int r = rb + j * NT, rr = r < ng ? r : ng - 1; lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_g[rr]; sv[j] = r_s[rr]; dsv[j] = r_ds[rr]; zlv[j] = r_zL[rr]; zuv[j] = r_zU[rr]; }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          if (rb + j * NT >= ng) continue;
          const double lb = lbv[j], ub = ubv[j], g = gv[j];
          if (lb == ub) { th0 += fabs(g - lb); continue; }
          const double s = sv[j];
          double ds = dsv[j];
          { const int r = rb + j * NT; if (r >= 36) { ds = ds + (g - s); r_ds[r] = ds; } }      // row_products left J_d dx: the row's `+ (g - s)` is added here (the terminal rows 12..35 are complete)
          th0 += fabs(g - s);
          double dprod = 1.0;
          if (lb > -INF) {
            const double d = s - lb, rd = fast_rcp(d), zl = zlv[j];
            const double dz = fma(-zl * rd, ds, mu * rd - zl);
            m_pr = fmax(m_pr, -ds * rd); top4_push(top, -ds * rd);
            m_du = fmax(m_du, -dz * fast_rcp(zl));
            dprod = d; dphi -= mu * ds * rd;
          }
          if (ub < INF) {
            const double d = ub - s, rd = fast_rcp(d), zu = zuv[j];
            const double dz = fma(zu * rd, ds, mu * rd - zu);
            m_pr = fmax(m_pr, ds * rd); top4_push(top, ds * rd);
            m_du = fmax(m_du, -dz * fast_rcp(zu));
            dprod *= d; dphi += mu * ds * rd;
          }
          bar -= log(dprod);
        }
      }
      if (lane < 12 && !feas) {
        const double d = M.x[12 * N + lane] - p[12 * N + lane], qn = p[L.o_QN + lane];
        f0 = qn * d * d; dphi += 2.0 * qn * d * M.dx[12 * N + lane];
      }
      if (L.run_cost && !feas) rc_f_dphi(f0, dphi);
      double v[6] = {m_pr, m_du, th0, bar, dphi, f0}; const int op[6] = {RMAX, RMAX, RSUM, RSUM, RSUM, RSUM};
      block_reduce<6>(v, op, S.red);
      if (clip_now) block_top4(top, S.red);         // (uniform: clip_now comes from K)
      KS_BEGIN_SYNCED()
        const double tau = K.tau;
        double a_pr = (v[0] > tau) ? tau / v[0] : 1.0;
        K.a_du = (v[1] > tau) ? tau / v[1] : 1.0;
        if (clip_now) {
          const double rk = top[(K.clip_k_cur > 4 ? 4 : K.clip_k_cur) - 1];
          a_pr = (rk > tau) ? tau / rk : 1.0;
        }
        K.a_pr = a_pr;
        S.clip_now = clip_now ? 1 : 0; K.omt = clip_now ? 1.0 - tau : -1.0;
        K.th0 = v[2]; K.dphi = v[4]; K.ph0 = v[5] + mu * v[3];
        if (K.th_max == 0.0) K.th_max = 1e4 * fmax(1.0, v[2]);
        // line search state
        K.alpha = a_pr; K.s_corr = 0.0; K.accepted = 0; K.armijo_step = 0; K.ls_done = a_pr > 1e-10 ? 0 : 1;
        S.first_trial = (feas || !LANDING_EMU_FUSED_ON) ? 0 : 1; S.fast = 0;
      KS_END();
    }
    PROF_ADD(PH_DUAL, K.tp);
    // ================================================================ filter line search
    // The FIRST trial point of an iteration is nearly always the one accepted (1.001 trial points per iteration on the bench batches), and what the
    // accept pass computes for it -- s, zL, zU, y, Sigma, rho of the new point and its error sums -- depends on the step lengths and on gt only, not
    // on the outcome of the test.  So in interior-point mode the first trial pass does the accept pass's work as well (same expressions, s_corr = 0),
    // into the shadow instance; if ipm_ls_test takes the point as it stands, accepting it is a swap of instances (below) instead of a third walk
    // over the rows.  A rejected first trial leaves the shadow values to be overwritten; back-tracking, the slack correction, the fallback step and
    // the feasibility phase go through the accept pass as before.
    while (!K.ls_done) {
      const MemberMem M = live_mem();
      ROW_PTRS(M);
      const double alpha = K.alpha, omt = K.omt, mu = K.mu;
      const bool fused = S.first_trial != 0;      // (uniform; cleared in the control section behind the reduction)
      if (lane == 0) S.prof[PH_NTRIAL] += 1.0;
      for (int i = lane; i < nx; i += NT) M.xt[i] = M.x[i] + alpha * M.dx[i];
      __syncthreads();
      if (lane < nst) member_eval_g(L, M.xt, p, M.gt);
      __syncthreads();
      double tht = 0.0, bt = 0.0, ft = 0.0;
      double npr = 0.0, nco = 0.0, ncm = 0.0, nys = 0.0, nzs = 0.0, nnz = 0.0;      // (fused first trial: errors and sums of the new point)
      const bool feas = K.feas != 0;
      if (feas) {      // elastic rows at the trial step length: theta over all rows, merit = rho_pen (n + q) - mu sum of logs (mu applied below)
        const double frho = o.feas_rho;
        for (int r = lane + 12; r < ng; r += NT) {
          const double lb = S.bnd_lb[bidx(r)], ub = S.bnd_ub[bidx(r)], g = r_gt[r];
          if (lb == ub) { tht += fabs(g - lb); continue; }
          const double s0 = r_s[r], ds = r_ds[r], s = s0 + alpha * ds;
          tht += fabs(g - s);
          if (lb > -INF) { const double n0 = M.en[r]; const ElStep e = el_step(1.0, s0 - lb + n0, n0, r_zL[r], M.wn[r], mu, frho, ds); const double n = n0 + alpha * e.dn; bt -= log((s - lb + n) * n); ft += frho * n; }
          if (ub < INF) { const double q0 = M.ep[r]; const ElStep e = el_step(-1.0, ub + q0 - s0, q0, r_zU[r], M.wp[r], mu, frho, ds); const double q = q0 + alpha * e.dn; bt -= log((ub + q - s) * q); ft += frho * q; }
        }
      } else if (fused) {
        // trial pass + accept pass of this trial point in one walk: rows 12.. under the trial pass's ownership (rows lane + 12 + j NT); rows 0..11
        // carry g only, which comes with the swap gt -> g, and Sigma = rho = 0 in both instances.  The dual step length is the one ipm_ls_end
        // will leave if this point is accepted (alpha stays as it is).
        const double a_du = o.dual_step_cap > 0.0 ? fmin(K.a_du, o.dual_step_cap * alpha) : K.a_du;
        double* __restrict__ w_s = M.s2; double* __restrict__ w_zL = M.zL2; double* __restrict__ w_zU = M.zU2; double* __restrict__ w_y = M.y2;
        double* __restrict__ w_sig = M.sig2; double* __restrict__ w_rho = M.rho2;
        for (int rb = lane + 12; rb < ng; rb += NT * RB) {
          double lbv[RB], ubv[RB], gv[RB], sv[RB], dsv[RB], zlv[RB], zuv[RB], yv[RB], ynv[RB];
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            const int r = rb + j * NT, rr = r < ng ? r : ng - 1;
            lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_gt[rr]; sv[j] = r_s[rr]; dsv[j] = r_ds[rr]; zlv[j] = r_zL[rr]; zuv[j] = r_zU[rr]; yv[j] = r_y[rr]; ynv[j] = r_yn[rr];
          }
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            const int r = rb + j * NT;
            if (r >= ng) continue;
            const double lb = lbv[j], ub = ubv[j], g = gv[j];
            double sg = 0.0, rh = 0.0;
            if (lb == ub) {
              tht += fabs(g - lb);
              const double yn_ = yv[j] + alpha * (ynv[j] - yv[j]); w_y[r] = yn_; nys += fabs(yn_); npr = fmax(npr, fabs(g - lb));
            } else {
              const double so = sv[j], ds = dsv[j];
              double s = so + alpha * ds;
              if (omt > 0.0) { if (lb > -INF) s = fmax(s, fma(omt, so - lb, lb)); if (ub < INF) s = fmin(s, fma(-omt, ub - so, ub)); }
              tht += fabs(g - s);
              bt -= log((lb > -INF ? s - lb : 1.0) * (ub < INF ? ub - s : 1.0));
              double zl = 0.0, zu = 0.0;
              if (lb > -INF) {
                const double dold = so - lb, ro = fast_rcp(dold), zo = zlv[j], dz = fma(-zo * ro, ds, mu * ro - zo), d = s - lb, rd = fast_rcp(d);
                zl = fmin(fmax(zo + a_du * dz, 1e-10 * mu * rd), 1e10 * mu * rd);
                nco = fmax(nco, d * zl); ncm = fmax(ncm, fabs(d * zl - mu)); sg += zl * rd; rh -= mu * rd; nzs += zl; nnz += 1.0;
              }
              if (ub < INF) {
                const double dold = ub - so, ro = fast_rcp(dold), zo = zuv[j], dz = fma(zo * ro, ds, mu * ro - zo), d = ub - s, rd = fast_rcp(d);
                zu = fmin(fmax(zo + a_du * dz, 1e-10 * mu * rd), 1e10 * mu * rd);
                nco = fmax(nco, d * zu); ncm = fmax(ncm, fabs(d * zu - mu)); sg += zu * rd; rh += mu * rd; nzs += zu; nnz += 1.0;
              }
              npr = fmax(npr, fabs(g - s));
              rh += sg * (g - s);
              w_s[r] = s; w_zL[r] = zl; w_zU[r] = zu; w_y[r] = zu - zl; nys += fabs(zu - zl);
            }
            w_sig[r] = sg; w_rho[r] = rh;
          }
        }
        // block_reduce pairs partial sums by thread id, and the accept pass owns rows lane + j NT: its thread t sums the rows this pass gives to
        // thread t - 12 (mod NT; for t < 12 behind the rows 0..11, which add nothing).  Handing the two order-dependent sums of the new point to
        // that thread keeps their association -- and with it every later bit -- what it was (maxima and the row count do not depend on it).
        static_assert(ASM_NSLOT >= 2 * SOLVER_THREADS, "carry takes two partial sums per thread");
        { const int t = lane + 12 < NT ? lane + 12 : lane + 12 - NT; S.carry[2 * t] = nys; S.carry[2 * t + 1] = nzs; }      // (carry is idle outside the backward sweep)
        __syncthreads();
        nys = S.carry[2 * lane]; nzs = S.carry[2 * lane + 1];
      } else
      for (int rb = lane + 12; rb < ng; rb += NT * RB) {
        double lbv[RB], ubv[RB], gv[RB], sv[RB], dsv[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) { const int r = rb + j * NT, rr = r < ng ? r : ng - 1; lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_gt[rr]; sv[j] = r_s[rr]; dsv[j] = r_ds[rr]; }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          if (rb + j * NT >= ng) continue;
          const double lb = lbv[j], ub = ubv[j], g = gv[j];
          if (lb == ub) { tht += fabs(g - lb); continue; }
          double s = sv[j] + alpha * dsv[j];
          if (omt > 0.0) { if (lb > -INF) s = fmax(s, fma(omt, sv[j] - lb, lb)); if (ub < INF) s = fmin(s, fma(-omt, ub - sv[j], ub)); }
          tht += fabs(g - s);
          bt -= log((lb > -INF ? s - lb : 1.0) * (ub < INF ? ub - s : 1.0));
        }
      }
      if (lane < 12 && !feas) { const double d = M.xt[12 * N + lane] - p[12 * N + lane]; ft = p[L.o_QN + lane] * d * d; }
      if (L.run_cost && !feas) ft += rc_f(M.xt);
      if (fused) {
        double v[9] = {tht, bt, ft, npr, nco, ncm, nys, nzs, nnz}; const int op[9] = {RSUM, RSUM, RSUM, RMAX, RMAX, RMAX, RSUM, RSUM, RSUM};
        block_reduce<9>(v, op, S.red);
        KS_BEGIN_SYNCED()
          ipm_ls_test(K, o, v[0], v[2], v[1], S.filt_th, S.filt_ph);
          S.first_trial = 0; S.fast = K.accepted;      // accepted at once: alpha is the one the pass ran with, s_corr = 0
          for (int i = 0; i < 6; ++i) S.nxt[i] = v[3 + i];
          LANDING_EMU_COUNT(m, K.accepted ? (omt > 0.0 ? EMU_ACC_FAST_CLIP : EMU_ACC_FAST) : EMU_ACC_FIRST_REJECTED);
        KS_END();
      } else {
        { double v[3] = {tht, bt, ft}; const int op[3] = {RSUM, RSUM, RSUM}; block_reduce<3>(v, op, S.red); tht = v[0]; bt = v[1]; ft = v[2]; }
        KS_BEGIN_SYNCED() ipm_ls_test(K, o, tht, ft, bt, S.filt_th, S.filt_ph); KS_END();
      }
      if (K.need_corr) {
        // slack correction (landing_nlp.h): the rejected first trial point once more with the inequality slacks moved to g(x_trial)
        double tht2 = 0.0, bt2 = 0.0;
        for (int rb = lane + 12; rb < ng; rb += NT * RB) {
          double lbv[RB], ubv[RB], gv[RB], sv[RB], dsv[RB];
#pragma unroll
          for (int j = 0; j < RB; ++j) { const int r = rb + j * NT, rr = r < ng ? r : ng - 1; lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_gt[rr]; sv[j] = r_s[rr]; dsv[j] = r_ds[rr]; }
#pragma unroll
          for (int j = 0; j < RB; ++j) {
            if (rb + j * NT >= ng) continue;
            const double lb = lbv[j], ub = ubv[j], g = gv[j];
            if (lb == ub) { tht2 += fabs(g - lb); continue; }
            double s = sv[j] + alpha * dsv[j];
            if (omt > 0.0) { if (lb > -INF) s = fmax(s, fma(omt, sv[j] - lb, lb)); if (ub < INF) s = fmin(s, fma(-omt, ub - sv[j], ub)); }
            const double lo = lb > -INF ? lb + o.slack_corr * (s - lb) : -INF, hi = ub < INF ? ub - o.slack_corr * (ub - s) : INF;
            s = fmin(fmax(g, lo), hi);
            tht2 += fabs(g - s);
            bt2 -= log((lb > -INF ? s - lb : 1.0) * (ub < INF ? ub - s : 1.0));
          }
        }
        { double v[2] = {tht2, bt2}; const int op[2] = {RSUM, RSUM}; block_reduce<2>(v, op, S.red); tht2 = v[0]; bt2 = v[1]; }
        KS_BEGIN_SYNCED() ipm_ls_corr_test(K, o, tht2, bt2, S.filt_th, S.filt_ph); KS_END();
      }
    }
    KS_BEGIN()
      ipm_ls_end(K, o, S.filt_th, S.filt_ph, FILT_CAP);
      if (o.jam_clip > 0) S.jamrun = (!S.clip_now && K.a_pr < 0.02) ? S.jamrun + 1 : 0;
      if (S.fast) {      // accept = swap: the fused pass left the new point in the shadow instance
#ifndef __HIPCC__
        for (int r = 0; r < ng; ++r) {      // emulation build: the rule stated at MemberMem holds
          const MemberMem& Q = S.M;
          const bool eq = r >= 12 && S.bnd_lb[bidx(r)] == S.bnd_ub[bidx(r)];
          if ((r < 12 && (Q.y[r] != Q.y2[r] || Q.sig[r] != Q.sig2[r] || Q.rho[r] != Q.rho2[r])) || (eq && (Q.s[r] != Q.s2[r] || Q.zL[r] != Q.zL2[r] || Q.zU[r] != Q.zU2[r]))) {
            fprintf(stderr, "landing_ipm_kernel: member %d row %d differs between the two instances of the row arrays at a swap\n", m, r); abort();
          }
        }
#endif
        mem_accept_swap(S.M);
        K.c_pr = S.nxt[0]; K.c_co = S.nxt[1]; K.c_cm = S.nxt[2]; K.c_ys = S.nxt[3]; K.c_zs = S.nxt[4]; K.c_nz = fmax(S.nxt[5], 1.0);
        K.it++;
      }
    KS_END();
    if (S.fast) { PROF_ADD(PH_LS, K.tp); PROF_ADD(PH_ACCEPT, K.tp); continue; }
    {
    const MemberMem M = live_mem();
    ROW_PTRS(M);
    if (K.fallback) {
      const double alpha = K.alpha;
      for (int i = lane; i < nx; i += NT) M.xt[i] = M.x[i] + alpha * M.dx[i];
      __syncthreads();
      member_eval_g_rare(L, M.xt, p, M.gt);
      __syncthreads();
    }
    PROF_ADD(PH_LS, K.tp);
    // ================================================================ accept the trial point; the same pass produces the
    // primal / complementarity errors, Sigma and rho of the new iterate (what point_pass computes)
    for (int i = lane; i < nx; i += NT) M.x[i] = M.xt[i];
    if (K.feas) {      // elastic rows: primal variables with alpha, multipliers with a_du (kept inside the kappa_Sigma band), then the quantities of the new point
      const double alpha = K.alpha, a_du = K.a_du, mu = K.mu, frho = o.feas_rho;
      for (int r = lane; r < ng; r += NT) {
        const double lb = S.bnd_lb[bidx(r)], ub = S.bnd_ub[bidx(r)];
        r_g[r] = r_gt[r];
        if (r < 12) continue;
        if (lb == ub) { r_y[r] = r_y[r] + alpha * (r_yn[r] - r_y[r]); continue; }
        const double s0 = r_s[r], ds = r_ds[r], s = s0 + alpha * ds;
        double zl = 0.0, zu = 0.0;
        if (lb > -INF) {
          const double n0 = M.en[r], z0 = r_zL[r], w0 = M.wn[r];
          const ElStep e = el_step(1.0, s0 - lb + n0, n0, z0, w0, mu, frho, ds);
          const double n = n0 + alpha * e.dn, a = s - lb + n;
          zl = fmin(fmax(z0 + a_du * e.dz, 1e-10 * mu / a), 1e10 * mu / a);
          M.wn[r] = fmin(fmax(w0 + a_du * e.dw, 1e-10 * mu / n), 1e10 * mu / n); M.en[r] = n;
        }
        if (ub < INF) {
          const double q0 = M.ep[r], z0 = r_zU[r], w0 = M.wp[r];
          const ElStep e = el_step(-1.0, ub + q0 - s0, q0, z0, w0, mu, frho, ds);
          const double q = q0 + alpha * e.dn, b = ub + q - s;
          zu = fmin(fmax(z0 + a_du * e.dz, 1e-10 * mu / b), 1e10 * mu / b);
          M.wp[r] = fmin(fmax(w0 + a_du * e.dw, 1e-10 * mu / q), 1e10 * mu / q); M.ep[r] = q;
        }
        r_s[r] = s; r_zL[r] = zl; r_zU[r] = zu; r_y[r] = zu - zl;
      }
      __syncthreads();
      feas_point_pass(mu);
      KS_BEGIN() K.it++; LANDING_EMU_COUNT(m, EMU_ACC_FEAS); KS_END();
    } else {
      const double alpha = K.alpha, a_du = K.a_du, omt = K.omt, mu = K.mu, s_corr = K.s_corr;
      double npr = 0.0, nco = 0.0, ncm = 0.0, nys = 0.0, nzs = 0.0, nnz = 0.0;
      for (int rb = lane; rb < ng; rb += NT * RB) {
        double lbv[RB], ubv[RB], gv[RB], sv[RB], dsv[RB], zlv[RB], zuv[RB], yv[RB], ynv[RB];
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const int r = rb + j * NT, rr = r < ng ? r : ng - 1;
          lbv[j] = S.bnd_lb[bidx(rr)]; ubv[j] = S.bnd_ub[bidx(rr)]; gv[j] = r_gt[rr]; sv[j] = r_s[rr]; dsv[j] = r_ds[rr]; zlv[j] = r_zL[rr]; zuv[j] = r_zU[rr]; yv[j] = r_y[rr]; ynv[j] = r_yn[rr];
        }
#pragma unroll
        for (int j = 0; j < RB; ++j) {
          const int r = rb + j * NT;
          if (r >= ng) continue;
          const double lb = lbv[j], ub = ubv[j], g = gv[j];
          r_g[r] = g;
          double sg = 0.0, rh = 0.0;
          if (r >= 12) {
            if (lb == ub) { const double yn_ = yv[j] + alpha * (ynv[j] - yv[j]); r_y[r] = yn_; nys += fabs(yn_); npr = fmax(npr, fabs(g - lb)); }
            else {
              const double so = sv[j], ds = dsv[j];
              double s = so + alpha * ds;
              if (omt > 0.0) { if (lb > -INF) s = fmax(s, fma(omt, so - lb, lb)); if (ub < INF) s = fmin(s, fma(-omt, ub - so, ub)); }
              if (s_corr > 0.0) {
                const double lo = lb > -INF ? lb + s_corr * (s - lb) : -INF, hi = ub < INF ? ub - s_corr * (ub - s) : INF;
                s = fmin(fmax(g, lo), hi);
              }
              double zl = 0.0, zu = 0.0;
              if (lb > -INF) {
                const double dold = so - lb, ro = fast_rcp(dold), zo = zlv[j], dz = fma(-zo * ro, ds, mu * ro - zo), d = s - lb, rd = fast_rcp(d);
                zl = fmin(fmax(zo + a_du * dz, 1e-10 * mu * rd), 1e10 * mu * rd);
                nco = fmax(nco, d * zl); ncm = fmax(ncm, fabs(d * zl - mu)); sg += zl * rd; rh -= mu * rd; nzs += zl; nnz += 1.0;
              }
              if (ub < INF) {
                const double dold = ub - so, ro = fast_rcp(dold), zo = zuv[j], dz = fma(zo * ro, ds, mu * ro - zo), d = ub - s, rd = fast_rcp(d);
                zu = fmin(fmax(zo + a_du * dz, 1e-10 * mu * rd), 1e10 * mu * rd);
                nco = fmax(nco, d * zu); ncm = fmax(ncm, fabs(d * zu - mu)); sg += zu * rd; rh += mu * rd; nzs += zu; nnz += 1.0;
              }
              npr = fmax(npr, fabs(g - s));
              rh += sg * (g - s);
              r_s[r] = s; r_zL[r] = zl; r_zU[r] = zu; r_y[r] = zu - zl; nys += fabs(zu - zl);
            }
          }
          r_sig[r] = sg; r_rho[r] = rh;
        }
      }
      double v[6] = {npr, nco, ncm, nys, nzs, nnz}; const int op[6] = {RMAX, RMAX, RMAX, RSUM, RSUM, RSUM};
      block_reduce<6>(v, op, S.red);
      KS_BEGIN_SYNCED()
        K.c_pr = v[0]; K.c_co = v[1]; K.c_cm = v[2]; K.c_ys = v[3]; K.c_zs = v[4]; K.c_nz = fmax(v[5], 1.0);
        K.it++;
        LANDING_EMU_COUNT(m, K.fallback ? EMU_ACC_FALLBACK : (s_corr > 0.0 ? EMU_ACC_CORR : EMU_ACC_BACKTRACK));
      KS_END();
    }
    PROF_ADD(PH_ACCEPT, K.tp);
    }
  }
  __syncthreads();
  if (A.prof && lane == 0) { S.prof[PH_NITER] = (double)K.it; for (int i = 0; i < PH_COUNT; ++i) A.prof[(size_t)m * PH_COUNT + i] = S.prof[i]; }
  if (lane == 0) {      // exit record (EXIT_REC): M still holds the instances as carve() laid them out, S.M the live ones
    double* rec = M.y2 + ng;
    rec[0] = K.mu; rec[1] = K.delta; rec[2] = K.alpha; rec[3] = K.a_du; rec[4] = ((S.M.s == M.s) ? 0.0 : 1.0) + (K.feas ? 2.0 : 0.0); rec[5] = (double)K.it; rec[6] = K.omt; rec[7] = K.s_corr;
  }

  // -------------------------------------------------------------------- outputs
  // multipliers of the initial-state rows from stationarity of X(:,1): lam = -(grad f + J^T y)
  {
  const MemberMem M = live_mem();
  double fo = 0.0;
  if (lane < 12) { M.y[lane] = -M.gx[lane]; const double d = M.x[12 * N + lane] - p[12 * N + lane]; fo = p[L.o_QN + lane] * d * d; }
  if (L.run_cost) fo += rc_f(M.x);
  fo = block_reduce1(fo, RSUM, S.red);
  // reference-consistent KKT residual: max_viol(g), ||grad f + J^T lam||_inf, |lam * dist|
  double kp = 0.0, kc = 0.0;
  for (int r = lane; r < ng; r += NT) {
    const double lb = S.bnd_lb[bidx(r)], ub = S.bnd_ub[bidx(r)], g = M.g[r], lam = M.y[r];
    kp = fmax(kp, fmax(lb - g, fmax(g - ub, 0.0)));
    if (lb != ub) {
      const double dist = lam > 0.0 ? ub - g : g - lb;
      if (lam != 0.0 && dist < INF) kc = fmax(kc, fabs(lam * dist));
    }
  }
  { double v[2] = {kp, kc}; const int op[2] = {RMAX, RMAX}; block_reduce<2>(v, op, S.red); kp = v[0]; kc = v[1]; }
  for (int i = lane; i < nx; i += NT) A.x_out[(size_t)m * nx + i] = M.x[i];
  if (A.lam_out) for (int r = lane; r < ng; r += NT) A.lam_out[(size_t)m * ng + r] = M.y[r];
  if (lane == 0) {
    if (A.f_out) A.f_out[m] = fo;
    if (A.status) A.status[m] = K.status;
    if (A.iters) A.iters[m] = K.it;
    if (A.kkt) { A.kkt[3 * m] = kp; A.kkt[3 * m + 1] = K.e_du; A.kkt[3 * m + 2] = kc; }
  }
  }
#undef ROW_PTRS
#undef KS_BEGIN
#undef KS_BEGIN_SYNCED
#undef KS_END
}

}  // namespace landing
