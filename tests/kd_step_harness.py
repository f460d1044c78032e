"""What the CPU and the GPU tests of the kinodynamic refinement solver's Newton step share (test helper): running landing_kinodyn_solve_batch for a given
number of iterations through a library -- the host emulation or the product on the device --, reading dx / ds / yn, the row arrays, gc and the iteration
scalars from the member's workspace block (landing_debug_kd_*), and comparing them with tests/kd_newton_reference.py."""
import os

import numpy as np

import kd_newton_reference as kr
import newton_reference as nr
from conftest import lc
from emu_support import EMU_LIB, is_emulation, load_runs, pool_map, run_workers, save_runs, worker_main      # (pool_map: for the tests that take it from here)
from solver_step_harness import OPTION_SETS      # (the option sets of the SRBM step check; "warm" = landing_kinodyn_solver_opts_warm here)

ULP4 = 4 * kr.EPS
GC_TOL = 8 * kr.EPS      # per entry of gc, times the sum of |terms|.  An entry is a sum of n products in a fixed order; with two roundings per product (one for J_I' rho) it errs
                         # by at most (n + 1) 2^-53 of that sum, so entries of up to 15 terms are held to (n + 2) 2^-53 (gc_bound; the extra unit covers the second-order
                         # terms and the np.longdouble restatement) -- a derived bound.  The longest sums (diagonal entries of forces and joint angles: 52 products) are held to
                         # the flat 8 eps, which for them is below the worst case (26.5 eps) and holds by measurement only: worst 2.7 eps on the emulation, 4.7 eps on the MI355X


def gc_bound(n_terms):
    """per entry: min(8 eps, (n + 2) 2^-53), as a multiple of the sum of |terms|"""
    return np.minimum(GC_TOL, (np.asarray(n_terms) + 2) * (kr.EPS / 2)).astype(kr.LD)


# LATER steps of the short horizons (N < 20) from production drop states, on the device and on the emulation alike: the stage recursion's forward error exceeds 16 x the
# sparse LU's although its normwise backward error stays <= 1e-13 and every intermediate is inside its bound -- the unstructured LU solves these 300 .. 400-unknown systems to a
# backward error of ~1e-19, the recursion to its usual ~10 eps.  Worst ratio measured: N = 2: 2.5e3 (MI355X, K = 12; emulation 360), N = 3: 150 (emulation 170); per horizon the
# factor is the next power of two above twice that, with the backward error <= 1e-12 asserted alongside.  Every other case keeps 16.
SHORT_LATER_FACTOR = {2: 8192.0, 3: 512.0}
WORST_GC = [0.0, 0]      # worst measured |error| / (eps * sum |terms|) of an entry of gc and the most terms of one, for the docstrings


def consts():
    mass, Ib, Ibi = lc("constants").robot_constants()
    return mass, np.asarray(Ib), np.asarray(Ibi)


def problem_of(N, q, qd, x_guess, dt, mu_fric):
    """(Problem, x0) of a drop state as the production callers pose it (kinodyn.member_problem) from an SRBM trajectory x_guess [36 N + 12]"""
    lb, ub, cost, x0 = lc("kinodyn").member_problem(N, q, qd, x_guess)
    return kr.Problem(N, lb, ub, cost, dt, *consts(), mu_fric), x0


def step_opts(R, oset, max_iter, delta_floor=None):
    """portfolio off, no feasibility phase; oset: (bound_push = bound_frac, mu_init), "warm" or None (the defaults)"""
    o = R.kinodyn_warm_opts() if oset == "warm" else R.kinodyn_default_opts()
    if oset != "warm" and oset is not None:
        o.bound_push = o.bound_frac = oset[0]; o.mu_init = oset[1]
    o.max_iter = max_iter; o.feas_phase = 0; o.kd_clone_after = 0; o.kd_clone_max = 0
    if delta_floor is not None:
        o.delta_floor = delta_floor
    return o


def function_layer(R, pr, X, Y):
    """the product's Jacobian blocks [B, N, 141, 72] and Hessian blocks of Y' g [B, N, 72, 72] at the points X [B, nx]"""
    import torch
    dev = "cpu" if is_emulation(R) else "cuda"
    X = np.ascontiguousarray(np.atleast_2d(X), float); Y = np.ascontiguousarray(np.atleast_2d(Y), float)
    B, N = X.shape[0], pr.N
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev)
    dx, dl = t(X), t(Y)
    J = torch.zeros(B, N, 141, 72, dtype=torch.float64, device=dev); H = torch.zeros(B, N, 72, 72, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev == "cuda" else 0
    R.kinodyn_nlp_eval(B, N, dx.data_ptr(), *pr.model(), 0, J.data_ptr(), st)
    R.kinodyn_nlp_hess(B, N, dx.data_ptr(), *pr.model(), dl.data_ptr(), H.data_ptr(), st)
    if dev == "cuda":
        torch.cuda.synchronize()
    return J.cpu().numpy(), H.cpu().numpy()


def kd_run(R, probs, X0, opts):
    """one solve of the members probs (same horizon and model): outputs, the members' workspace blocks, their iteration scalars, and the function layer's
    J / H blocks at the returned (x, lam_g)"""
    pr = probs[0]; N = pr.N
    lb, ub, cost = (np.array([getattr(p, n) for p in probs]) for n in ("lb", "ub", "cost"))
    res = R.kinodyn_solve_host(N, lb, ub, cost, np.atleast_2d(X0), *pr.model(), opts)
    B = len(probs)
    ws, n_ws = R.kinodyn_debug_workspace(B)
    assert n_ws == N
    rec = [R.kinodyn_debug_state(b) for b in range(B)]
    Jb, Hb = function_layer(R, pr, res["x"], res["lam_g"])
    return dict(res=res, ws=ws, rec=rec, off=R.kinodyn_workspace_layout(N), Jb=Jb, Hb=Hb)


def member_view(run, b):
    """arrays of member b by name and its iteration scalars"""
    w, off = run["ws"][b], run["off"]
    v = {n: w[o[0]:o[0] + o[1]] for n, o in off.items() if isinstance(o, tuple)}
    return v, run["rec"][b]


def check_step(pr, st, v, rec, J, H, dreg=None, label="", factor=nr.TOL_FACTOR):
    """the kernel's (dx, ds, yn on the defect rows) against the refined reference at state st with the record's mu and delta: asserts the bound of
    newton_reference (factor = 16 x the better of two unrefined fp64 LU solves; SHORT_LATER_FACTOR[N] where the GPU tests say so); returns (ratios, backward error, reference)"""
    N = pr.N
    ref = kr.solve_step(pr, st, rec["mu"], kr.d_reg(N, rec["delta"]) if dreg is None else dreg, J, H)
    assert ref["res"] <= 1e-13, (label, "the reference did not refine", ref["res"])
    err = nr.errors(ref, v["dx"], v["ds"], v["yn"])
    ratio = nr.ratios(ref, err)
    bound = {k: b * (factor / nr.TOL_FACTOR) for k, b in nr.bounds_of(ref).items()}
    bwd = nr.backward_error(ref, v["dx"], v["ds"], v["yn"])
    print("%s: err dx %.1e ds %.1e y %.1e | ratio dx %.2g ds %.2g y %.2g (bound %g) | backward error %.1e" % (
        label, err["dx"], err["ds"], err["y"], ratio["dx"], ratio["ds"], ratio["y"], factor, bwd))
    for k in ("dx", "ds", "y"):
        assert err[k] <= bound[k], (label, k, err[k], bound[k], ref["e_aug"][k], ref["e_cond"][k])
    if factor != nr.TOL_FACTOR:
        assert bwd <= 1e-12, (label, "backward error", bwd)      # (what licenses the wider factor: the excess is forward-error amplification, not a wrong matrix)
    return ratio, bwd, ref


def check_sig_rho(pr, v, rec, label):
    """Sigma / rho the run left in the workspace (of its last iterate, at the record's mu) against the formula: <= 4 ulp of the term sums"""
    sig, rho, tsig, trho = kr.sig_rho_reference(pr, v["g"], v["s"], v["zL"], v["zU"], rec["mu"])
    es = np.abs(v["sig"].astype(kr.LD) - sig); er = np.abs(v["rho"].astype(kr.LD) - rho)
    assert (es <= ULP4 * tsig).all(), (label, "sig", int(np.argmax(es - ULP4 * tsig)))
    assert (er <= ULP4 * trho).all(), (label, "rho", int(np.argmax(er - ULP4 * trho)))
    assert not v["sig"][:24].any() and not v["rho"][:24].any()


def check_gc(pr, vk, reck, vn, recn, Jk, label):
    """gc of the step run n took from the iterate run k ended in: every interval's J_I' Sigma J_I and J_I' rho against the np.longdouble restatement over the
    function layer's Jacobian Jk [ng, nx] at x_k, Sigma as run k left it (it does not depend on mu), rho as run k left it when the step used the same mu -- else the
    formula at the step's mu, with 4 ulp of its term sums as the error of the kernel's own rho.  Entries the kernel never writes: exactly 0 on both sides."""
    N = pr.N
    same_mu = recn["mu"] == reck["mu"]
    if same_mu:
        rho, rerr = vk["rho"], None
    else:
        _, rho, _, trho = kr.sig_rho_reference(pr, vk["g"], vk["s"], vk["zL"], vk["zU"], recn["mu"])
        rerr = ULP4 * trho
    G, m, A, Am, most, Em, nG, nm = kr.gc_reference(N, Jk, vk["sig"], rho, rerr)
    bG, bm = gc_bound(nG) * A, gc_bound(nm) * Am + Em
    gc = vn["gc"].reshape(N, kr.GC)
    Gk = gc[:, :kr.NV * kr.NV].reshape(N, kr.NV, kr.NV); mk = gc[:, kr.NV * kr.NV:]
    eG = np.abs(Gk.astype(kr.LD) - G); em = np.abs(mk.astype(kr.LD) - m)
    assert (eG <= bG).all(), (label, "J_I' Sigma J_I", np.unravel_index(int(np.argmax(eG - bG)), eG.shape), float(eG.max()))
    assert (em <= bm).all(), (label, "J_I' rho", np.unravel_index(int(np.argmax(em - bm)), em.shape), float(em.max()))
    assert (Gk[A == 0] == 0.0).all() and (mk[Am == 0] == 0.0).all(), (label, "an entry no row couples")
    assert (A[:, :24, :24] > 0).any() and (A == 0).any()
    with np.errstate(divide="ignore", invalid="ignore"):
        w = max(float(np.nanmax(np.where(A > 0, eG / (kr.EPS * A), 0.0))), float(np.nanmax(np.where(Am > 0, (em - Em) / (kr.EPS * Am), 0.0))))
    WORST_GC[0] = max(WORST_GC[0], w); WORST_GC[1] = max(WORST_GC[1], most)
    print("%s: gc worst error %.2f eps of the term sums (bound 8), most terms %d, rho %s" % (label, w, most, "of the workspace" if same_mu else "restated at the step's mu"))
    return most


def state_of(run, b):
    v, rec = member_view(run, b)
    return dict(x=run["res"]["x"][b], y=run["res"]["lam_g"][b], s=v["s"], zL=v["zL"], zU=v["zU"])


def check_pair(pr, x0, runs, K, b, label, jac="product", jac_check=False, opts=None, hess_check=False, factor=nr.TOL_FACTOR):
    """The step of iteration K + 1 (run K + 1: dx, ds, yn, gc, the record's mu and delta) against the reference at the iterate run K ended in, with the intermediate
    quantities.  K = 0: run 0 is the start (max_iter = 0), and the state is ALSO restated from the inputs (kd_newton_reference.initial_state) and compared.
    jac = "oracle": J of the reference from the oracle's complex step (and the product's blocks held against it to 1e-11); "product": the function layer's blocks,
    held against the complex step when jac_check.  Returns (None, worst ratio, backward error) or (reason, None, None) for a skipped pair."""
    rk, rn = runs[K], runs[K + 1]
    vk, reck = member_view(rk, b); vn, recn = member_view(rn, b)
    N = pr.N
    if not (rk["res"]["iters"][b] == K and rn["res"]["iters"][b] == K + 1 and reck["it"] == K and recn["it"] == K + 1):
        return label + ": stopped before the limit (status %d after %d iterations)" % (rn["res"]["status"][b], rn["res"]["iters"][b]), None, None
    if (reck["nreset"], reck["last_reset_it"]) != (recn["nreset"], recn["last_reset_it"]):
        return label + ": restart between the two runs", None, None
    assert recn["feas"] == 0 and recn["pending"] == 0 and recn["nfact"] > reck["nfact"], (label, recn)
    # run K + 1 passed through run K's iterate: x_K = x_{K+1} - alpha dx to rounding
    xk, xn, step = rk["res"]["x"][b], rn["res"]["x"][b], recn["alpha"] * vn["dx"]
    assert (np.abs(xk - (xn - step)) <= 4 * kr.EPS * (np.abs(xn) + np.abs(step))).all(), (label, "x_{K+1} = x_K + alpha dx")
    assert np.array_equal(vk["x"], xk) and np.array_equal(vk["y"][24:], rk["res"]["lam_g"][b][24:])
    st = state_of(rk, b)
    if K == 0:      # the start, restated from the inputs
        s0 = kr.initial_state(pr, x0, opts)
        assert np.array_equal(s0["x"], st["x"]) and np.array_equal(s0["zL"], st["zL"]) and np.array_equal(s0["zU"], st["zU"]), (label, "initial point")
        assert (np.abs(s0["s"] - st["s"]) <= 1e-13 * np.maximum(1.0, np.abs(st["s"]))).all(), (label, "initial slacks")
        assert reck["mu"] == opts.mu_init
        st = dict(s0, y=st["y"])
    Jp = kr.jacobian_from_blocks(N, rk["Jb"][b])
    if jac == "oracle" or jac_check:
        Jo = kr.jacobian_complex_step(pr, st["x"]) if jac == "oracle" else kr.jacobian_from_blocks(N, kr.jacobian_complex_step_blocks(pr, st["x"]))
        ej = abs(Jp - Jo).max() / max(1.0, abs(Jo).max())
        print("%s: product Jacobian against the complex step %.1e" % (label, ej))
        assert ej <= 1e-11, (label, "Jacobian", ej)
    J = Jo if jac == "oracle" else Jp
    H = kr.hessian_from_blocks(N, rk["Hb"][b])
    if hess_check:
        print("%s: product Hessian against central differences of the oracle's gradient %.1e" % (label, kr.hessian_check(pr, st["x"], st["y"], H)))
    check_sig_rho(pr, vn, recn, label)
    most = check_gc(pr, vk, reck, vn, recn, Jp, label)
    nf = int(recn["nfact"] - reck["nfact"])
    ratio, bwd, _ = check_step(pr, st, vn, recn, J, H, factor=factor, label="%s (mu %.1e delta %.1e alpha %.2e, %d factorisations, gc terms <= %d)" % (label, recn["mu"], recn["delta"], recn["alpha"], nf, most))
    return None, max(ratio.values()), bwd


# ---- the host emulation in parallel: it keeps the kernels' LDS in static storage, so one process runs one launch at a time; every (member, option set) is a
# process of this file that runs its iteration limits one after the other
def emu_member(spec):
    """(Problem, x0) of member `m` at horizon N: the gentle drop of tests/test_kd_solver_cpu.py (dt = 50 ms), varied by a seeded perturbation for m > 0"""
    kd, P = lc("kinodyn"), lc("problem")
    N, m = spec["N"], spec["member"]
    dtv = np.full(N, 0.05)
    rng = np.random.default_rng(1000 + m)
    q = np.array([0, 0, 0.0, 0.05, 0.15, -0.05]); qd = np.array([0.1, -0.1, 0.05, 0.2, -0.1, -1.0])
    if m > 0:
        q[3:6] += 0.05 * rng.normal(size=3); qd += 0.1 * rng.normal(size=6)
    q[2] = 0.35 + abs(min((kd.rot_xyz(q[3:6]) @ np.array([sx * 0.19, sy * 0.1, 0.0]))[2] for sx in (1, -1) for sy in (1, -1))) + abs(dtv[0] * qd[5])
    consts = P.production_constants("main")
    _, x0s, _, _ = P.make_member(N, 0.05 * N, q, qd, consts, dtv)
    return problem_of(N, q, qd, x0s, dtv, 0.75)


FIELDS = ("ws", "rec", "Jb", "Hb")


def save_kd_runs(path, R, runs):
    """emu_support.save_runs of kd_run()s, the members' iteration scalars as rows of an array"""
    save_runs(path, {t: dict(run, rec=np.array([[r[n] for n in R.KD_STATE] for r in run["rec"]])) for t, run in runs.items()}, FIELDS)


def load_kd_runs(paths, R, N):
    """the inverse, over the members' files: {tag: run} as kd_run() returns them"""
    off = R.kinodyn_workspace_layout(N)
    return {t: dict(run, rec=[dict(zip(R.KD_STATE, r)) for r in run["rec"]], off=off) for t, run in load_runs(paths, FIELDS).items()}


def emu_runs_parallel(specs, tmp_dir, jobs=None):
    """specs: list of dict(N, member, oset, delta_floor, max_iters).  Returns per spec (Problem, x0, opts of the longest run, {max_iter: run})"""
    todo = [dict(spec, out=os.path.join(str(tmp_dir), "kd_emu_%d.npz" % i)) for i, spec in enumerate(specs)]
    run_workers(__file__, sorted(todo, key=lambda s: -sum(s["max_iters"]) * s["N"]), jobs)      # longest first
    L = lc("capi").LandingLib(20, lib_path=EMU_LIB); R = lc("rbd").Rbd(L)
    out = []
    for spec in todo:
        pr, x0 = emu_member(spec)
        oset = spec["oset"]
        out.append((pr, x0, step_opts(R, tuple(oset) if isinstance(oset, list) else oset, max(spec["max_iters"]), spec["delta_floor"]), load_kd_runs([spec["out"]], R, spec["N"])))
    L.close()
    return out


def _emu_worker(spec):
    pr, x0 = emu_member(spec)
    L = lc("capi").LandingLib(spec["N"], lib_path=EMU_LIB); R = lc("rbd").Rbd(L)
    oset = spec["oset"]; oset = tuple(oset) if isinstance(oset, list) else oset
    save_kd_runs(spec["out"], R, {K: kd_run(R, [pr], x0[None], step_opts(R, oset, K, spec["delta_floor"])) for K in spec["max_iters"]})
    L.close()


if __name__ == "__main__":
    worker_main(_emu_worker)
