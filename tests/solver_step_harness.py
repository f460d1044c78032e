"""What the CPU and the GPU tests of the solver kernel's Newton step share (test helper): running landing_ipm_kernel for a given number of
iterations through a library -- the host emulation or the product on the device --, reading dx / ds / yn, the live row arrays and the exit
record from the member's workspace block, and comparing them with tests/newton_reference.py."""
import os

import numpy as np

import newton_reference as nr
from conftest import lc
from emu_support import EMU_LIB, is_emulation, load_runs, pool_map, run_workers, save_runs, worker_main

RUN_COST = dict(QX=[0, 0, 10, 1, 1, 0, .1, .1, .1, .1, .1, .1], Qc=[1.0, 1.0, 0.5], Qf=[1e-4, 1e-4, 1e-3], f_ref=[0, 0, 20.0])
# (bound_push = bound_frac, mu_init); "warm" = landing_solver_opts_warm
OPTION_SETS = [(1e-2, 0.1), (1e-4, 1e-2), (1e-6, 1e-6), (1e-8, 1e-4), "warm"]
LATER_K = (1, 2, 5, 12, 25)


def step_opts(L, oset, max_iter=1, delta_floor=None):
    o = L.warm_opts() if oset == "warm" else L.default_opts()
    if oset != "warm" and oset is not None:
        o.bound_push = o.bound_frac = oset[0]; o.mu_init = oset[1]
    o.max_iter = max_iter; o.feas_phase = 0
    if delta_floor is not None:
        o.delta_floor = delta_floor
    return o


def kernel_run(L, P, X0, opts):
    """one launch: the solver's outputs, the members' workspace blocks and the profile counters [B, 16] (slot 8 = factorisations)"""
    P = np.ascontiguousarray(np.atleast_2d(P), float); X0 = np.ascontiguousarray(np.atleast_2d(X0), float)
    B = P.shape[0]
    if is_emulation(L):
        prof = np.zeros((B, 16))
        L.lib.landing_set_profile_buffer(L.ctx, prof.ctypes.data)
        try:
            res = L.solve_host(P, X0, opts)
        finally:
            L.lib.landing_set_profile_buffer(L.ctx, None)
    else:
        import torch
        dprof = torch.zeros((B, 16), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        L.lib.landing_set_profile_buffer(L.ctx, dprof.data_ptr())
        try:
            res = L.solve_host(P, X0, opts)
        finally:
            L.lib.landing_set_profile_buffer(L.ctx, None)
        torch.cuda.synchronize()
        prof = dprof.cpu().numpy()
    ws = L.debug_workspace(B)
    return dict(res=res, ws=ws, prof=prof, off=L.workspace_offsets())


def member_view(run, b):
    """arrays of member b by name (the LIVE instance of s / zL / zU / y by the record's flag) and its exit record as a dict"""
    w, off = run["ws"][b], run["off"]
    raw = lambda n: w[off[n][0]:off[n][0] + off[n][1]]
    rec = dict(zip(lc("capi").EXIT_RECORD, raw("rec")))
    assert rec["live"] in (0.0, 1.0, 2.0, 3.0)      # live + 2 feas (include/landing_nlp.h, EXIT RECORD)
    rec["feas"] = int(rec["live"]) >> 1; rec["live"] = float(int(rec["live"]) & 1)
    live = "2" if rec["live"] else ""
    v = {n: raw(n) for n in ("dx", "ds", "yn", "en", "ep", "wn", "wp")}
    v.update({n: raw(n + live) for n in ("s", "zL", "zU", "y")})
    v["g"] = raw("gt" if rec["live"] else "g")
    return v, rec


def check_step(O, p, st, v, rec, dreg=None, label=""):
    """the kernel's (dx, ds, yn) against the refined reference at state st with the record's mu and delta: asserts the bound of
    newton_reference (16 x the better of two unrefined fp64 LU solves); returns (ratios, backward error, reference)"""
    N = O.N
    ref = nr.solve_step(O, p, st, rec["mu"], nr.d_reg(N, rec["delta"]) if dreg is None else dreg)
    assert ref["res"] <= 1e-13, (label, "the reference did not refine", ref["res"])
    assert not v["dx"][:12].any(), (label, "dx of the fixed initial state")
    err = nr.errors(ref, v["dx"], v["ds"], v["yn"])
    bound = nr.bounds_of(ref); ratio = nr.ratios(ref, err)
    bwd = nr.backward_error(ref, v["dx"], v["ds"], v["yn"])
    print("%s: err dx %.1e ds %.1e y %.1e | ratio dx %.2g ds %.2g y %.2g (bound %g) | backward error %.1e" % (
        label, err["dx"], err["ds"], err["y"], ratio["dx"], ratio["ds"], ratio["y"], nr.TOL_FACTOR, bwd))
    for k in ("dx", "ds", "y"):
        assert err[k] <= bound[k], (label, k, err[k], bound[k], ref["e_aug"][k], ref["e_cond"][k])
    return ratio, bwd, ref


def first_step_group(L, O, P, X0, opts, label, plain_form):
    """max_iter = 1 from a cold start: every member's step against the reference at initial_state(); the record's mu and delta against
    mu_init and the schedule at the factorisation count.  Returns (worst ratio, factorisation counts, views)."""
    run = kernel_run(L, P, X0, opts)
    B = P.shape[0]
    assert (run["res"]["iters"] == 1).all() and (run["res"]["status"] == 1).all(), (label, run["res"]["iters"], run["res"]["status"])
    floor = opts.delta_floor if plain_form else 0.0
    mu0 = nr.effective_opts(opts, not plain_form)[0]

    def one(b):
        v, rec = member_view(run, b)
        nfact = int(run["prof"][b, 8])
        assert rec["mu"] == mu0, (label, b, rec["mu"], mu0)
        assert rec["it"] == 1 and nfact >= 1
        assert rec["delta"] == nr.delta_schedule(opts, nfact, floor), (label, b, rec["delta"], nfact)
        st = nr.initial_state(O, P[b], X0[b], opts)
        step = rec["alpha"] * v["dx"]
        assert (np.abs(run["res"]["x"][b] - (st["x"] + step)) <= 4 * np.finfo(float).eps * (np.abs(st["x"]) + np.abs(step))).all(), (label, b, "x_1 = x_0 + alpha dx")
        ratio, _, _ = check_step(O, P[b], st, v, rec, label="%s member %d (factorisations %d, delta %.1e)" % (label, b, nfact, rec["delta"]))
        return max(ratio.values())
    worst = max(pool_map(one, range(B)))
    return worst, run["prof"][:, 8].astype(int), run


def later_step_pairs(runs, O, P, label):
    """runs: max_iter -> kernel_run of the SAME inputs.  For every K with K and K + 1 present and every member: the step of iteration K + 1
    (dx, ds, yn and the record of run K + 1) against the reference at the state run K ended in.  An iteration in which run K + 1 took no
    Newton step (a restart: no factorisation) is skipped.  Returns (worst ratio, checked pairs, skipped pairs)."""
    B = P.shape[0]
    jobs = [(K, b) for K in sorted(runs) if K + 1 in runs for b in range(B)]

    def one(job):
        K, b = job
        rk, rn = runs[K], runs[K + 1]
        vk, reck = member_view(rk, b); vn, recn = member_view(rn, b)
        tag = "%s K %d member %d" % (label, K, b)
        if not (rk["res"]["iters"][b] == K and rn["res"]["iters"][b] == K + 1 and reck["it"] == K and recn["it"] == K + 1):
            return tag + ": stopped before the limit", None      # converged earlier: there is no step K + 1
        if rn["prof"][b, 8] - rk["prof"][b, 8] < 1:
            return tag + ": restart (no factorisation in iteration %d)" % (K + 1), None
        lam = rk["res"]["lam_g"][b]
        assert np.array_equal(vk["y"][12:], lam[12:]), (tag, "the record's live-instance flag")
        # the first K iterates of the two runs are the same: x_K = x_{K+1} - alpha dx to rounding
        xk, xn, step = rk["res"]["x"][b], rn["res"]["x"][b], recn["alpha"] * vn["dx"]
        assert (np.abs(xk - (xn - step)) <= 4 * np.finfo(float).eps * (np.abs(xn) + np.abs(step))).all(), (tag, "run K + 1 did not pass through run K's iterate")
        st = dict(x=xk, y=lam, s=vk["s"], zL=vk["zL"], zU=vk["zU"])
        ratio, _, _ = check_step(O, P[b], st, vn, recn, label="%s (mu %.1e delta %.1e alpha %.2e)" % (tag, recn["mu"], recn["delta"], recn["alpha"]))
        return None, max(ratio.values())
    out = pool_map(one, jobs)
    skipped = [s for s, _ in out if s]
    ratios = [r for _, r in out if r is not None]
    return (max(ratios) if ratios else 0.0), len(ratios), skipped


# ---- the host emulation in parallel (emu_support.run_workers): the later-step tests need the same members at nine iteration limits, which are
# independent processes of this file
def emu_runs_parallel(N, seed, B, max_iters, tmp_dir, members=None, delta_floor=None, jobs=None):
    """kernel_run() of members `members` (default: all) of make_batch(B, N, 0.6, seed) through the emulation at every iteration limit of
    max_iters (default options but no feasibility phase; delta_floor if given), one process per (limit, member).
    Returns (P, X0, {max_iter: run}) with the chosen members only, in the order given."""
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=seed)
    members = list(range(B)) if members is None else list(members)
    todo = [dict(N=N, seed=seed, B=B, member=b, max_iter=K, delta_floor=delta_floor, out=os.path.join(str(tmp_dir), "emu_N%d_s%d_K%d_m%d.npz" % (N, seed, K, b)))
            for K in sorted(max_iters, reverse=True) for b in members]      # longest first
    runs = load_runs(run_workers(__file__, todo, jobs), ("ws", "prof"))
    off = lc("capi").workspace_offsets(N)
    return P[members], X0[members], {K: dict(runs[K], off=off) for K in max_iters}


def _emu_worker(spec):
    P, X0, _, _ = lc("problem").make_batch(spec["B"], spec["N"], 0.6, seed=spec["seed"])
    b = spec["member"]
    L = lc("capi").LandingLib(spec["N"], lib_path=EMU_LIB)
    save_runs(spec["out"], {spec["max_iter"]: kernel_run(L, P[b:b + 1], X0[b:b + 1], step_opts(L, None, max_iter=spec["max_iter"], delta_floor=spec["delta_floor"]))}, ("ws", "prof"))
    L.close()


if __name__ == "__main__":
    worker_main(_emu_worker)
