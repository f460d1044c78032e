"""What the CPU and the GPU tests of the SRBM solver's feasibility-phase step share (test helper): running landing_ipm_kernel with max_iter = M, feas_phase = 1,
feas_jam = 0 under landing_debug_iter_cap = M + 1 + j through a library -- the host emulation or the product on the device --, so that the member enters the
phase at x_M and stops after exactly j steps of it; reading the row state (s, en, ep, zL, wn, zU, wp), the step (dx, ds, yn) and the exit record from the member's
workspace block; and comparing them with tests/elastic_newton_reference.py.  Run T gives the state, run T + 1 from the same inputs the step.

Tolerances: the step is held to newton_reference's bound (16 x the better of two unrefined fp64 LU solves, per quantity).  The update and the step lengths are held to
that bound PROPAGATED: a direction the kernel eliminates (dn, dzL, dwn, ...) depends linearly on ds, with the slope k the reference reads off the row's own 3 x 3 block,
so its bound is |k| x (bound of ds), and an updated value v + step * d is held to step * |k| * bound_ds + 4 eps (|v| + |step * d|).
"""
import os

import numpy as np

import elastic_newton_reference as er
import newton_reference as nr
import solver_step_harness as H
from conftest import lc
from emu_support import EMU_LIB, load_runs, pool_map, run_workers, save_runs, worker_main

EPS = np.finfo(float).eps
PAIR_J = (0, 1, 2, 5, 12, 25)      # pairs (j, j + 1): 0 = the first step of the phase, from the entry state
NAMED = [(100000, m) for m in (40, 120, 131, 154, 252, 592)] + [(3, m) for m in (7, 63, 76, 95, 187, 189)]      # tests/test_gpu_certificates.py: locally infeasible ...
CONVERGING = [(100000, m) for m in (0, 1, 2, 3)]                                                                   # ... and four the solver solves


def pairs_within(M, js=PAIR_J):
    """the pairs (j, j + 1) a run with max_iter = M can hold: the phase entered after M iterations runs to iteration 2 M at most (ipm_core.hpp ipm_enter_phase:
    lim = it + max_iter), and the entry counts as iteration M + 1, so step j + 1 exists iff M + 2 + j <= 2 M"""
    return [j for j in js if M + 2 + j <= 2 * M]


def caps_of(M, js):
    """the iteration caps of the runs the pairs js need, plus M itself (the run that ends at x_M without entering the phase) and M + 1 (the entry state)"""
    return sorted({M, M + 1} | {M + 1 + j for j in js} | {M + 2 + j for j in js})


def named_batch(N=20):
    Pm = lc("problem")
    batches = {seed: Pm.make_batch(1024, N, 0.6, seed=seed, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")[:2] for seed in (100000, 3)}
    P = np.array([batches[s][0][m] for s, m in NAMED + CONVERGING]); X0 = np.array([batches[s][1][m] for s, m in NAMED + CONVERGING])
    return P, X0


def feas_opts(L, M, rho=None):
    o = L.default_opts()
    o.max_iter = M; o.feas_phase = 1; o.feas_jam = 0
    if rho is not None:
        o.feas_rho = rho
    return o


def capped_run(L, P, X0, opts, cap):
    """H.kernel_run under landing_debug_iter_cap = cap (restored to 0 afterwards)"""
    L._check(L.lib.landing_debug_iter_cap(L.ctx, int(cap)), "landing_debug_iter_cap")
    try:
        return H.kernel_run(L, P, X0, opts)
    finally:
        L._check(L.lib.landing_debug_iter_cap(L.ctx, 0), "landing_debug_iter_cap")


def row_state(v):
    return {k: v[k] for k in ("s", "en", "ep", "zL", "wn", "zU", "wp")}


def check_entry(O, p, opts, M, run_M, run_0, b, label):
    """j = 0 (cap M + 1) against the run that stopped at x_M (cap M): the phase is entered at x_M; the kernel's g there matches the oracle's to 1e-12; the entry state is
    el_init_row of that g -- s, en, ep bit for bit, the multipliers to 4 eps.  Returns a reason when the member has no entry to check (it converged within M iterations)."""
    vM, recM = H.member_view(run_M, b); v, rec = H.member_view(run_0, b)
    if run_M["res"]["status"][b] == 0 or run_0["res"]["iters"][b] != M + 1 or not rec["feas"]:
        return "%s: no entry (status %d after %d iterations at cap M, %d iterations at cap M + 1, feas %d)" % (
            label, run_M["res"]["status"][b], run_M["res"]["iters"][b], run_0["res"]["iters"][b], rec["feas"])
    assert recM["feas"] == 0 and run_M["res"]["iters"][b] == M and rec["it"] == M + 1, (label, recM, rec)
    x = run_0["res"]["x"][b]
    assert np.array_equal(x, run_M["res"]["x"][b]), (label, "the phase is not entered at x_M")
    mu0 = nr.effective_opts(opts, O.form.run_cost != 0)[0]
    assert rec["mu"] == mu0, (label, rec["mu"], mu0)
    lb, ub = O.bounds(p)
    go = O.g(x, p)
    eg = np.abs(v["g"][12:] - go[12:]) / np.maximum(1.0, np.abs(go[12:]))
    assert eg.max() <= 1e-12, (label, "g at the entry", float(eg.max()))
    e0 = er.init_rows(v["g"], lb, ub, mu0, opts.feas_rho, 12)
    for k in ("s", "en", "ep"):
        assert np.array_equal(v[k][12:], e0[k][12:]), (label, k, int(np.argmax(v[k][12:] != e0[k][12:])) + 12)
    worst = 0.0
    for k in ("zL", "zU", "wn", "wp"):
        d = np.abs(v[k][12:] - e0[k][12:]); ok = d <= 4 * EPS * np.abs(e0[k][12:])
        assert ok.all(), (label, k, int(np.argmin(ok)) + 12)
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(e0[k][12:] != 0, d / (EPS * np.abs(e0[k][12:])), 0.0))))
    eq = (lb == ub) & (np.arange(O.ng) >= 12)
    assert not v["y"][eq].any() and np.array_equal(v["y"][12:][~eq[12:]], (v["zU"] - v["zL"])[12:][~eq[12:]]), (label, "y at the entry")
    print("%s: entry state restated; g against the oracle %.1e, multipliers within %.2f eps" % (label, float(eg.max()), worst))
    return None


def _ftb(m, tau):
    return tau / m if m > tau else 1.0


def check_update(ref, opts, vk, vn, recn, xk, xn, lb, ub, label, factor=nr.TOL_FACTOR):
    """state of run T + 1 = state of run T advanced by the REFERENCE's directions with the record's step lengths; the dual step length follows
    fraction-to-the-boundary over z, w with the reference's directions; alpha <= the primal fraction-to-the-boundary value.  Bounds: module docstring."""
    alpha, a_du, mu = recn["alpha"], recn["a_du"], recn["mu"]
    bnd = {k: v * (factor / nr.TOL_FACTOR) for k, v in nr.bounds_of(ref).items()}      # (the step's bound, with the caller's factor where one is licensed)
    B = {"dx": bnd["dx"] * nr._scale(ref["dx"]), "ds": bnd["ds"] * nr._scale(ref["ds"][ref["ineq"]]), "y": bnd["y"] * nr._scale(ref["y_new"][ref["eq"]])}

    def held(name, got, old, d, step, slope_bound, rows):
        want = old + step * d
        tol = step * slope_bound + 4 * EPS * (np.abs(old) + np.abs(step * d))
        bad = ~(np.abs(got - want) <= tol)
        assert not bad.any(), (label, name, int(np.asarray(rows)[np.argmax(bad)]), float(np.abs(got - want)[np.argmax(bad)]), float(np.asarray(tol)[np.argmax(bad)]))

    held("x", xn, xk, ref["dx"], alpha, B["dx"], np.arange(len(xk)))
    I = np.nonzero(ref["ineq"])[0]
    held("s", vn["s"][I], vk["s"][I], ref["ds"][I], alpha, B["ds"], I)
    E = np.nonzero(ref["eq"])[0]
    held("y", vn["y"][E], vk["y"][E], ref["y_new"][E] - vk["y"][E], alpha, B["y"], E)
    tau = max(opts.tau_min, 1.0 - mu)
    m_pr = [0.0, 0.0]; m_du = [0.0, 0.0]      # [low, high] ends of the largest ratio
    for side, var, z, w, bound in (("L", "en", "zL", "wn", lb), ("U", "ep", "zU", "wp", ub)):
        S = ref[side]; R = S["rows"]
        kv, kz, kw = (np.abs(S["k"][:, i]) * B["ds"] for i in range(3))
        held(var, vn[var][R], vk[var][R], S["dv"], alpha, kv, R)
        dist = (vn["s"][R] - bound[R] + vn[var][R]) if side == "L" else (bound[R] + vn[var][R] - vn["s"][R])      # of the kernel's own new point (held above)
        assert (dist > 0).all() and (vn[var][R] > 0).all(), (label, side, "a distance left the interior")
        for nm, d, old, kk, dd in ((z, S["dz"], vk[z][R], kz, dist), (w, S["dw"], vk[w][R], kw, vn[var][R])):
            lo, hi = 1e-10 * mu / dd, 1e10 * mu / dd
            want = np.minimum(np.maximum(old + a_du * d, lo), hi)
            tol = a_du * kk + 4 * EPS * (np.abs(old) + np.abs(a_du * d)) + 4 * EPS * np.abs(want)
            bad = ~(np.abs(vn[nm][R] - want) <= tol)
            assert not bad.any(), (label, nm, int(R[np.argmax(bad)]), float(np.abs(vn[nm][R] - want)[np.argmax(bad)]), float(tol[np.argmax(bad)]))
            r = -d / old; e = (kk + 4 * EPS * np.abs(d)) / old
            m_du[0] = max(m_du[0], float((r - e).max())); m_du[1] = max(m_du[1], float((r + e).max()))
        da = S["sd"] * ref["ds"][R] + S["dv"]; ka = np.abs(S["sd"] + S["k"][:, 0]) * B["ds"]
        for d, old, kk in ((da, S["dist"], ka), (S["dv"], S["v"], kv)):
            r = -d / old; e = (kk + 4 * EPS * np.abs(d)) / old
            m_pr[0] = max(m_pr[0], float((r - e).max())); m_pr[1] = max(m_pr[1], float((r + e).max()))
    cap = (lambda a: min(a, opts.dual_step_cap * alpha)) if opts.dual_step_cap > 0.0 else (lambda a: a)
    lo, hi = cap(_ftb(m_du[1], tau)), cap(_ftb(m_du[0], tau))
    assert lo * (1 - 8 * EPS) <= a_du <= hi * (1 + 8 * EPS), (label, "a_du", a_du, lo, hi)
    assert alpha <= _ftb(m_pr[0], tau) * (1 + 8 * EPS), (label, "alpha beyond the fraction to the boundary", alpha, _ftb(m_pr[0], tau))
    assert np.array_equal(vn["y"][I], (vn["zU"] - vn["zL"])[I]), (label, "y = zU - zL")      # inequality rows at the new point


def check_pair(O, p, opts, runs, T, b, label):
    """the step of run T + 1 against the reference at the state run T ended in, then the update.  Returns (reason, None) for a skipped pair, else (None, ratios)."""
    rk, rn = runs[T], runs[T + 1]
    vk, reck = H.member_view(rk, b); vn, recn = H.member_view(rn, b)
    if not (rk["res"]["iters"][b] == T and rn["res"]["iters"][b] == T + 1 and reck["it"] == T and recn["it"] == T + 1):
        # (a member handed back by the phase AT the cap counts the hand-over as one more iteration and stops: iters = cap + 1, no step taken)
        return "%s: did not stop at the caps %d, %d (status %d after %d iterations)" % (label, T, T + 1, rn["res"]["status"][b], rn["res"]["iters"][b]), None
    if not (reck["feas"] and recn["feas"]):
        return "%s: outside the phase (feas %d, %d)" % (label, reck["feas"], recn["feas"]), None
    assert rn["prof"][b, 8] - rk["prof"][b, 8] >= 1, (label, "no factorisation")
    xk, xn = rk["res"]["x"][b], rn["res"]["x"][b]
    y = np.array(vk["y"]); y[:12] = 0.0
    ref = er.solve_step(O, p, dict(x=xk, y=y), row_state(vk), recn["mu"], opts.feas_rho, nr.d_reg(O.N, recn["delta"]))
    assert ref["res"] <= 1e-13, (label, "the reference did not refine", ref["res"])
    assert not vn["dx"][:12].any(), (label, "dx of the fixed initial state")
    err = nr.errors(ref, vn["dx"], vn["ds"], vn["yn"])
    bound = nr.bounds_of(ref); ratio = nr.ratios(ref, err)
    bwd = nr.backward_error(ref, vn["dx"], vn["ds"], vn["yn"])
    print("%s (mu %.1e delta %.1e alpha %.2e a_du %.2e): err dx %.1e ds %.1e y %.1e | ratio dx %.2g ds %.2g y %.2g (bound %g) | backward error %.1e" % (
        label, recn["mu"], recn["delta"], recn["alpha"], recn["a_du"], err["dx"], err["ds"], err["y"], ratio["dx"], ratio["ds"], ratio["y"], nr.TOL_FACTOR, bwd))
    for k in ("dx", "ds", "y"):
        assert err[k] <= bound[k], (label, k, err[k], bound[k], ref["e_aug"][k], ref["e_cond"][k])
    lb, ub = O.bounds(p)
    check_update(ref, opts, vk, vn, recn, xk, xn, lb, ub, label)
    return None, ratio


def check_config(O, P, opts, M, js, runs, label, entry=True):
    """every member's entry (cap M + 1 against cap M) and every pair (j, j + 1) of js.  Returns dict(worst: per quantity, checked, skipped: list of reasons,
    by_j: {j: members that contributed a checked pair})"""
    Bn = P.shape[0]
    jobs = [("entry", b) for b in range(Bn)] if entry else []
    jobs += [(j, b) for j in js for b in range(Bn)]

    def one(job):
        j, b = job
        if j == "entry":
            return job, check_entry(O, P[b], opts, M, runs[M], runs[M + 1], b, "%s member %d entry" % (label, b)), None
        reason, ratio = check_pair(O, P[b], opts, runs, M + 1 + j, b, "%s member %d j %d" % (label, b, j))
        return job, reason, ratio
    out = pool_map(one, jobs)
    worst = {"dx": 0.0, "ds": 0.0, "y": 0.0}; by_j = {j: [] for j in js}; skipped = []; no_entry = []; checked = 0
    for (j, b), reason, ratio in out:
        if j == "entry":
            if reason:
                no_entry.append(reason)
            continue
        if reason:
            skipped.append(reason); continue
        checked += 1; by_j[j].append(b)
        for k in worst:
            worst[k] = max(worst[k], ratio[k])
    for s in no_entry + skipped:
        print("  skipped:", s)
    print("%s: %d pairs checked, %d skipped, %d members without an entry; WORST RATIO dx %.3g ds %.3g y %.3g" % (label, checked, len(skipped), len(no_entry), worst["dx"], worst["ds"], worst["y"]))
    return dict(worst=worst, checked=checked, skipped=skipped, no_entry=no_entry, by_j=by_j)


# ---- the host emulation in parallel: one process per member, which runs the member alone at every cap of every M (solver_step_harness.emu_runs_parallel's reason)
def problem_of(spec):
    """(library keyword arguments, oracle keyword arguments, P, X0) of spec["batch"]: "named" (N = 20 production grid, the 12 + 4 named members) or
    dict(seed, B) of make_batch(B, N, 0.6, seed); spec["form"]: "plain" or "rc" (solver_step_harness.RUN_COST)"""
    N = spec["N"]
    if spec["batch"] == "named":
        P, X0 = named_batch(N)
    else:
        P, X0, _, _ = lc("problem").make_batch(spec["batch"]["B"], N, 0.6, seed=spec["batch"]["seed"])
    kw = dict(run_cost=H.RUN_COST) if spec["form"] == "rc" else {}
    return kw, P, X0


def emu_runs_parallel(spec, members, plan, tmp_dir, rho=None, jobs=None):
    """plan: {M: caps}.  Returns (P, X0 of the chosen members, {M: {cap: run}})"""
    kw, P, X0 = problem_of(spec)
    members = list(members)
    todo = [dict(spec=spec, member=b, plan=[(M, cap) for M, caps in plan.items() for cap in caps], rho=rho,
                 out=os.path.join(str(tmp_dir), "feas_emu_%s_N%d_m%d_rho%s.npz" % (spec["form"], spec["N"], b, rho))) for b in members]
    runs = load_runs(run_workers(__file__, todo, jobs), ("ws", "prof"))
    off = lc("capi").workspace_offsets(spec["N"])
    return P[members], X0[members], {M: {cap: dict(runs[M, cap], off=off) for cap in caps} for M, caps in plan.items()}


def _emu_worker(job):
    spec, b = job["spec"], job["member"]
    kw, P, X0 = problem_of(spec)
    L = lc("capi").LandingLib(spec["N"], lib_path=EMU_LIB, **kw)
    save_runs(job["out"], {(M, cap): capped_run(L, P[b:b + 1], X0[b:b + 1], feas_opts(L, M, job["rho"]), cap) for M, cap in job["plan"]}, ("ws", "prof"))
    L.close()


if __name__ == "__main__":
    worker_main(_emu_worker)
