"""What the CPU and the GPU tests of the kinodynamic refinement solver's feasibility-phase step share (test helper): landing_kinodyn_solve_batch with max_iter = M,
feas_phase = 1, feas_jam = 0, portfolio off, under landing_debug_iter_cap = M + 1 + j; the row state (s, en, ep, zL, wn, zU, wp), the step (dx, ds, yn) and the
iteration scalars from the member's workspace block (landing_debug_kd_*); compared with tests/elastic_newton_reference.py.  The SRBM solver's counterpart is
tests/feas_step_harness.py: the construction, the pairs a run holds and the tolerances are the same (its docstring), and check_update is shared."""
import os
import threading

import numpy as np

import elastic_newton_reference as er
import feas_step_harness as F
import kd_newton_reference as kr
import kd_step_harness as KH
import newton_reference as nr
from conftest import lc
from emu_support import EMU_LIB, pool_map, run_workers, worker_main

EPS = np.finfo(float).eps
_LIB_LOCK = threading.Lock()


def feas_opts(R, M, rho=None):
    o = KH.step_opts(R, None, M)
    o.feas_phase = 1; o.feas_jam = 0
    if rho is not None:
        o.feas_rho = rho
    return o


def capped_run(R, probs, X0, opts, cap):
    R.L._check(R.L.lib.landing_debug_iter_cap(R.L.ctx, int(cap)), "landing_debug_iter_cap")
    try:
        return KH.kd_run(R, probs, X0, opts)
    finally:
        R.L._check(R.L.lib.landing_debug_iter_cap(R.L.ctx, 0), "landing_debug_iter_cap")


def check_entry(pr, opts, M, run_M, run_0, b, label):
    """j = 0 (cap M + 1) against the run that stopped at x_M (cap M); a member the presolve certifies, or one that converged within M iterations, has no entry"""
    vM, recM = KH.member_view(run_M, b); v, rec = KH.member_view(run_0, b)
    if run_M["res"]["status"][b] in (0, 3) or run_0["res"]["iters"][b] != M + 1 or not rec["feas"]:
        return "%s: no entry (status %d after %d iterations at cap M, %d iterations at cap M + 1, feas %d)" % (
            label, run_M["res"]["status"][b], run_M["res"]["iters"][b], run_0["res"]["iters"][b], rec["feas"])
    assert recM["feas"] == 0 and run_M["res"]["iters"][b] == M and rec["it"] == M + 1, (label, recM, rec)
    x = run_0["res"]["x"][b]
    assert np.array_equal(x, run_M["res"]["x"][b]) and np.array_equal(v["x"], x), (label, "the phase is not entered at x_M")
    assert rec["mu"] == opts.mu_init, (label, rec["mu"])
    go = pr.g(x)
    eg = np.abs(v["g"][24:] - go[24:]) / np.maximum(1.0, np.abs(go[24:]))
    assert eg.max() <= 1e-12, (label, "g at the entry", float(eg.max()))
    e0 = er.init_rows(v["g"], pr.lb, pr.ub, opts.mu_init, opts.feas_rho, 24)
    for k in ("s", "en", "ep"):
        assert np.array_equal(v[k][24:], e0[k][24:]), (label, k, int(np.argmax(v[k][24:] != e0[k][24:])) + 24)
    for k in ("zL", "zU", "wn", "wp"):
        ok = np.abs(v[k][24:] - e0[k][24:]) <= 4 * EPS * np.abs(e0[k][24:])
        assert ok.all(), (label, k, int(np.argmin(ok)) + 24)
    eq = (pr.lb == pr.ub) & (np.arange(pr.ng) >= 24)
    ie = ~eq & (np.arange(pr.ng) >= 24)
    assert not v["y"][eq].any() and np.array_equal(v["y"][ie], (v["zU"] - v["zL"])[ie]), (label, "y at the entry")
    print("%s: entry state restated; g against the oracle %.1e" % (label, float(eg.max())))
    return None


def check_pair(pr, opts, runs, T, b, label, factor=nr.TOL_FACTOR):
    """the step of run T + 1 against the reference at the state run T ended in (J and H: the product's function layer at that point, as kd_step_harness.check_pair
    takes them by default; the function layer has its own tests against the oracle), then the update"""
    rk, rn = runs[T], runs[T + 1]
    vk, reck = KH.member_view(rk, b); vn, recn = KH.member_view(rn, b)
    if not (rk["res"]["iters"][b] == T and rn["res"]["iters"][b] == T + 1 and reck["it"] == T and recn["it"] == T + 1):
        return "%s: did not stop at the caps %d, %d (status %d after %d iterations)" % (label, T, T + 1, rn["res"]["status"][b], rn["res"]["iters"][b]), None
    if not (reck["feas"] and recn["feas"]):
        return "%s: outside the phase (feas %d, %d)" % (label, reck["feas"], recn["feas"]), None
    assert recn["pending"] == 0 and recn["nfact"] > reck["nfact"], (label, recn)
    xk, xn = rk["res"]["x"][b], rn["res"]["x"][b]
    assert np.array_equal(vk["x"], xk) and np.array_equal(vk["y"][24:], rk["res"]["lam_g"][b][24:])
    N = pr.N
    J = kr.jacobian_from_blocks(N, rk["Jb"][b]); Hm = kr.hessian_from_blocks(N, rk["Hb"][b])
    y = np.array(rk["res"]["lam_g"][b])
    ref = er.kd_solve_step(pr, dict(x=xk, y=y), F.row_state(vk), recn["mu"], opts.feas_rho, kr.d_reg(N, recn["delta"]), J, Hm)
    assert ref["res"] <= 1e-13, (label, "the reference did not refine", ref["res"])
    err = nr.errors(ref, vn["dx"], vn["ds"], vn["yn"])
    ratio = nr.ratios(ref, err)
    bound = {k: v * (factor / nr.TOL_FACTOR) for k, v in nr.bounds_of(ref).items()}
    bwd = nr.backward_error(ref, vn["dx"], vn["ds"], vn["yn"])
    print("%s (mu %.1e delta %.1e alpha %.2e a_du %.2e): err dx %.1e ds %.1e y %.1e | ratio dx %.2g ds %.2g y %.2g (bound %g) | backward error %.1e" % (
        label, recn["mu"], recn["delta"], recn["alpha"], recn["a_du"], err["dx"], err["ds"], err["y"], ratio["dx"], ratio["ds"], ratio["y"], factor, bwd))
    for k in ("dx", "ds", "y"):
        assert err[k] <= bound[k], (label, k, err[k], bound[k], ref["e_aug"][k], ref["e_cond"][k])
    if factor != nr.TOL_FACTOR:
        assert bwd <= 1e-12, (label, "backward error", bwd)
    F.check_update(ref, opts, vk, vn, recn, xk, xn, pr.lb, pr.ub, label, factor=factor)
    return None, ratio


def check_config(probs, opts, M, js, runs, label, factor=nr.TOL_FACTOR):
    """every member's entry and every pair (j, j + 1) of js; members the presolve certifies are left out altogether.  Returns feas_step_harness.check_config's dict."""
    Bn = len(probs)
    certified = [b for b in range(Bn) if runs[M]["res"]["status"][b] == 3 and runs[M]["res"]["iters"][b] == 0]
    for b in certified:
        print("  left out: %s member %d is certified infeasible by the presolve" % (label, b))
    members = [b for b in range(Bn) if b not in certified]
    jobs = [("entry", b) for b in members] + [(j, b) for j in js for b in members]

    def one(job):
        j, b = job
        if j == "entry":
            return job, check_entry(probs[b], opts, M, runs[M], runs[M + 1], b, "%s member %d entry" % (label, b)), None
        reason, ratio = check_pair(probs[b], opts, runs, M + 1 + j, b, "%s member %d j %d" % (label, b, j), factor=factor)
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
    print("%s: %d pairs checked, %d skipped, %d members without an entry, %d certified by the presolve; WORST RATIO dx %.3g ds %.3g y %.3g" % (
        label, checked, len(skipped), len(no_entry), len(certified), worst["dx"], worst["ds"], worst["y"]))
    return dict(worst=worst, checked=checked, skipped=skipped, no_entry=no_entry, by_j=by_j, members=members)


# ---- the host emulation in parallel: one process per member (kd_step_harness.emu_member), which runs the member alone at every cap
def emu_runs_parallel(N, members, M, caps, tmp_dir, rho=None, jobs=None):
    """Returns (problems, X0, opts, {cap: run}) of the members, in the order given"""
    todo = [dict(N=N, member=m, M=M, caps=list(caps), rho=rho, out=os.path.join(str(tmp_dir), "kd_feas_emu_N%d_M%d_m%d_rho%s.npz" % (N, M, m, rho))) for m in members]
    paths = run_workers(__file__, todo, jobs)
    probs, X0 = zip(*[KH.emu_member(dict(N=N, member=m)) for m in members])
    with _LIB_LOCK:      # (callers may collect several configurations from threads; the library is opened by one at a time)
        L = lc("capi").LandingLib(20, lib_path=EMU_LIB); R = lc("rbd").Rbd(L)
        opts, runs = feas_opts(R, M, rho), KH.load_kd_runs(paths, R, N)
        L.close()
    return list(probs), np.array(X0), opts, runs


def _emu_worker(job):
    pr, x0 = KH.emu_member(dict(N=job["N"], member=job["member"]))
    L = lc("capi").LandingLib(job["N"], lib_path=EMU_LIB); R = lc("rbd").Rbd(L)
    KH.save_kd_runs(job["out"], R, {cap: capped_run(R, [pr], x0[None], feas_opts(R, job["M"], job["rho"]), cap) for cap in job["caps"]})
    L.close()


if __name__ == "__main__":
    worker_main(_emu_worker)
