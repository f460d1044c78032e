"""GPU tests (MI355X) at the reference's own KNITRO solution and multipliers of the production kinodynamic refinement problem
(tests/golden/n1_kinodyn_multipliers.npz tag m, tests/kd_reference_kkt.py; the CPU side and what the vector pins: tests/test_kd_multipliers_cpu.py):
the function layer AT (x*, lam*) through the C ABI and through the shipped CasADi drop-in, every column of the Hessian of lam*' g at x*, the warm
re-solve started from x*, and the cold chain SRBM solve -> refinement from the file's initial state on the production grid."""
import ctypes as C
import os

import numpy as np
import pytest

import kd_reference_kkt as K
from conftest import ROOT, lc
from test_gpu_kd_solver import _certify
from test_pipeline_cpu import _mirror

pytestmark = pytest.mark.gpu
N, KKT_TOL, MU = K.N, K.KKT_TOL, K.MU
PKG = os.path.join(ROOT, "landing-controller_amd")


@pytest.fixture(scope="module")
def ctx():
    L = lc("capi").LandingLib(N, device=0)
    R = lc("rbd").Rbd(L)
    yield L, R
    L.close()


def test_casadi_face_at_the_reference_solution_gpu(ctx):
    """landing_kinodyn_casadi_eval_host on the device at (x*, lam*), lam_f = 1: the checks of test_casadi_face_at_the_reference_solution_emulated"""
    L, R = ctx
    K.casadi_face_at_reference(R, "device")


def test_knitro_dropin_at_the_reference_solution_gpu(ctx):
    """the shipped landingCtrller_KNITRO_mi355x.so called as CasADi's external() calls it (nlp_jac_g, nlp_grad) with the reference's (x*, lam*): the solver that
    loads the drop-in would be handed a stationary point at the reference's solution -- g, grad_gamma_x, grad f + J' lam* <= 1e-6 through the CCS values"""
    L, R = ctx
    pr = K.Problem("m")
    nx, ng = lc("kinodyn").dims(N)
    p = pr.knitro_params()
    lib = C.CDLL(os.path.join(PKG, "landingCtrller_KNITRO_mi355x.so"))
    dp = C.POINTER(C.c_double); llp = C.POINTER(C.c_longlong)
    lib.nlp_jac_g_sparsity_out.restype = llp; lib.nlp_jac_g_sparsity_out.argtypes = [C.c_longlong]
    lib.nlp_incref()
    spj = lib.nlp_jac_g_sparsity_out(1)
    assert (spj[0], spj[1]) == (ng, nx)
    nnz = spj[2 + nx]
    colind = np.array(spj[2:2 + nx + 1]); rows = np.array(spj[3 + nx:3 + nx + nnz])
    ptr = lambda a: a.ctypes.data_as(dp)

    def call(name, ins, outs):
        arg = (dp * len(ins))(*[ptr(a) if a is not None else None for a in ins])
        res = (dp * len(outs))(*[ptr(a) if a is not None else None for a in outs])
        f = getattr(lib, name); f.restype = C.c_int
        assert f(arg, res, None, None, 0) == 0
    x, lam, lf = pr.x.copy(), pr.lam.copy(), np.array([1.0])
    g = np.zeros(ng); jac = np.zeros(nnz)
    call("nlp_jac_g", [x, p], [g, jac])
    f = np.zeros(1); g2 = np.zeros(ng); gx = np.zeros(nx); gp = np.zeros(p.size)
    call("nlp_grad", [x, p, lf, lam], [f, g2, gx, gp])
    lib.nlp_decref()
    assert np.array_equal(g, g2) and abs(f[0] - pr.grad_f()[0]) <= 1e-15
    lb, ub = R.kinodyn_casadi_bounds(N, p)
    K.check_face_outputs(pr, g, gx, K.scatter_ccs(colind, rows, jac, (ng, nx)), lb, ub, "drop-in")


def test_hessian_at_the_reference_solution_gpu(ctx):
    """landing_kinodyn_nlp_hess on the device with lam* at x*: EVERY column of the [972, 972] Hessian of lam*' g against central differences of the oracle's
    complex-step gradient (tests/kd_reference_kkt.py HESS_TOL: 1e-6 of the largest entry).  Measured through the host emulation: largest entry 5.655e-4, worst error 5.3e-13 =
    9.3e-4 x the tolerance (column 630)."""
    L, R = ctx
    K.hessian_at_reference(R, "cuda", range(lc("kinodyn").dims(N)[0]), "device")


def test_warm_resolve_from_the_reference_solution(ctx):
    """landing_kinodyn_solve_batch_host with the warm preset from x0 = x*, the file's own initial state, stance and kd.bounds: converges (status 0) within the
    preset's max_iter to a KKT point <= 1e-6 under the oracle with f <= 1e-7.  The optimum f* = 0 is a continuum, so closeness to x* is printed, not asserted.
    Measured through the host emulation (tests/test_kd_multipliers_cpu.py): 4 iterations, |x - x*|_inf 1.26e-2, f 3.4e-11, KKT 2.0e-8 / 3.1e-7 / 1.0e-7."""
    L, R = ctx
    K.warm_resolve_from_reference(R, _certify, "device")


def test_cold_known_answer_on_the_production_grid(ctx):
    """the drop state X*(:, 1) of main_scripts/prevSoln.mat on the production grid (test_gpu_kd_solver.py::test_stored_drop_known_answer is uniform-grid only):
    SRBM solve -> make_args24 -> landing_solve_kinodyn_24 ends converged (status 0: pitch -47 deg, but the file's own solution lies inside tighter bounds, so no presolve certificate can fire -- the branch
    for one asserts the certificate's rows all the same) with f <= 1e-7, certified
    <= 1e-6 under the oracle; the same state through pipeline.RefineChain is kept, and every output equals the passes called one by one on the device (SRBM solve,
    pose, cold refinement, warm re-solve, final choice), bit for bit.  Measured through the host emulation (host path only): SRBM 28 iterations, refinement status 0 after 53 iterations, f 3.3e-12, KKT 7.5e-9 / 4.4e-7 / 1.0e-7;
    the chain: status [0, 0, 0], iterations [28, 53, 4], kept, equal to its passes bit for bit."""
    import torch
    from oracle import kinodyn_oracle as ko
    L, R = ctx
    P, kd, pl = lc("problem"), lc("kinodyn"), lc("pipeline")
    pr = K.Problem("m")
    mass, Ib, Ibi = K.consts()
    q, qd = pr.q_init, pr.qd_init
    dt = np.asarray(P.REFERENCE_DT_GRID, float)
    assert np.array_equal(dt, pr.dt)
    consts = P.production_constants("main")
    assert consts.mu == MU
    p, x0s, _, _ = P.make_member(N, 0.6, q, qd, consts, dt)
    srbm = L.solve_host(p[None], x0s[None])
    assert srbm["status"][0] == 0
    args = kd.make_args24(N, q[None], qd[None], srbm["x"], dt, mass, Ib, Ibi, mu=consts.mu)
    s = R.kinodyn_solve_24(N, args)
    lb, ub, cost, _ = kd.member_problem(N, q, qd, srbm["x"][0], kin_box_y0=0.125)      # the 24-argument function's form (landing_kinodyn_form_knitro)
    print("cold refinement from the reference's drop state: SRBM %d iterations; refinement status %d, %d iterations, f %.3e, kkt %s" % (
        srbm["iters"][0], s["status"][0], s["iters"][0], s["f"][0], np.array2string(s["kkt"][0], precision=3)))
    if s["status"][0] == 3:      # presolve certificate: a row of the first interval over FIXED variables is violated (test_refinement_of_1024_...)
        g = ko.nlp_g_batch(s["x"], N, dt, mass, Ib, Ibi, consts.mu)
        rows = 48 + 16 + 15 * np.repeat(np.arange(4), 5) + np.tile([0, 8, 9, 10, 11], 4)
        viol = np.maximum(np.maximum(lb - g[0], g[0] - ub), 0.0)
        assert viol[rows].max() > KKT_TOL and s["iters"][0] == 0 and np.isclose(viol.max(), s["kkt"][0, 0], rtol=1e-9, atol=1e-12)
    else:
        assert s["status"][0] == 0 and s["f"][0] <= 1e-7, (s["status"], s["f"], s["kkt"])
        k = _certify(s["x"], s["lam_g"], lb[None], ub[None], cost[None], dt, consts.mu)
        print("  certified under the oracle: %s" % np.array2string(k[0], precision=4))
        assert k.max() <= 1e-6, k
    # the chain on the same state, against its passes one by one on the device
    chain = pl.RefineChain(N, device=0)
    f64, i32 = dict(device="cuda", dtype=torch.float64), dict(device="cuda", dtype=torch.int32)
    dP, dX0 = torch.as_tensor(p[None].copy(), **f64), torch.as_tensor(x0s[None].copy(), **f64)
    xs_c = torch.empty(1, chain.L.nx, **f64)
    out = chain.run_device(dP, dX0, out=chain.alloc(1, lam=True), x_srbm=xs_c)
    torch.cuda.synchronize()
    r = chain.to_host(out)
    st = torch.cuda.current_stream().cuda_stream
    nxk, ng = kd.dims(N)
    xs, st0, it0 = torch.empty(1, L.nx, **f64), torch.empty(1, **i32), torch.empty(1, **i32)
    L.solve_device(1, dP.data_ptr(), dX0.data_ptr(), L.default_opts(), xs.data_ptr(), d_status=st0.data_ptr(), d_iters=it0.data_ptr(), stream=st)
    dlb, dub, dcost, dx0 = torch.empty(1, ng, **f64), torch.empty(1, ng, **f64), torch.empty(1, 24, **f64), torch.empty(1, nxk, **f64)
    R.kinodyn_pose_device(1, dP.data_ptr(), xs.data_ptr(), dlb.data_ptr(), dub.data_ptr(), dcost.data_ptr(), dx0.data_ptr(), stream=st)
    passes = []
    for o, start in ((R.kinodyn_default_opts(), dx0), (R.kinodyn_warm_opts(), None)):
        start = start if start is not None else passes[-1]["x"]
        pp = dict(x=torch.empty(1, nxk, **f64), f=torch.empty(1, **f64), lam=torch.empty(1, ng, **f64), st=torch.empty(1, **i32), it=torch.empty(1, **i32), kkt=torch.empty(1, 3, **f64))
        R.kinodyn_solve_device(1, N, dlb.data_ptr(), dub.data_ptr(), dcost.data_ptr(), start.data_ptr(), dt, mass, Ib, Ibi, consts.mu, o, pp["x"].data_ptr(), pp["f"].data_ptr(),
                               pp["lam"].data_ptr(), pp["st"].data_ptr(), pp["it"].data_ptr(), pp["kkt"].data_ptr(), stream=st)
        passes.append(pp)
    torch.cuda.synchronize()
    a, w = ({k_: v.cpu().numpy() for k_, v in pp.items()} for pp in passes)
    assert np.array_equal(xs_c.cpu().numpy(), xs.cpu().numpy())
    status3 = np.stack([st0.cpu().numpy(), a["st"], w["st"]], axis=1); iters3 = np.stack([it0.cpu().numpy(), a["it"], w["it"]], axis=1)
    assert np.array_equal(r["status"], status3) and np.array_equal(r["iters"], iters3)
    take1 = (w["st"] != 0) & (a["st"] == 0)
    for mine, theirs in (("x", "x"), ("f", "f"), ("lam_g", "lam"), ("kkt", "kkt")):
        assert np.array_equal(r[mine], np.where(take1.reshape((-1,) + (1,) * (a[theirs].ndim - 1)), a[theirs], w[theirs])), mine
    print("chain on the same state: status %s, iterations %s, final %d, kept %d, f %.3e" % (r["status"][0].tolist(), r["iters"][0].tolist(), r["final_status"][0], r["n_kept"], r["f"][0]))
    if s["status"][0] == 3:
        assert r["final_status"][0] == 3 and r["n_kept"] == 0
    else:
        assert r["final_status"][0] == 0 and r["n_kept"] == 1 and np.array_equal(r["index"], [0]) and r["f"][0] <= 1e-7
        mlb, mub, mcost, _ = _mirror(p[None], srbm["x"], N)
        k = _certify(r["x"], r["lam_g"], mlb, mub, mcost, dt, consts.mu)
        assert k.max() <= KKT_TOL * 1.0001, k
    chain.close()
