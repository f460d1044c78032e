"""GPU parity tests of the function layer (run with -m gpu on an MI355X), all through the C ABI.

Bar: fp64, <=1e-11 absolute against the oracle / the reference's golden outputs (values are O(1..500)).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, lc

pytestmark = pytest.mark.gpu
PKG = os.path.join(ROOT, "landing-controller_amd")


@pytest.fixture(scope="module")
def libs():
    capi = lc("capi")
    return {N: capi.LandingLib(N, device=0) for N in (20, 40)}


def _cmp(out, O, x, p, lf, lam, tol=1e-11):
    for b in range(x.shape[0]):
        f, gf = O.grad_f(x[b], p[b]); g, jac = O.jac_g(x[b], p[b])
        h = O.hess_l(x[b], p[b], lf[b], lam[b]); _, _, gx, gp = O.grad(x[b], p[b], lf[b], lam[b])
        assert abs(out["f"][b] - f) <= tol * max(1, abs(f))
        assert np.max(np.abs(out["grad_f"][b] - gf)) <= tol
        assert np.max(np.abs(out["g"][b] - g)) <= tol
        assert np.max(np.abs(out["jac"][b] - jac)) <= tol
        assert np.max(np.abs(out["hess"][b] - h)) <= 10 * tol
        assert np.max(np.abs(out["grad_gamma_x"][b] - gx)) <= 10 * tol
        assert np.max(np.abs(out["grad_gamma_p"][b] - gp)) <= 100 * tol


@pytest.mark.parametrize("N", [20, 40])
def test_sweep_matches_oracle_random(libs, oracle_mod, N):
    O = oracle_mod.Oracle(N)
    rng = np.random.default_rng(100 + N)
    B = 8
    x = rng.normal(size=(B, O.nx)) * 0.5; p = rng.uniform(0.5, 1.5, size=(B, O.np_))
    lam = rng.normal(size=(B, O.ng)); lf = rng.uniform(0.5, 2, size=B)
    _cmp(libs[N].eval_host(x, p, lf, lam), O, x, p, lf, lam)


@pytest.mark.parametrize("N", [20, 40])
def test_sweep_matches_oracle_realistic(libs, oracle_mod, N):
    """drop states as the callers sample them (incl. +-60 deg pitch), perturbed initial guesses"""
    O = oracle_mod.Oracle(N)
    P, X0, _, _ = lc("problem").make_batch(16, N, 0.6, seed=5)
    rng = np.random.default_rng(6)
    X = X0 + 0.02 * rng.normal(size=X0.shape)
    X[:, 12 * (N + 1) + 12::24] += 50 * rng.random(size=X[:, 12 * (N + 1) + 12::24].shape)
    lam = rng.normal(size=(16, O.ng)); lf = np.ones(16)
    _cmp(libs[N].eval_host(X, P, lf, lam), O, X, P, lf, lam, tol=2e-10)


def test_sweep_matches_reference_golden(libs):
    d = np.load(os.path.join(GOLDEN, "n20_eval.npz"))
    for c in range(3):
        g = lambda k: d[f"c{c}_{k}"]
        out = libs[20].eval_host(g("x"), g("p"), np.array([float(g("lam_f"))]), g("lam_g"))
        for k, tol in (("f", 1e-12), ("g", 1e-12), ("grad_f", 1e-12), ("jac", 1e-12), ("hess", 1e-11), ("grad_gamma_x", 1e-11), ("grad_gamma_p", 1e-10)):
            assert np.max(np.abs(out[k][0] - g(k))) <= tol * max(1.0, np.max(np.abs(g(k)))), k


def test_casadi_dropin_on_gpu_matches_reference_golden():
    """the drop-in .so called exactly as CasADi's external() calls the reference's library"""
    lib = C.CDLL(os.path.join(PKG, "landingCtrller_IPOPT_mi355x.so"))
    dp = C.POINTER(C.c_double)
    d = np.load(os.path.join(GOLDEN, "n20_eval.npz"))
    x, p, lam = d["c1_x"].copy(), d["c1_p"].copy(), d["c1_lam_g"].copy()
    lf = np.array([float(d["c1_lam_f"])])
    ptr = lambda a: a.ctypes.data_as(dp)

    def call(name, ins, outs):
        arg = (dp * len(ins))(*[ptr(a) if a is not None else None for a in ins])
        res = (dp * len(outs))(*[ptr(a) if a is not None else None for a in outs])
        f = getattr(lib, name); f.restype = C.c_int
        assert f(arg, res, None, None, 0) == 0
    lib.nlp_incref()
    g = np.zeros(2092); jac = np.zeros(7664)
    call("nlp_jac_g", [x, p], [g, jac])
    assert np.max(np.abs(g - d["c1_g"])) < 1e-12 and np.max(np.abs(jac - d["c1_jac"])) < 1e-12
    h = np.zeros(3780)
    call("nlp_hess_l", [x, p, lf, lam], [h])
    assert np.max(np.abs(h - d["c1_hess"])) < 1e-11
    f = np.zeros(1); gx = np.zeros(732); gp = np.zeros(354)
    call("nlp_grad", [x, p, lf, lam], [f, None, gx, gp])      # res[1]==NULL is skipped
    assert abs(f[0] - d["c1_f"]) < 1e-15 and np.max(np.abs(gx - d["c1_grad_gamma_x"])) < 1e-11
    assert np.max(np.abs(gp - d["c1_grad_gamma_p"])) < 1e-10
    f2 = np.zeros(1); gf = np.zeros(732)
    call("nlp_grad_f", [x, p], [f2, gf])
    assert np.max(np.abs(gf - d["c1_grad_f"])) < 1e-12
    # arg[i]==NULL reads as zeros (landingCtrller_IPOPT.c:69-70)
    g0 = np.zeros(2092)
    call("nlp_g", [None, p], [g0])
    assert np.all(np.isfinite(g0)) and np.all(g0[:36] == 0)
    lib.nlp_decref()


def test_knitro_dropin_on_gpu_matches_oracle():
    """landingCtrller_KNITRO_mi355x.so (round 6): the CasADi-external face of the kinodynamic refinement NLP (generate_landingCtrller_KNITRO.m:360-377 generates and loads
    ./landingCtrller_KNITRO.so; a missing blob of the reference) called exactly as CasADi's external() would -- metadata CasADi asserts on (external.cpp:325-363),
    arg / res pointer arrays, NULL outputs skipped -- at the script's size (21 knots: x 972, p 373, g 2844) against the oracle (KD oracle: pinned by the reference's own
    KNITRO multipliers for 19 of its 27 row groups, the other 8 -- c_init, the four terminal boxes, leg torques, joint limits lower / upper -- by feasibility only:
    tests/test_kd_multipliers_cpu.py; the drop-in AT the reference's solution: tests/test_gpu_kd_multipliers.py; derivatives of the oracle are complex-step /
    Richardson derivatives of itself)."""
    from oracle import kinodyn_oracle as ko
    kd = lc("kinodyn")
    N, nx, ng, npar = 20, 972, 2844, 373
    lib = C.CDLL(os.path.join(PKG, "landingCtrller_KNITRO_mi355x.so"))
    dp = C.POINTER(C.c_double); llp = C.POINTER(C.c_longlong)
    lib.nlp_incref()
    for fn, i, want in (("nlp_jac_g_sparsity_in", 0, (nx, 1)), ("nlp_jac_g_sparsity_in", 1, (npar, 1)), ("nlp_jac_g_sparsity_out", 0, (ng, 1)), ("nlp_jac_g_sparsity_out", 1, (ng, nx)), ("nlp_hess_l_sparsity_out", 0, (nx, nx))):
        f = getattr(lib, fn); f.restype = llp; f.argtypes = [C.c_longlong]
        sp = f(i); assert (sp[0], sp[1]) == want, (fn, i, sp[0], sp[1])
    spj = lib.nlp_jac_g_sparsity_out(1); nnz_j = spj[2 + nx]
    sph = lib.nlp_hess_l_sparsity_out(0); nnz_h = sph[2 + nx]
    assert (nnz_j, nnz_h) == (13536, 5720)      # the counts of landing_kinodyn_pattern
    lib.nlp_grad_name_out.restype = C.c_char_p; lib.nlp_grad_name_out.argtypes = [C.c_longlong]
    assert [lib.nlp_grad_name_out(i) for i in range(4)] == [b"f", b"g", b"grad_gamma_x", b"grad_gamma_p"]
    mass, Ib, Ibi = lc("constants").robot_constants()
    Ib, Ibi = np.asarray(Ib), np.asarray(Ibi)
    rng = np.random.default_rng(21)
    dt = np.asarray(lc("problem").REFERENCE_DT_GRID, float); mu = 0.75
    x = 0.3 * rng.normal(size=nx); x[2:12 * (N + 1):12] += 0.3
    lam = rng.normal(size=ng); lf = np.array([0.6])
    Xref = rng.normal(size=(12, N + 1)); QN = np.array(kd.QN_DEFAULT, float)
    q_init = np.array([0, 0, 0.6, 0.1, -0.3, 0.05]); qd_init = np.array([0.1, -0.2, 0.3, 0.5, -0.4, -3.0])
    p = kd.pack_params_knitro(N, Xref=Xref, dt=dt, q_init=q_init, qd_init=qd_init, c_init=kd.c_init_of(q_init), jpos_min=kd.JPOS_MIN, jpos_max=kd.JPOS_MAX,
                              q_term_min=[-10, -10, 0.15, -0.1, -0.1, -10], q_term_max=[10, 10, 5, 0.1, 0.1, 10], qd_term_min=[-10, -10, -10, -.5, -.5, -.5], qd_term_max=[10, 10, 10, .5, .5, .5],
                              q_min=[-10, -10, 0.075, -10, -10, -10], QN=QN, mu=mu, l_leg_max=0.4, mass=mass, Ib=Ib, Ib_inv=Ibi, kin_box=kd.kin_box_of(q_init[3:6], qd_init[3:6]))
    ptr = lambda a: a.ctypes.data_as(dp)

    def call(name, ins, outs):
        arg = (dp * len(ins))(*[ptr(a) if a is not None else None for a in ins])
        res = (dp * len(outs))(*[ptr(a) if a is not None else None for a in outs])
        f = getattr(lib, name); f.restype = C.c_int
        assert f(arg, res, None, None, 0) == 0
    g = np.zeros(ng); jac = np.zeros(nnz_j)
    call("nlp_jac_g", [x, p], [g, jac])
    assert np.abs(g - ko.nlp_g(x, N, dt, mass, Ib, Ibi, mu)).max() <= 1e-11
    f = np.zeros(1); gx = np.zeros(nx); gp = np.zeros(npar)
    call("nlp_grad", [x, p, lf, lam], [f, None, gx, gp])      # res[1] == NULL is skipped
    d = x[12 * N:12 * N + 12] - Xref[:, N]
    assert abs(f[0] - QN @ d ** 2) <= 1e-12
    gfx = np.zeros(nx); gfx[12 * N:12 * N + 12] = lf[0] * 2 * QN * d
    ref = ko.grad_lagrangian_batch(x[None], lam[None], N, dt, mass, Ib, Ibi, mu, gfx[None])[0]
    assert np.abs(gx - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
    # J' lam through the CCS values == grad_gamma_x - lam_f grad f
    colind = np.array(spj[2:2 + nx + 1]); rows = np.array(spj[3 + nx:3 + nx + nnz_j])
    jtl = np.array([jac[colind[c]:colind[c + 1]] @ lam[rows[colind[c]:colind[c + 1]]] for c in range(nx)])
    assert np.abs(jtl - (gx - gfx)).max() <= 1e-10 * max(1.0, np.abs(gx).max())
    # Hessian columns against central differences of the oracle's exact gradient
    h = np.zeros(nnz_h)
    call("nlp_hess_l", [x, p, lf, lam], [h])
    hc = np.array(sph[2:2 + nx + 1]); hr = np.array(sph[3 + nx:3 + nx + nnz_h])
    H = np.zeros((nx, nx))
    for c in range(nx):
        H[hr[hc[c]:hc[c + 1]], c] = h[hc[c]:hc[c + 1]]
    H = H + np.triu(H, 1).T
    def grad_gamma(xx):
        gq = np.zeros(nx); gq[12 * N:12 * N + 12] = lf[0] * 2 * QN * (xx[12 * N:12 * N + 12] - Xref[:, N])
        return ko.grad_lagrangian_batch(xx[None], lam[None], N, dt, mass, Ib, Ibi, mu, gq[None])[0]
    for j in (4, 9, 12 * 7 + 3, 12 * N + 2, 12 * (N + 1) + 5, 12 * (N + 1) + 12 * N + 30, nx - 3):
        e = np.zeros(nx); e[j] = 1e-5
        col = (grad_gamma(x + e) - grad_gamma(x - e)) / 2e-5
        assert np.abs(H[:, j] - col).max() <= 1e-6 * max(1.0, np.abs(col).max()), j
    assert gp[252 + 3] != 0.0 and (gp[12 * (N + 1) + N:12 * (N + 1) + N + 60] == 0.0).all()      # dt enters g; q_init ... jpos_max sit in the bounds only
    lib.nlp_decref()


def test_ccc_dropin_on_gpu_matches_oracle(oracle_mod):
    """nlp_quad_SRBM_mi355x.so (the N=41 script's NLP: kin-box .05/.05/.27, running cost, QX / Qc / Qf / Uref in p) through the CasADi ABI
    against the oracle; no generated C of that script exists in the reference, so the oracle's restatement (finite-difference checked,
    tests/test_ccc_params.py, tests/test_hess_rc.py) is the pin"""
    N = 40
    rc = dict(QX=[0.3, 0.2, 10, 1, 1, 0.4, .1, .2, .1, .3, .1, .2], Qc=[1.0, 0.8, 0.5], Qf=[1e-4, 2e-4, 1e-3], f_ref=[0, 0, 0])
    O = oracle_mod.Oracle(N, kin_box=(0.05, 0.05, 0.27), run_cost=rc, ccc_params=True)
    Pm = lc("problem")
    P, X0, _, _ = Pm.make_batch(1, N, 0.6, seed=9)
    rng = np.random.default_rng(4)
    Uref = X0[0][12 * (N + 1):].reshape(24, N, order="F").copy(); Uref[12:] = 5.0 + rng.normal(size=(12, N))
    p = Pm.ccc_from_ipopt_params(N, P[0], Uref, rc["QX"], rc["Qc"], rc["Qf"])
    x = X0[0] + 0.02 * rng.normal(size=X0[0].shape); lam = rng.normal(size=O.ng); lf = np.array([0.7])
    lib = C.CDLL(os.path.join(PKG, "nlp_quad_SRBM_mi355x.so"))
    dp = C.POINTER(C.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)

    def call(name, ins, outs):
        arg = (dp * len(ins))(*[ptr(a) if a is not None else None for a in ins])
        res = (dp * len(outs))(*[ptr(a) if a is not None else None for a in outs])
        f = getattr(lib, name); f.restype = C.c_int
        assert f(arg, res, None, None, 0) == 0
    lib.nlp_incref()
    f = np.zeros(1); g = np.zeros(O.ng); gx = np.zeros(O.nx); gp = np.zeros(O.np_)
    call("nlp_grad", [x, p, lf, lam], [f, g, gx, gp])
    fo, go, gxo, gpo = O.grad(x, p, 0.7, lam)
    assert abs(f[0] - fo) <= 1e-12 * abs(fo) and np.allclose(g, go, rtol=0, atol=1e-12)
    assert np.allclose(gx, gxo, rtol=1e-10, atol=1e-11) and np.allclose(gp, gpo, rtol=1e-10, atol=1e-11)
    h = np.zeros(7560 + 18 * N)
    call("nlp_hess_l", [x, p, lf, lam], [h])
    assert np.allclose(h, O.hess_l_rc(x, p, 0.7, lam), rtol=1e-11, atol=1e-12)
    jac = np.zeros(O.nnz_jac); g2 = np.zeros(O.ng)
    call("nlp_jac_g", [x, p], [g2, jac])
    assert np.allclose(jac, O.jac_g(x, p)[1], rtol=0, atol=1e-12)
    lib.nlp_decref()


def test_bounds_kernel_matches_oracle(libs, oracle_mod):
    import torch
    N = 40
    O = oracle_mod.Oracle(N)
    P, _, _, _ = lc("problem").make_batch(3, N, 0.6, seed=9)
    dP = torch.tensor(P, device="cuda"); lb = torch.empty(3, O.ng, device="cuda", dtype=torch.float64); ub = torch.empty_like(lb)
    libs[N].bounds_device(3, dP.data_ptr(), lb.data_ptr(), ub.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for b in range(3):
        l, u = O.bounds(P[b])
        assert np.array_equal(lb[b].cpu().numpy(), l) and np.array_equal(ub[b].cpu().numpy(), u)


def test_full_size_batch_properties(libs):
    """BASELINE config 2 size (N=40, B=1024) through the device-pointer entry point: size-independent
    checks -- J is the derivative of g (directional finite difference), grad_gamma_x = lam_f grad_f + J^T lam
    with J^T lam rebuilt from the CCS nonzeros, H symmetric action = derivative of grad_gamma_x."""
    import torch
    N, B = 40, 1024
    L = libs[N]
    P, X0, _, _ = lc("problem").make_batch(B, N, 0.6, seed=21)
    rng = np.random.default_rng(2)
    X = X0 + 0.01 * rng.normal(size=X0.shape)
    lam = rng.normal(size=(B, L.ng)); dxn = rng.normal(size=X.shape)
    dev = "cuda"
    t = lambda a: torch.tensor(a, device=dev)
    dX, dP, dlam = t(X), t(P), t(lam)
    mk = lambda *s: torch.empty(*s, device=dev, dtype=torch.float64)
    g, jac, hess, gx, gf = mk(B, L.ng), mk(B, L.nnz_jac), mk(B, L.nnz_hess), mk(B, L.nx), mk(B, L.nx)
    st = torch.cuda.current_stream().cuda_stream
    L.eval_device(B, dX.data_ptr(), dP.data_ptr(), 0, dlam.data_ptr(), 0, g.data_ptr(), gf.data_ptr(), jac.data_ptr(), hess.data_ptr(), gx.data_ptr(), 0, st)
    h = 1e-6
    gp_, gm_, gxp, gxm = mk(B, L.ng), mk(B, L.ng), mk(B, L.nx), mk(B, L.nx)
    dXp, dXm = t(X + h * dxn), t(X - h * dxn)
    L.eval_device(B, dXp.data_ptr(), dP.data_ptr(), 0, dlam.data_ptr(), 0, gp_.data_ptr(), 0, 0, 0, gxp.data_ptr(), 0, st)
    L.eval_device(B, dXm.data_ptr(), dP.data_ptr(), 0, dlam.data_ptr(), 0, gm_.data_ptr(), 0, 0, 0, gxm.data_ptr(), 0, st)
    torch.cuda.synchronize()
    ci, r = L.pattern_jac(); hci, hr = L.pattern_hess()
    cols = np.repeat(np.arange(L.nx), np.diff(ci)); hcols = np.repeat(np.arange(L.nx), np.diff(hci))
    import scipy.sparse as sp
    jac_h, hess_h, gx_h, gf_h = jac.cpu().numpy(), hess.cpu().numpy(), gx.cpu().numpy(), gf.cpu().numpy()
    fd_g = ((gp_ - gm_) / (2 * h)).cpu().numpy(); fd_gx = ((gxp - gxm) / (2 * h)).cpu().numpy()
    assert np.all(np.isfinite(jac_h)) and np.all(np.isfinite(hess_h))
    for b in range(0, B, 37):
        J = sp.csc_matrix((jac_h[b], r, ci), shape=(L.ng, L.nx))
        Hu = sp.csc_matrix((hess_h[b], hr, hci), shape=(L.nx, L.nx))
        H = Hu + sp.triu(Hu, 1).T
        assert np.max(np.abs(J @ dxn[b] - fd_g[b])) < 1e-5 * max(1, np.max(np.abs(fd_g[b])))
        assert np.max(np.abs(gx_h[b] - (gf_h[b] + J.T @ lam[b]))) < 1e-9
        assert np.max(np.abs(H @ dxn[b] - fd_gx[b])) < 1e-4 * max(1, np.max(np.abs(fd_gx[b])))


@pytest.mark.parametrize("N", [3, 7, 33, 64, 100])
def test_sweep_other_horizon_lengths(oracle_mod, N):
    """N is a runtime parameter here (the reference regenerates code per N: N=16/18/21/41/61 variants exist as
    separate scripts): odd N, the smallest N, N=64 (one full wavefront of stages) and N>64 (stage chunks)."""
    capi = lc("capi")
    O = oracle_mod.Oracle(N)
    L = capi.LandingLib(N, device=0)
    assert all(np.array_equal(a, b) for a, b in zip(L.pattern_jac(), O.pattern_jac()))
    assert all(np.array_equal(a, b) for a, b in zip(L.pattern_hess(), O.pattern_hess()))
    rng = np.random.default_rng(N)
    B = 3
    x = rng.normal(size=(B, O.nx)) * 0.5; p = rng.uniform(0.5, 1.5, size=(B, O.np_))
    lam = rng.normal(size=(B, O.ng)); lf = rng.uniform(0.5, 2, size=B)
    _cmp(L.eval_host(x, p, lf, lam), O, x, p, lf, lam)
    L.close()


def test_empty_and_single_member_batches(libs):
    """ragged / degenerate batch sizes: B=0 is a no-op, B=1 works, output subsets may be skipped (res[i]==NULL)"""
    import torch
    L = libs[20]
    L.eval_device(0, 0, 0)                                   # empty batch: returns without touching memory
    P, X0, _, _ = lc("problem").make_batch(1, 20, 0.6, seed=2)
    out = L.eval_host(X0, P, want=("g",))
    assert set(out) == {"g"} and np.all(np.isfinite(out["g"]))
    with pytest.raises(RuntimeError):                        # hess without lam_g is an argument error, not a crash
        L.eval_host(X0, P, want=("hess",))


def test_bad_arguments_are_reported():
    capi = lc("capi")
    with pytest.raises(RuntimeError, match="N must be"):
        capi.LandingLib(1, device=0)
    with pytest.raises(RuntimeError, match="bad device"):
        capi.LandingLib(20, device=99)
