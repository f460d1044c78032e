"""Tracking gains straight from a solved batch on the GPU: landing_tracking_gains_batch (landing_sample_reference_kernel, then
landing_rde_kernel, one stream) against the oracle chain vbl_oracle.sample_reference -> vbl_oracle.rde_backward.

Entry-wise tolerances, the same as tests/test_vbl.py::_check: 1e-10 * max(1, max |A|) on A and likewise on B (closed forms against the
oracle's Jacobians); 1e-9 * max(1, max |P|) on P and likewise on K after the whole backward sweep (the matrix cores accumulate the
products in another order); P symmetric to 1e-10 * max |P|.  The device-resampled reference differs from the oracle's by a few ulps
(tests/test_gains_chain_cpu.py), far inside these."""
import numpy as np
import pytest

from conftest import lc

pytestmark = pytest.mark.gpu


def _weights():
    from oracle import vbl_oracle as vo
    F, Q, R = vo.reference_weights()
    return lc("constants").composite_body_inertia()[0:3, 0:3], 8.252, Q, R, F


def _check_member(P, K, A, Bm, xref, fref, Ib, mass, Q, R, F, dt, rk4):
    from oracle import vbl_oracle as vo
    Po, Ko = vo.rde_backward(xref, fref, Ib, mass, Q, R, F, dt, rk4=rk4)
    for j in range(xref.shape[0]):
        Ao, Bo = vo.vbl_AB(xref[j], fref[j], Ib, mass)
        assert np.max(np.abs(A[j] - Ao)) <= 1e-10 * max(1.0, np.max(np.abs(Ao)))
        assert np.max(np.abs(Bm[j] - Bo)) <= 1e-10 * max(1.0, np.max(np.abs(Bo)))
    assert np.max(np.abs(P - Po)) <= 1e-9 * max(1.0, np.max(np.abs(Po))), np.max(np.abs(P - Po))
    assert np.max(np.abs(K - Ko)) <= 1e-9 * max(1.0, np.max(np.abs(Ko))), np.max(np.abs(K - Ko))
    assert np.max(np.abs(P - np.swapaxes(P, 1, 2))) <= 1e-10 * np.max(np.abs(P))


def _solve_on_device(L, P, X0):
    import torch
    f64 = dict(device="cuda", dtype=torch.float64)
    p, x0 = torch.tensor(P, **f64), torch.tensor(X0, **f64)
    x = torch.empty_like(x0); st = torch.empty(P.shape[0], device="cuda", dtype=torch.int32)
    L.solve_device(P.shape[0], p.data_ptr(), x0.data_ptr(), L.default_opts(), x.data_ptr(), d_status=st.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    return p, x, st


def _gains(L, B, n, x, p, dt_r, rk4, st=None, ref=True):
    import torch
    Ib, mass, Q, R, F = _weights()
    mk = lambda *s: torch.full(s, float("nan"), device="cuda", dtype=torch.float64)
    o = dict(P=mk(B, n, 24, 24), K=mk(B, n, 12, 24), A=mk(B, n, 24, 24), B=mk(B, n, 24, 12))
    if ref:
        o.update(xref=mk(B, n, 24), fref=mk(B, n, 12))
    L.tracking_gains_device(B, x.data_ptr(), p.data_ptr(), dt_r, n, Ib, mass, Q, np.diag(R), F, rk4, d_status=0 if st is None else st.data_ptr(),
                            d_P=o["P"].data_ptr(), d_K=o["K"].data_ptr(), d_A=o["A"].data_ptr(), d_B=o["B"].data_ptr(),
                            d_xref=o["xref"].data_ptr() if ref else 0, d_fref=o["fref"].data_ptr() if ref else 0, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


def test_production_grid_gains_match_oracle_chain():
    """N = 20 on the production time grid (dt = [0.05, 15 x 0.02, 0.05, 0.05, 0.1, 0.2], carried per member in p), B = 8, seed 1 (the
    first 8 members of the batch tests/test_gpu_solver.py solves: the solver alone converges on all of them; >= 6 are required here)."""
    from oracle import vbl_oracle as vo
    capi, Pm = lc("capi"), lc("problem")
    N, B, dt_r, n = 20, 8, 0.02, 26
    L = capi.LandingLib(N, device=0)
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=1, consts=Pm.production_constants("main"), dt_grid="reference")
    p, x, st = _solve_on_device(L, P, X0)
    g = _gains(L, B, n, x, p, dt_r, False, st)
    status, xs = st.cpu().numpy(), x.cpu().numpy()
    conv = np.nonzero(status == 0)[0]
    assert conv.size >= 6, status
    Ib, mass, Q, R, F = _weights()
    o = Pm.param_offsets(N)["dt"]
    for b in conv:
        Xs, Us = Pm.split_solution(N, xs[b])
        xd, ud = vo.sample_reference(Xs, Us, np.concatenate([[0.0], np.cumsum(P[b, o:o + N])]), dt_r, n)
        assert np.max(np.abs(g["xref"][b] - xd)) <= 1e-13 * np.max(np.abs(xs[b])) and np.array_equal(g["fref"][b], ud)
        _check_member(g["P"][b], g["K"][b], g["A"][b], g["B"][b], xd, ud, Ib, mass, Q, R, F, dt_r, False)
    for b in np.nonzero(status != 0)[0]:
        assert all(not v[b].any() for v in g.values())
    L.close()


def test_uniform_grid_gains_bit_identical_to_two_calls():
    """N = 40, B = 6, seed 4 (the batch of tests/test_vbl.py): K and P of the fused call = riccati_gains_device fed with the device-resampled
    references, bit for bit, and both pass the oracle check of the existing GPU test"""
    import torch
    from oracle import vbl_oracle as vo
    capi, Pm = lc("capi"), lc("problem")
    N, B, dt_r, n = 40, 6, 0.022, 28
    L = capi.LandingLib(N, device=0)
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=4)
    p, x, st = _solve_on_device(L, P, X0)
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0).all()
    Ib, mass, Q, R, F = _weights()
    stream = torch.cuda.current_stream().cuda_stream
    mk = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.float64)
    xs = x.cpu().numpy()
    for rk4 in (False, True):
        xref, fref = mk(B, n, 24), mk(B, n, 12)
        L.sample_reference_device(B, x.data_ptr(), p.data_ptr(), dt_r, n, xref.data_ptr(), fref.data_ptr(), stream)
        P2, K2 = mk(B, n, 24, 24), mk(B, n, 12, 24)
        L.riccati_gains_device(B, n, xref.data_ptr(), fref.data_ptr(), Ib, mass, Q, np.diag(R), F, dt_r, rk4, P2.data_ptr(), K2.data_ptr(), stream=stream)
        g = _gains(L, B, n, x, p, dt_r, rk4, st)
        s = _gains(L, B, n, x, p, dt_r, rk4, ref=False)      # reference kept in the context
        for v in (g, s):
            assert np.array_equal(v["K"], K2.cpu().numpy()) and np.array_equal(v["P"], P2.cpu().numpy())
        assert np.array_equal(g["xref"], xref.cpu().numpy()) and np.array_equal(g["fref"], fref.cpu().numpy())
        for b in range(B):
            Xs, Us = Pm.split_solution(N, xs[b])
            xd, ud = vo.sample_reference(Xs, Us, np.linspace(0, 0.6, N + 1), dt_r, n)      # the grid the existing GPU test samples on
            _check_member(g["P"][b], g["K"][b], g["A"][b], g["B"][b], xd, ud, Ib, mass, Q, R, F, dt_r, rk4)
    L.close()


def test_members_are_independent_of_the_batch():
    """B = 70, n = 5: 350 samples = five full workgroups of the resampler and a ragged one, members straddling every boundary; each
    member's rows equal those it gets when it is submitted alone"""
    import torch
    capi, Pm = lc("capi"), lc("problem")
    N, B, dt_r, n = 20, 70, 0.11, 5
    L = capi.LandingLib(N, device=0)
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=9, dt_grid="reference")
    rng = np.random.default_rng(9)
    X = X0 + 0.01 * rng.normal(size=X0.shape)
    U = X[:, 12 * (N + 1):].reshape(B, N, 24)      # (a copy: U is column-major 24 x N per member)
    U[:, :, 12:] = np.tile([3.0, -2.0, 25.0], 4) + 5 * rng.normal(size=(B, N, 12))
    X[:, 12 * (N + 1):] = U.reshape(B, 24 * N)
    o = Pm.param_offsets(N)["dt"]
    for b in range(B):
        P[b, o:o + N] = rng.permutation(P[b, o:o + N])      # a time grid of its own per member
    status = np.zeros(B, np.int32); status[[3, 64]] = 1
    f64 = dict(device="cuda", dtype=torch.float64)
    p, x, st = torch.tensor(P, **f64), torch.tensor(X, **f64), torch.tensor(status, device="cuda")
    g = _gains(L, B, n, x, p, dt_r, False, st)
    assert np.isfinite(g["K"]).all() and not g["K"][3].any() and not g["xref"][64].any() and g["K"][2].any()
    for b in range(B):
        a = _gains(L, 1, n, x[b:b + 1], p[b:b + 1], dt_r, False, st[b:b + 1])
        for k, v in a.items():
            assert np.array_equal(v[0], g[k][b]), (b, k)
    L.close()


def test_receding_horizon_tracking_gains():
    """mpc.RecedingHorizon.tracking_gains: the gains of the current plan = landing_tracking_gains_batch on the loop's own tensors"""
    import torch
    capi, Pm, mpc = lc("capi"), lc("problem"), lc("mpc")
    N, B, dt_r, n = 40, 6, 0.022, 28
    L = capi.LandingLib(N, device=0)
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=4)
    ctl = mpc.RecedingHorizon(L, P, X0)
    Ib, mass, Q, R, F = _weights()
    K, Pr = ctl.tracking_gains(dt_r, n, weights=(Q, np.diag(R), F), Ib=Ib, mass=mass, want_P=True)
    torch.cuda.synchronize()
    assert (ctl.status.cpu().numpy() == 0).all()
    g = _gains(L, B, n, ctl.x, ctl.p, dt_r, False, ctl.status)
    assert K.shape == (B, n, 12, 24) and np.array_equal(K.cpu().numpy(), g["K"]) and np.array_equal(Pr.cpu().numpy(), g["P"]) and g["K"].any()
    K2 = ctl.tracking_gains(dt_r, n, weights=(Q, np.diag(R), F))      # the robot's own inertia and mass
    torch.cuda.synchronize()
    assert np.isfinite(K2.cpu().numpy()).all()
    L.close()
