"""Ownership of device memory in the C ABI (host emulation, no GPU).  The emulation counts the live hipMalloc / hipHostMalloc blocks and can make
the k-th allocation from now fail (tests/emu: hip_emu_live_blocks, hip_emu_fail_alloc).  For each entry point below, on a fresh context:
  * a call that succeeds leaves the count, after landing_destroy, where it was before landing_create -- what a context keeps is freed with it
    (the CasADi face's cache included, without landing_kinodyn_casadi_release);
  * with any one of the call's allocations made to fail, the call returns LANDING_E_HIP and the count still returns to its start."""
import ctypes as C

import numpy as np
import pytest

from conftest import lc
from emu_support import build_emu, emu_landing_lib

LANDING_E_HIP = -2
_dp, _ip, _lp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_longlong)


def _p(a):
    return a.ctypes.data_as(_ip if a.dtype == np.int32 else _dp)


@pytest.fixture(scope="module")
def emu():
    return lc("capi").load(build_emu())      # (the table of capi.py declares every entry point and the emulation's counters)


RC = dict(QX=[1.0] * 12, Qc=[0.1] * 3, Qf=[0.01] * 3)
NS, NK = 4, 2      # horizons of the SRBM and the kinodynamic cases
NG, NP = 6, 3      # ... of the tracking gains and of the drop-state chain (tests/test_gains_chain_cpu.py, tests/test_pipeline_cpu.py)


def _srbm(L):
    P, X0, _, _ = lc("problem").make_batch(2, L.N, 0.6, seed=3)
    return np.ascontiguousarray(P), np.ascontiguousarray(X0)


def _solve_out(L, B):
    return [np.zeros(B * L.nx), np.zeros(B), np.zeros(B * L.ng), np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(3 * B)]


def _opts(o):      # one iteration: the test is about the host side
    o.max_iter = 1; o.feas_phase = 0
    return o


def eval_batch_host(lib, L):
    P, X = _srbm(L)
    out = [np.zeros(2 * n) for n in (1, L.ng, L.nx, L.nnz_jac, L.nnz_hess, L.nx, L.np_)]
    return lib.landing_eval_batch_host(L.ctx, 2, _p(X), _p(P), _p(np.ones(2)), _p(np.ones(2 * L.ng)), *map(_p, out))


def eval_hess_rc_batch_host(lib, L):
    P, X = _srbm(L)
    h = np.zeros(2 * lib.landing_nnz_hess_rc(L.N))
    return lib.landing_eval_hess_rc_batch_host(L.ctx, 2, _p(X), _p(P), _p(np.ones(2)), _p(np.ones(2 * L.ng)), _p(h))


def solve_batch_host(lib, L):
    P, X = _srbm(L)
    return lib.landing_solve_batch_host(L.ctx, 2, _p(P), _p(X), C.byref(_opts(L.default_opts())), *map(_p, _solve_out(L, 2)))


def solve_stream_host(lib, L):      # two chunks of one member on two lanes: a child context per lane beyond the first
    P, X = _srbm(L)
    return lib.landing_solve_stream_host(L.ctx, 2, 1, 2, _p(P), _p(X), C.byref(_opts(L.default_opts())), *map(_p, _solve_out(L, 2)))


def kinodyn_pattern(lib, L):      # the Hessian's: builds the context's pair table on the way (kd_ensure_pairs)
    colind, nnz = np.zeros(48 * NK + 13, np.int64), C.c_longlong()
    return lib.landing_kinodyn_pattern(L.ctx, NK, 1, colind.ctypes.data_as(_lp), None, C.byref(nnz))


def kinodyn_block_nonzeros(lib, L):      # kd_ensure_jpat
    n0, n1 = C.c_int(), C.c_int()
    return lib.landing_kinodyn_block_nonzeros(L.ctx, C.byref(n0), C.byref(n1), None)


def kinodyn_solve_batch_host(lib, L):
    nx, ng = lc("kinodyn").dims(NK)
    prm = lc("rbd").KinodynParams()
    mass, Ib, Ibi = lc("constants").robot_constants()
    for k in range(NK):
        prm.dt[k] = 0.05
    prm.mass, prm.mu = mass, 0.75
    for i in range(3):
        prm.Ib[i], prm.Ib_inv[i] = Ib[i], Ibi[i]
    lb, ub, cost, x0 = -np.ones(ng), np.ones(ng), np.zeros(24), np.zeros(nx)
    o = lc("capi").SolverOpts()
    lib.landing_kinodyn_solver_opts_default(C.byref(o))
    _opts(o)
    out = [np.zeros(nx), np.zeros(1), np.zeros(ng), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(3)]
    return lib.landing_kinodyn_solve_batch_host(L.ctx, 1, NK, C.byref(prm), _p(lb), _p(ub), _p(cost), _p(x0), C.byref(o), *map(_p, out))


def kinodyn_casadi_pattern(lib, L):      # the CasADi face builds its cache in the context; no landing_kinodyn_casadi_release before landing_destroy
    ci, r, nnz = _lp(), _lp(), C.c_longlong()
    return lib.landing_kinodyn_casadi_pattern(L.ctx, NK, 0, C.byref(ci), C.byref(r), C.byref(nnz))


def tracking_gains_host(lib, L):      # every output and the status mask; the Riccati launch keeps a device block and a pinned one in the context
    P, X = _srbm(L)
    n = 3
    Ib = np.ascontiguousarray(lc("constants").composite_body_inertia()[0:3, 0:3])
    out = [np.zeros(2 * n * k) for k in (576, 288, 576, 288, 24, 12)]
    return lib.landing_tracking_gains_host(L.ctx, 2, _p(X), _p(P), _p(np.zeros(2, np.int32)), 0.03, n, _p(Ib), 8.252, _p(np.eye(24)), _p(np.ones(12)), None, 0,
                                           *map(_p, out))


def pipeline_21(lib, L):      # SRBM solve, refinement and warm re-solve of one iteration each, every output
    capi = lc("capi")
    a, keep, B = capi.matlab_args21(NP, lc("problem").make_args21(2, NP, 0.6, seed=5))
    o = capi.PipelineOpts()
    lib.landing_pipeline_opts_default(C.byref(o))
    for s in (o.srbm, o.refine, o.resolve):
        _opts(s)
    nx, ng = lc("kinodyn").dims(NP)
    out = [np.zeros(B * nx), np.zeros(B), np.zeros(B * ng), np.zeros(3 * B, np.int32), np.zeros(3 * B, np.int32), np.zeros(3 * B), np.zeros(9 * B), np.zeros(B * nx)]
    return lib.landing_pipeline_21(L.ctx, B, *[getattr(a, n) for n in capi.ARGS21], C.byref(o), *map(_p, out), C.byref(C.c_int()))


CASES = [(eval_batch_host, NS, None), (eval_hess_rc_batch_host, NS, RC), (solve_batch_host, NS, None), (solve_stream_host, NS, None),
         (kinodyn_pattern, NK, None), (kinodyn_block_nonzeros, NK, None), (kinodyn_solve_batch_host, NK, None), (kinodyn_casadi_pattern, NK, None),
         (tracking_gains_host, NG, None), (pipeline_21, NP, None)]


def _run(emu, call, N, run_cost, fail_at):
    """live-block count before the context, rc of the call with allocation `fail_at` failing (0: none), allocations the call made, count after landing_destroy"""
    start = emu.hip_emu_live_blocks()
    L = emu_landing_lib(N, run_cost=run_cost)
    try:
        if N in (NK, NP):
            lc("rbd").Rbd(L)      # (sets the model)
        emu.hip_emu_fail_alloc(fail_at)
        rc = call(emu, L)
    finally:
        n = emu.hip_emu_fail_alloc(0)
        L.close()
    return start, rc, n, emu.hip_emu_live_blocks()


@pytest.mark.parametrize("call,N,run_cost", CASES, ids=[c[0].__name__ for c in CASES])
def test_every_allocation_is_freed_also_when_one_fails(emu, call, N, run_cost):
    start, rc, n, end = _run(emu, call, N, run_cost, 0)
    assert rc == 0, emu.landing_last_error()
    assert n > 0 and end == start, (n, start, end)
    for k in range(1, n + 1):
        start, rc, _, end = _run(emu, call, N, run_cost, k)
        assert rc == LANDING_E_HIP and end == start, (k, n, rc, start, end)
