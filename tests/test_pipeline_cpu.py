"""CPU tests of the drop-state chain (include/landing_nlp.h landing_pipeline_*, kernels csrc/pipeline_kernels.hip) on the host emulation of the same
sources (tests/emu; emulated device pointers are host pointers): the pose kernel against the host mirror (kinodyn.bounds / c_init_of / kin_box_of), the
pairs kernel against dataset.training_pairs, the select rule, the plumbing and argument checks of landing_pipeline_batch, the header's options struct
against its ctypes mirror, and the MATLAB gateway compiled against tests/stubs/mex.h."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import lc
from emu_support import EMU_LIB as EMU, build_emu, compile_mex_gateway, emu_landing_lib
from header_decls import _header_fields

N = 20


@pytest.fixture(scope="module")
def emu():
    L = emu_landing_lib(N)
    yield L, lc("rbd").Rbd(L)
    L.close()


def _a(v):
    return v.ctypes.data      # (an emulated device pointer)


def _mirror(P, xs, N):
    """the refinement problem of every member from the host mirror, every value taken from the member's p; kin_box_y0 = 0.125
    (generate_landingCtrller_KNITRO.m:154, landing_kinodyn_form_knitro)"""
    kd, o = lc("kinodyn"), lc("problem").param_offsets(N)
    out = []
    for b in range(P.shape[0]):
        p = P[b]
        six = lambda n: p[o[n]:o[n] + 6]
        q, qd = six("q_init"), six("qd_init")
        lb, ub = kd.bounds(N, q, qd, kd.c_init_of(q), kd.kin_box_of(q[3:6], qd[3:6]), q_term_min=six("q_term_min"), q_term_max=six("q_term_max"),
                           qd_term_min=six("qd_term_min"), qd_term_max=six("qd_term_max"), z_min=p[o["q_min"] + 2], l_leg_max=p[o["l_leg_max"]], kin_box_y0=0.125)
        cost = np.concatenate([p[o["QN"]:o["QN"] + 12], p[12 * N:12 * N + 12]])
        out.append((lb, ub, cost, kd.member_problem(N, q, qd, xs[b])[3]))
    return [np.array([m[i] for m in out]) for i in range(4)]


def trig_rows(N):
    """rows of lbg / ubg whose value passes through sin / cos: c_init (12-23) and the kinematic box's x / y rows of every leg and interval"""
    rows = list(range(12, 24))
    for k in range(N):
        last = k == N - 1
        S, o = (9, 2) if last else (15, 8)
        for leg in range(4):
            r = 48 + 141 * k + 16 + S * leg + o
            rows += [r, r + 1]
    return np.array(rows)


def pose(R, P, xs, opts=None):
    kd = lc("kinodyn")
    B = P.shape[0]
    nx, ng = kd.dims(N)
    lb, ub, cost, x0 = np.full((B, ng), np.nan), np.full((B, ng), np.nan), np.full((B, 24), np.nan), np.full((B, nx), np.nan)
    R.kinodyn_pose_device(B, _a(P), _a(xs), _a(lb), _a(ub), _a(cost), _a(x0), opts)
    return lb, ub, cost, x0


@pytest.mark.parametrize("law", ["main", "datagen"])
def test_pose_kernel_equals_the_host_mirror(emu, law):
    """256 members of each sampling law, production grid, random SRBM-shaped x: x0 and cost bit-equal; lbg / ubg bit-equal except on the rows
    that pass through sin / cos (c_init, the kinematic box), which agree to 4 ulp"""
    L, R = emu
    Pm = lc("problem")
    B = 256
    P, _, _, _ = Pm.make_batch(B, N, 0.6, seed=20211, consts=Pm.production_constants(law), dt_grid="reference", law=law)
    xs = np.random.default_rng(5).normal(size=(B, Pm.nx(N)))
    lb, ub, cost, x0 = pose(R, P, xs)
    mlb, mub, mcost, mx0 = _mirror(P, xs, N)
    assert np.array_equal(x0, mx0) and np.array_equal(cost, mcost)
    t = trig_rows(N)
    rest = np.setdiff1d(np.arange(lb.shape[1]), t)
    assert np.array_equal(lb[:, rest], mlb[:, rest]) and np.array_equal(ub[:, rest], mub[:, rest])
    assert_trig_rows_close(lb[:, t], mlb[:, t]); assert_trig_rows_close(ub[:, t], mub[:, t])


def assert_trig_rows_close(got, ref):
    """within 4 ulp at the scale of the rows' terms: a foot position under the hip is q + R (+-0.2, +-0.15, -0.3), whose lateral coordinates cancel
    to a few millimetres (measured: 1 ulp of 0.5 = 57 ulp of -1.3e-3 between the emulated kernel and numpy's matrix products), so the ulp is taken
    at max(|value|, 0.5)"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin)
    ulp = np.abs(got[fin] - ref[fin]) / np.spacing(np.maximum(np.abs(ref[fin]), 0.5))
    assert ulp.max() <= 4, ulp.max()


def test_pairs_kernel_equals_training_pairs(emu):
    """mixed final statuses (3 and 4 among them), 300 members (more than one per scan thread): columns, order, count and index bit-equal to
    dataset.training_pairs(..., jpos_star=...)"""
    L, R = emu
    Pm, ds, kd = lc("problem"), lc("dataset"), lc("kinodyn")
    B = 300
    P, _, q, qd = Pm.make_batch(B, N, 0.6, seed=3, consts=Pm.production_constants("main"), dt_grid="reference")
    nxk = kd.dims(N)[0]
    rng = np.random.default_rng(9)
    x = rng.normal(size=(B, nxk))
    status = rng.choice([0, 0, 0, 1, 2, 3, 4], size=B).astype(np.int32)
    din, dout = np.full((B, 9), np.nan), np.full((B, nxk), np.nan)
    idx, cnt = np.full(B, -7, np.int32), np.full(1, -7, np.int32)
    R.training_pairs_device(B, _a(P), _a(x), _a(status), _a(din), _a(dout), _a(idx), _a(cnt))
    nX = 12 * (N + 1)
    inp, out = ds.training_pairs(N, q, qd, np.concatenate([x[:, :nX], x[:, nX + 12 * N:]], axis=1), status, jpos_star=x[:, nX:nX + 12 * N])
    M = int((status == 0).sum())
    assert cnt[0] == M and 0 < M < B and inp.shape == (9, M) and out.shape == (nxk, M)
    assert np.array_equal(idx[:M], np.nonzero(status == 0)[0]) and (idx[M:] == -1).all()
    assert np.array_equal(din[:M].T, inp) and np.array_equal(dout[:M].T, out)
    assert np.isnan(din[M:]).all() and np.isnan(dout[M:]).all()      # only the first `count` columns are written


def test_select_rule(emu):
    """the final status of a member (landing_pipeline_final_status = the select kernel's rule), all four cases, and its numpy mirror"""
    L, _ = emu
    pl = lc("pipeline")
    fs = L.lib.landing_pipeline_final_status
    assert fs(1, 0) == 0 and fs(4, 0) == 0            # warm re-solve converged: its result
    assert fs(0, 1) == 0 and fs(0, 4) == 0            # re-solve undecided, refinement converged: the refinement's (a KKT point of the same NLP)
    assert fs(1, 2) == 2 and fs(3, 4) == 4            # both undecided: the re-solve's
    assert fs(3, -1) == 3 and fs(0, -1) == 0          # no re-solve: the refinement's
    st = np.array([[0, s1, s2] for s1 in range(5) for s2 in range(-1, 5)], np.int32)
    assert np.array_equal(pl.final_status(st), [fs(int(a), int(b)) for _, a, b in st])


def _chain(L, R, P, X0, opts, n=None):
    kd = lc("kinodyn")
    B = P.shape[0]
    nxk, ng = kd.dims(L.N)
    out = dict(x=np.full((B, nxk), np.nan), f=np.full(B, np.nan), lam_g=np.full((B, ng), np.nan), status=np.full((B, 3), -9, np.int32),
               iters=np.full((B, 3), -9, np.int32), kkt=np.full((B, 3), np.nan), pin=np.full((B, 9), np.nan), pout=np.full((B, nxk), np.nan),
               index=np.full(B, -9, np.int32), count=np.full(1, -9, np.int32), xs=np.full((B, L.nx), np.nan))
    a = {k: _a(v) for k, v in out.items()}
    R.pipeline_device(B, _a(P), _a(X0), opts, a["x"], a["f"], a["status"], a["iters"], a["kkt"], a["lam_g"], a["pin"], a["pout"], a["index"], a["count"], a["xs"])
    return out


def test_pipeline_batch_plumbing_on_the_emulation():
    """landing_pipeline_batch at N = 3, B = 2, two iterations per pass: every column of status / iters is filled, the count matches the final statuses,
    warm = 0 leaves the re-solve column at -1 / 0; LANDING_E_ARG for mixed dt, N > 64, a context without a model and the N=41 script's context"""
    build_emu()
    capi, rbd, Pm, pl = lc("capi"), lc("rbd"), lc("problem"), lc("pipeline")
    n = 3
    L = capi.LandingLib(n, lib_path=EMU)
    R = rbd.Rbd(L)
    P, X0, _, _ = Pm.make_batch(2, n, 0.6, seed=5)
    o = R.pipeline_opts()
    o.srbm.max_iter = o.refine.max_iter = o.resolve.max_iter = 2
    r = _chain(L, R, P, X0, o)
    st, it = r["status"], r["iters"]
    assert np.isin(st, (0, 1, 2, 3, 4)).all() and (it >= 0).all() and (it[:, 0] >= 1).all(), (st, it)      # (the -9 the arrays were filled with is gone)
    assert np.isfinite(r["x"]).all() and np.isfinite(r["f"]).all() and np.isfinite(r["kkt"]).all() and np.isfinite(r["xs"]).all()
    fin = pl.final_status(st)
    M = int((fin == 0).sum())
    assert r["count"][0] == M and np.array_equal(r["index"][:M], np.nonzero(fin == 0)[0]) and (r["index"][M:] == -1).all()
    o.warm = 0
    r0 = _chain(L, R, P, X0, o)
    assert (r0["status"][:, 2] == -1).all() and (r0["iters"][:, 2] == 0).all()
    assert np.array_equal(r0["status"][:, :2], st[:, :2]) and np.array_equal(r0["iters"][:, :2], it[:, :2])      # (the same first two passes)
    # mixed dt: refused before anything is solved
    P2 = P.copy(); P2[1, Pm.param_offsets(n)["dt"]] += 1e-3
    with pytest.raises(RuntimeError, match="same for every member"):
        _chain(L, R, P2, X0, o)
    # a context without a model
    L2 = capi.LandingLib(n, lib_path=EMU)
    b = [np.zeros(4096) for _ in range(5)]
    rc = L2.lib.landing_pipeline_batch(L2.ctx, 2, _a(P), _a(X0), None, None, _a(b[0]), _a(b[1]), None, _a(b[2]), _a(b[3]), _a(b[4]), None, None, None, None, None)
    assert rc == -1 and b"no model" in L2.lib.landing_last_error()
    L2.close()
    # the N=41 script's parameter vector (run_cost = 2)
    L3 = capi.LandingLib(n, lib_path=EMU, ccc_params=True)
    R3 = rbd.Rbd(L3)
    with pytest.raises(RuntimeError, match="run_cost"):
        R3.pipeline_device(2, _a(P), _a(X0), o, *[_a(np.zeros(4096)) for _ in range(5)])
    L3.close(); L.close()
    # N > 64: the refinement's limit
    L4 = capi.LandingLib(65, lib_path=EMU)
    R4 = rbd.Rbd(L4)
    with pytest.raises(RuntimeError, match="N <= 64"):
        R4.pipeline_device(1, _a(np.zeros(4096)), _a(np.zeros(4096)), None, *[_a(np.zeros(8192)) for _ in range(5)])
    L4.close()


def test_header_options_struct_equals_the_ctypes_mirror(emu):
    """landing_pipeline_opts / landing_kinodyn_form of the header, field for field, against capi.PipelineOpts / KinodynForm; the defaults as stated"""
    L, R = emu
    capi, kd = lc("capi"), lc("kinodyn")
    assert _header_fields("landing_pipeline_opts") == [f[0] for f in capi.PipelineOpts._fields_]
    assert _header_fields("landing_kinodyn_form") == [f[0] for f in capi.KinodynForm._fields_]
    o = R.pipeline_opts()
    assert bytes(o.srbm) == bytes(L.default_opts()) and bytes(o.refine) == bytes(R.kinodyn_default_opts()) and bytes(o.resolve) == bytes(R.kinodyn_warm_opts())
    assert (o.form.kin_box_x0, o.form.kin_box_y0, o.form.comp_eps, o.form.slip_eps, o.form.fk_band) == (0.125, 0.125, 1e-3, 1e-3, 0.01)
    assert list(o.form.tau_max) == list(kd.TAU_MAX)
    assert np.array_equal(list(o.jpos_min), kd.JPOS_MIN) and np.array_equal(list(o.jpos_max), kd.JPOS_MAX)
    assert list(o.jpos_guess) == [0.0, -np.pi / 4, np.pi / 2] and o.warm == 1


class PipelineGateway:
    """matlab/landing_pipeline_mex.c compiled against tests/stubs/mex.h with -Wall -Werror, linked to `lib_dir`/lib`lib_name`.so and called through
    tests/stubs/pipeline_mex_driver.c; call() returns the outputs or raises with the text of mexErrMsgTxt"""

    def __init__(self, tmp_dir, lib_dir, lib_name):
        self.gw = C.CDLL(compile_mex_gateway(tmp_dir, "landing_pipeline_mex.c", "pipeline_mex_driver.c", lib_dir, lib_name))
        self.gw.gateway_error.restype = C.c_char_p

    def call(self, N, args, names, opts=None, nlhs=7, single=()):
        bufs = [np.asfortranarray(np.asarray(args[n], float)) for n in names]
        bufs = [b if b.ndim >= 2 else b.reshape(-1, 1) for b in bufs]
        B = bufs[0].shape[2] if bufs[0].ndim > 2 else 1
        n = len(names)
        dpt = C.POINTER(C.c_double)
        data = (dpt * 21)(*[b.ctypes.data_as(dpt) for b in bufs])
        ndim = (C.c_int * 21)(*[b.ndim for b in bufs])
        dims = (C.c_int * 84)(*sum([list(b.shape) + [1] * (4 - b.ndim) for b in bufs], []))
        cls = (C.c_int * 21)(*[7 if nm in single else 6 for nm in names])
        items = list((opts or {}).items())
        on = (C.c_char_p * max(len(items), 1))(*[k.encode() for k, _ in items]); ov = (C.c_double * max(len(items), 1))(*[float(v) for _, v in items])
        nxk = 48 * N + 12
        X = np.zeros((B, nxk)); F = np.zeros(B); st = np.zeros((B, 3), np.int32); it = np.zeros((B, 3), np.int32); kk = np.zeros((B, 3))
        pin = np.zeros((B, 9)); pout = np.zeros((B, nxk)); kept = C.c_int(-1)
        dp = lambda a: a.ctypes.data_as(dpt); ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
        rc = self.gw.call_pipeline_gateway(n, data, ndim, dims, cls, len(items) if opts is not None else -1, on, ov, nlhs, dp(X), dp(F), ip(st), ip(it), dp(kk),
                                           dp(pin), dp(pout), nxk, B, C.byref(kept))
        if rc == 1:
            raise RuntimeError(self.gw.gateway_error().decode())
        assert rc == 0, "the gateway created an output that was not asked for"
        m = kept.value
        return dict(x=X, f=F, status=st, iters=it, kkt=kk, pair_in=pin[:max(m, 0)].T, pair_out=pout[:max(m, 0)].T, n_kept=m)


def test_pipeline_gateway_compiles_and_refuses_bad_arguments(tmp_path):
    """matlab/landing_pipeline_mex.c compiles against the mex.h stub with -Wall -Werror; its argument errors come back through the stub driver; on the
    emulation (N = 3, B = 2, two iterations per pass) it returns what landing_pipeline_batch returns for the same drop states"""
    build_emu()
    capi, Pm = lc("capi"), lc("problem")
    gw = PipelineGateway(tmp_path, os.path.dirname(EMU), "landing_emu")
    n = 3
    args = Pm.make_args21(2, n, 0.6, seed=5)
    names = capi.ARGS21
    with pytest.raises(RuntimeError, match="21 inputs"):
        gw.call(n, args, names[:20])
    with pytest.raises(RuntimeError, match=r"argument 16 \(mu\) must be a full real double array"):
        gw.call(n, args, names, single=("mu",))
    bad = dict(args); bad["QN"] = np.zeros((11, 2))
    with pytest.raises(RuntimeError, match=r"argument 14 \(QN\) has 22 elements"):
        gw.call(n, bad, names)
    with pytest.raises(RuntimeError, match="at most 7 outputs"):
        gw.call(n, args, names, nlhs=8)
    few = dict(max_iter_srbm=2, max_iter_refine=2, max_iter_resolve=2)
    g = gw.call(n, args, names, opts=few)
    L = capi.LandingLib(n, lib_path=EMU)
    R = lc("rbd").Rbd(L)
    o = R.pipeline_opts()
    o.srbm.max_iter = o.refine.max_iter = o.resolve.max_iter = 2
    P = L.pack_args21(args)
    r = _chain(L, R, P, np.ascontiguousarray(np.asarray(args["x0"]).T), o)
    L.close()
    m = int(r["count"][0])
    assert np.array_equal(g["x"], r["x"]) and np.array_equal(g["status"], r["status"]) and np.array_equal(g["iters"], r["iters"]) and np.array_equal(g["kkt"], r["kkt"])
    assert g["n_kept"] == m and np.array_equal(g["pair_in"], r["pin"][:m].T) and np.array_equal(g["pair_out"], r["pout"][:m].T)
    g1 = gw.call(n, args, names, opts=few, nlhs=1)      # outputs beyond X only when asked for (the driver checks)
    assert np.array_equal(g1["x"], g["x"])
