"""CPU tests of the actuator audit (include/landing_nlp.h landing_actuator_*, landing_pipeline_screened_pairs_batch; kernel csrc/actuator_kernels.hip) on the
host emulation of the same sources (tests/emu; emulated device pointers are host pointers), against tests/actuator_reference.py: the numpy restatement of
utilities_landing/plot_results.m:12-39 and of the header's summary / where / ok rules."""
import ctypes as C
import os

import numpy as np
import pytest

import actuator_reference as ar
from conftest import GOLDEN, ROOT, lc
from emu_support import emu_landing_lib
from header_decls import _header_fields

_libs = {}


@pytest.fixture(scope="module")
def emu():
    """N -> (LandingLib, Rbd) on the emulation, one context per horizon"""
    def get(N):
        if N not in _libs:
            L = emu_landing_lib(N)
            _libs[N] = (L, lc("rbd").Rbd(L))
        return _libs[N]
    yield get
    for L, _ in _libs.values():
        L.close()
    _libs.clear()


def _a(v):
    return v.ctypes.data      # (an emulated device pointer)


def audit_device(R, x, dt, stride, screen=None, full=True, model=None):
    """landing_actuator_audit_batch on (emulated) device arrays -> dict like actuator_reference.audit"""
    B, N = x.shape[0], R.L.N
    mk = lambda: np.full((B, N, 12), np.nan) if full else None
    out = dict(tau=mk(), jvel=mk(), volt=mk(), summary=np.full((B, 8), np.nan), where=np.full((B, 4), -9, np.int32), ok=np.full(B, -9, np.int32))
    p = lambda k: _a(out[k]) if out[k] is not None else 0
    R.actuator_audit_device(B, _a(dt), stride, _a(x), p("summary"), p("where"), p("ok"), model=model, screen=screen, d_tau=p("tau"), d_jvel=p("jvel"), d_volt=p("volt"))
    return out


@pytest.fixture(scope="module")
def stored():
    x = ar.stored_solutions(GOLDEN)
    return x, ar.audit(20, x, ar.PRODUCTION_DT), ar.audit(20, x, ar.PRODUCTION_DT, screen=dict(drive_only=0))


def test_stored_solutions_against_the_reference(emu, stored):
    """the seven stored solutions on the production grid: tau, jvel, volt to 1e-12, counts and where equal; volt_max 24 on every sample keeps only
    n1_kd_solved[2]; the default screen (positive-work samples) keeps a, m, g, n1_kd_solved[1] and [2] -- the sets asserted from the reference module"""
    L, R = emu(20)
    x, ref, ref_all = stored
    got = audit_device(R, x, ar.PRODUCTION_DT, 0)
    ar.assert_matches(got, ref)
    got_all = audit_device(R, x, ar.PRODUCTION_DT, 0, screen=R.actuator_screen(drive_only=0))
    ar.assert_matches(got_all, ref_all)
    names = np.array(ar.STORED)
    assert list(names[ref_all["ok"] == 1]) == ["kd2"] and list(names[got_all["ok"] == 1]) == ["kd2"]
    assert list(names[ref["ok"] == 1]) == ["a", "m", "g", "kd1", "kd2"] and list(names[got["ok"] == 1]) == ["a", "m", "g", "kd1", "kd2"]
    assert (ref["summary"][ref["ok"] == 1, 3] <= 24.0).all() and (ref["summary"][ref["ok"] == 0, 3] > 24.0).all()


@pytest.mark.parametrize("N", [2, 3, 20, 64])
@pytest.mark.parametrize("grid", ["B1", "rows", "shared"])
def test_small_shapes_against_the_reference(emu, N, grid):
    """N = 2 (one non-zero velocity column), 3, 20, 64 (every thread of the workgroup has an item); B = 1, and B = 3 with three different
    non-uniform dt rows (stride N) and with one shared row (stride 0); random states with pitch up to +-60 deg, forces of both signs"""
    L, R = emu(N)
    B = 1 if grid == "B1" else 3
    x = ar.random_states(N, B, seed=100 + N)
    dt = ar.random_dt(N, B, seed=N)
    if grid == "shared":
        dt = dt[1].copy()
    ref = ar.audit(N, x, dt)
    got = audit_device(R, x, dt, N if dt.ndim == 2 else 0)
    ar.assert_matches(got, ref)
    assert (got["jvel"][:, N - 1] == 0).all() and (got["jvel"][:, :N - 1] != 0).all()


def test_torques_equal_the_kinodynamic_rows(emu):
    """tau of the audit = tau of landing_kinodyn_rows_batch for the same points, to 1e-12: one formula in two kernels"""
    N, B = 20, 3
    L, R = emu(N)
    x = ar.random_states(N, B, seed=7)
    got = audit_device(R, x, ar.PRODUCTION_DT, 0)
    q6, jp, f = [], [], []
    for b in range(B):
        X, J, U = ar.split(N, x[b])
        q6.append(X[:6, :N].T); jp.append(J.T); f.append(U[12:].T)
    q6, jp, f = [np.ascontiguousarray(np.concatenate(v)) for v in (q6, jp, f)]
    tau = np.full((B * N, 12), np.nan)
    R.kinodyn_rows(B * N, _a(q6), 0, _a(f), _a(jp), d_tau=_a(tau))
    assert np.abs(tau.reshape(B, N, 12) - got["tau"]).max() <= 1e-12 * max(1.0, np.abs(tau).max())


def _still(N, B=1):
    """members at rest: level, every leg at the guess pose, zero forces"""
    X = np.zeros((12, N + 1)); J = np.tile(np.tile([0.0, -np.pi / 4, np.pi / 2], 4)[:, None], (1, N)); U = np.zeros((24, N))
    return np.array([ar.pack(X, J, U) for _ in range(B)])


def test_zero_forces_and_exact_tie(emu):
    """zero forces: no sample does positive work -- entry 4 is 0, its where is -1, count 8 is 0; two joints with the same gear ratio moving at the same
    rate under zero force are an exact tie of the voltage peak: where is the lower 12 knot + joint"""
    N = 3
    L, R = emu(N)
    x = _still(N)
    nX = 12 * (N + 1)
    dt = np.array([0.05, 0.05, 0.05])
    for joint in (10, 4, 1):      # hip of leg 3, hip of leg 1, hip of leg 0 move by the same angle over interval 1 (gear ratio 6 each); set out of order
        x[0, nX + 12 * 2 + joint] += 0.125
    ref = ar.audit(N, x, dt)
    got = audit_device(R, x, dt, 0)
    ar.assert_matches(got, ref)
    assert got["summary"][0, 3] == 0.0 and list(got["where"][0, 2:]) == [-1, -1] and got["summary"][0, 7] == 0.0
    assert got["volt"][0, 1, 1] == got["volt"][0, 1, 4] == got["volt"][0, 1, 10] == got["summary"][0, 2] != 0.0
    assert list(got["where"][0, :2]) == [1, 1]
    assert got["summary"][0, 4] == 0.0 and got["summary"][0, 5] == 0.0 and (got["tau"] == 0).all()


def test_nan_member_is_rejected_and_the_others_do_not_see_it(emu):
    """a NaN in one member of three: that member is not ok; the other two are bit-identical to auditing them alone"""
    N = 20
    L, R = emu(N)
    x = ar.random_states(N, 3, seed=11)
    big = R.actuator_screen(volt_max=1e9)
    for where in (0, 12 * (N + 1) + 40, 12 * (N + 1) + 12 * N + 24 * 3 + 14):      # a position the audit does not use, a joint angle, a force
        xn = x.copy(); xn[1, where] = np.nan
        got = audit_device(R, xn, ar.PRODUCTION_DT, 0, screen=big)
        assert list(got["ok"]) == [1, 0, 1]
        for b in (0, 2):
            alone = audit_device(R, np.ascontiguousarray(x[b:b + 1]), ar.PRODUCTION_DT, 0, screen=big)
            for k in alone:
                assert np.array_equal(got[k][b], alone[k][0]), k
    dtn = np.tile(ar.PRODUCTION_DT, (3, 1)); dtn[2, 19] = np.nan      # (the last interval's dt divides nothing: the member is refused all the same)
    assert list(audit_device(R, x, dtn, N, screen=big)["ok"]) == [1, 1, 0]


def test_screen_limits(emu, stored):
    """drive_only switches which peak volt_max sees; tau_ratio_max and jvel_max each reject a member the voltage passes; a limit <= 0 is off"""
    L, R = emu(20)
    x, ref, _ = stored
    s = ref["summary"]
    m = list(ar.STORED).index("m")      # peak 40.2 V, 23.1 V where the motor does positive work
    one = np.ascontiguousarray(x[m:m + 1])
    ok = lambda **kw: int(audit_device(R, one, ar.PRODUCTION_DT, 0, screen=R.actuator_screen(**kw), full=False)["ok"][0])
    assert s[m, 3] < 24.0 < s[m, 2]
    assert ok() == 1 and ok(drive_only=0) == 0 and ok(drive_only=0, volt_max=41.0) == 1 and ok(volt_max=23.0) == 0
    assert ok(tau_ratio_max=1.0) == 1 and ok(tau_ratio_max=0.99) == 0 and ok(volt_max=0.0, tau_ratio_max=0.99) == 0      # (s[m, 0] = 0.994)
    assert ok(jvel_max=44.0) == 1 and ok(jvel_max=43.0) == 0 and ok(volt_max=-1.0, jvel_max=43.0) == 0                   # (s[m, 1] = 43.4)
    assert ok(volt_max=0.0, drive_only=0) == 1      # every limit off
    for kw in (dict(drive_only=0), dict(volt_max=30.0), dict(tau_ratio_max=0.9), dict(jvel_max=40.0, volt_max=0.0)):
        got = audit_device(R, x, ar.PRODUCTION_DT, 0, screen=R.actuator_screen(**kw), full=False)
        assert np.array_equal(got["ok"], ar.audit(20, x, ar.PRODUCTION_DT, screen=kw)["ok"]), kw


def test_actuator_model_argument(emu):
    """a model of the caller's replaces the Mini-Cheetah values (volt and the torque ratio follow it; tau and jvel do not)"""
    N = 3
    L, R = emu(N)
    x, dt = ar.random_states(N, 2, seed=3), ar.random_dt(N, 2, seed=4)
    m = R.actuator_model()
    assert list(m.gr) == [6.0, 6.0, 9.33] and list(m.kt) == [0.05] * 3 and list(m.Rm) == [0.173] * 3 and list(m.tau_max) == list(ar.TAU_MAX) and m.battery_v == 24.0
    gr, kt, Rm, tm = np.array([5.0, 7.0, 8.5]), np.array([0.04, 0.05, 0.06]), np.array([0.2, 0.173, 0.15]), np.array([10.0, 20.0, 30.0])
    for i in range(3):
        m.gr[i], m.kt[i], m.Rm[i], m.tau_max[i] = gr[i], kt[i], Rm[i], tm[i]
    m.battery_v = 12.0
    ar.assert_matches(audit_device(R, x, dt, N, model=m), ar.audit(N, x, dt, gr=gr, kt=kt, Rm=Rm, tau_max=tm, battery_v=12.0))


def test_optional_outputs_empty_batch_and_host_form(emu):
    """tau / jvel / volt NULL leaves the rest unchanged; B = 0 returns 0 and writes nothing; landing_actuator_audit_host equals the device form bit
    for bit, with one grid and with a grid per member"""
    N = 20
    L, R = emu(N)
    x, dt = ar.random_states(N, 3, seed=5), ar.random_dt(N, 3, seed=6)
    full = audit_device(R, x, dt, N)
    bare = audit_device(R, x, dt, N, full=False)
    for k in ("summary", "where", "ok"):
        assert np.array_equal(full[k], bare[k])
    s = np.full((1, 8), np.nan)
    assert L.lib.landing_actuator_audit_batch(L.ctx, 0, None, 0, None, None, None, None, None, None, _a(s), None, None, None) == 0 and np.isnan(s).all()
    assert L.lib.landing_actuator_audit_host(L.ctx, 0, None, 0, None, None, None, None, None, None, None, None, None) == 0
    host = R.actuator_audit(x, dt)
    for k in full:
        assert np.array_equal(host[k], full[k]), k
    host1 = R.actuator_audit(x, dt[0], full=False)
    dev1 = audit_device(R, x, np.ascontiguousarray(dt[0]), 0)
    assert set(host1) == {"summary", "where", "ok"}
    for k in host1:
        assert np.array_equal(host1[k], dev1[k]), k


def test_argument_errors(emu):
    """every LANDING_E_ARG case of the header: NULL pointers, a dt_stride that is neither 0 nor >= N, N outside 2 .. 64, a context without a model"""
    N = 20
    L, R = emu(N)
    capi, rbd = lc("capi"), lc("rbd")
    x, dt = ar.random_states(N, 2, seed=1), ar.random_dt(N, 2, seed=2)
    s, w, ok = np.zeros((2, 8)), np.zeros((2, 4), np.int32), np.zeros(2, np.int32)
    good = [_a(dt), N, _a(x), None, None, None, None, None, _a(s), _a(w), _a(ok), None]
    call = lambda a, lib=L: lib.lib.landing_actuator_audit_batch(lib.ctx, 2, *a)
    assert call(good) == 0
    for i in (0, 2, 8, 9, 10):
        bad = list(good); bad[i] = None
        assert call(bad) == -1 and b"bad argument" in L.lib.landing_last_error(), i
    assert L.lib.landing_actuator_audit_batch(L.ctx, -1, *good) == -1
    assert L.lib.landing_actuator_audit_batch(None, 2, *good) == -1
    for stride in (1, N - 1, -N):
        bad = list(good); bad[1] = stride
        assert call(bad) == -1 and b"dt_stride" in L.lib.landing_last_error(), stride
    big = list(good); big[1] = N + 5      # (a wider row is fine)
    wide = np.zeros((2, N + 5)); wide[:, :N] = dt; big[0] = _a(wide)
    s2 = np.zeros((2, 8)); big[8] = _a(s2)
    assert call(big) == 0 and np.array_equal(s2, s)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    h = lambda v: v.ctypes.data_as(dp)
    assert L.lib.landing_actuator_audit_host(L.ctx, 2, h(dt), 3, h(x), None, None, None, None, None, h(s), w.ctypes.data_as(ip), ok.ctypes.data_as(ip)) == -1
    assert L.lib.landing_actuator_audit_host(L.ctx, 2, h(dt), N, h(x), None, None, None, None, None, None, w.ctypes.data_as(ip), ok.ctypes.data_as(ip)) == -1
    L2 = emu_landing_lib(N)      # no model
    assert call(good, L2) == -1 and b"no model" in L2.lib.landing_last_error()
    L2.close()
    L3 = emu_landing_lib(65)
    rbd.Rbd(L3)
    assert call(good, L3) == -1 and b"N <= 64" in L3.lib.landing_last_error()
    L3.close()
    L4 = emu_landing_lib(N)      # a tree whose legs are not numbered the quadruped's way: refused as the pipeline refuses it
    M = rbd.quad3d_model(); M.parent[7] = 6
    rbd.Rbd(L4, model=M)
    assert call(good, L4) == -1 and b"legs" in L4.lib.landing_last_error()
    L4.close()
    with pytest.raises(RuntimeError, match="dt_stride"):
        R.actuator_audit_device(2, _a(dt), 3, _a(x), _a(s), _a(w), _a(ok))


def _screened(R, P, x, st3, screen):
    B, nxk = x.shape[0], x.shape[1]
    o = dict(summary=np.full((B, 8), np.nan), where=np.full((B, 4), -9, np.int32), ok=np.full(B, -9, np.int32), pin=np.full((B, 9), np.nan),
             pout=np.full((B, nxk), np.nan), index=np.full(B, -9, np.int32), count=np.full(1, -9, np.int32))
    R.screened_pairs(B, _a(P), _a(x), _a(st3), _a(o["summary"]), _a(o["where"]), _a(o["ok"]), _a(o["pin"]), _a(o["pout"]), _a(o["index"]), _a(o["count"]), screen=screen)
    return o


def _pairs(R, P, x, fin):
    B, nxk = x.shape[0], x.shape[1]
    o = dict(pin=np.full((B, 9), np.nan), pout=np.full((B, nxk), np.nan), index=np.full(B, -9, np.int32), count=np.full(1, -9, np.int32))
    R.training_pairs_device(B, _a(P), _a(x), _a(fin), _a(o["pin"]), _a(o["pout"]), _a(o["index"]), _a(o["count"]))
    return o


def test_screened_pairs_against_the_unscreened_writer(emu, stored):
    """landing_pipeline_screened_pairs_batch on synthetic status rows covering every branch of the final-status rule (no re-solve, re-solve converged,
    only the refinement converged, neither): pairs, index and count bit-identical to landing_training_pairs_batch fed the final status with the rejected
    members masked out; the audit is the stand-alone audit with dt from p; a screen that rejects nobody gives the unscreened output, one that rejects
    everybody gives count 0"""
    N = 20
    L, R = emu(N)
    Pm, pl = lc("problem"), lc("pipeline")
    xs, _, _ = stored
    rows = [(0, 0, -1), (0, 3, -1), (0, 1, 0), (0, 0, 0), (0, 0, 2), (0, 0, 4), (0, 1, 2), (0, 3, 4), (0, 4, 0), (0, 2, -1)]
    B = 3 * len(rows)      # every status row meets members the default screen keeps and members it rejects
    st3 = np.array([rows[b % len(rows)] for b in range(B)], np.int32)
    x = np.ascontiguousarray(np.array([xs[(b // 2) % 7] for b in range(B)]))
    P, _, _, _ = Pm.make_batch(B, N, 0.6, seed=3, consts=Pm.production_constants("main"), dt_grid="reference")
    fin = pl.final_status(st3)
    assert np.array_equal(fin, [L.lib.landing_pipeline_final_status(int(a), int(b)) for _, a, b in st3])
    ref = ar.audit(N, x, ar.PRODUCTION_DT)
    assert 0 < ((fin == 0) & (ref["ok"] == 0)).sum() and 0 < ((fin == 0) & (ref["ok"] == 1)).sum() and 0 < ((fin != 0) & (ref["ok"] == 1)).sum()
    got = _screened(R, P, x, st3, None)
    ar.assert_matches(got, ref)
    alone = audit_device(R, x, ar.PRODUCTION_DT, 0, full=False)
    for k in ("summary", "where", "ok"):
        assert np.array_equal(got[k], alone[k]), k
    masked = np.where((fin == 0) & (ref["ok"] == 0), 1, fin).astype(np.int32)
    want = _pairs(R, P, x, masked)
    M = int(want["count"][0])
    assert M == int(((fin == 0) & (ref["ok"] == 1)).sum())
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    nobody = _screened(R, P, x, st3, R.actuator_screen(volt_max=1e9))
    plain = _pairs(R, P, x, fin)
    assert nobody["ok"].all()
    for k in plain:
        assert np.array_equal(nobody[k], plain[k], equal_nan=True), k
    everybody = _screened(R, P, x, st3, R.actuator_screen(volt_max=1e-3))
    assert everybody["count"][0] == 0 and (everybody["index"] == -1).all() and not everybody["ok"].any() and np.isnan(everybody["pout"]).all()
    # arguments: B = 0 writes a zero count; NULL pointers and a context without a model are refused
    cnt = np.full(1, -9, np.int32)
    fn = L.lib.landing_pipeline_screened_pairs_batch
    a = [_a(P), _a(x), _a(st3), None, None, _a(got["summary"]), _a(got["where"]), _a(got["ok"]), _a(got["pin"]), _a(got["pout"]), _a(got["index"]), _a(cnt), None]
    assert fn(L.ctx, 0, *a) == 0 and cnt[0] == 0
    for i in (0, 1, 2, 5, 6, 7, 8, 9, 10, 11):
        bad = list(a); bad[i] = None
        assert fn(L.ctx, B, *bad) == -1, i
    L2 = emu_landing_lib(N)
    assert fn(L2.ctx, B, *a) == -1 and b"no model" in L2.lib.landing_last_error()
    L2.close()


def test_header_structs_equal_the_ctypes_mirrors(emu):
    """landing_actuator_model / landing_actuator_screen of the header, field for field, against capi.ActuatorModel / ActuatorScreen; the defaults as
    stated; LANDING_AUDIT_NSUM against the mirror's"""
    L, R = emu(20)
    capi = lc("capi")
    assert _header_fields("landing_actuator_model") == [f[0] for f in capi.ActuatorModel._fields_]
    assert _header_fields("landing_actuator_screen") == [f[0] for f in capi.ActuatorScreen._fields_]
    assert C.sizeof(capi.ActuatorModel) == 13 * 8 and C.sizeof(capi.ActuatorScreen) == 32
    s = R.actuator_screen()
    assert (s.volt_max, s.tau_ratio_max, s.jvel_max, s.drive_only) == (24.0, 0.0, 0.0, 1)
    src = open(os.path.join(ROOT, "include", "landing_nlp.h")).read()
    assert "#define LANDING_AUDIT_NSUM %d\n" % capi.AUDIT_NSUM in src and len(capi.AUDIT_SUMMARY) == capi.AUDIT_NSUM == len(ar.SUMMARY)
    with pytest.raises(TypeError):
        R.actuator_screen(volts=1.0)


def test_member_log_takes_per_member_columns(tmp_path):
    """dataset.write_member_log: an entry of extra= with one value per member lands in that member's record; scalars go to every record as before"""
    import json
    ds = lc("dataset")
    path = str(tmp_path / "log.jsonl")
    ds.write_member_log(path, [0, 3], [5, 6], np.zeros((2, 3)), extra={"batch": 4, "volt": np.array([1.5, 2.5]), "ok": np.array([1, 0], np.int32)})
    recs = [json.loads(l) for l in open(path)]
    assert [r["volt"] for r in recs] == [1.5, 2.5] and [r["ok"] for r in recs] == [1, 0] and [r["batch"] for r in recs] == [4, 4]


@pytest.mark.parametrize("case", ["stored", "n2", "n3", "n20", "n64"])
def test_recorded_emulation_outputs_are_current(emu, case):
    """tests/golden/actuator_audit_emu.npz (what the GPU suite holds the product library against) is bit for bit what the emulation gives today, and
    agrees with the reference module"""
    import make_golden_actuator as mg
    emu(mg.CASES[case])      # (builds the emulation)
    now = mg.emulation_outputs(case, GOLDEN)
    with np.load(os.path.join(GOLDEN, "actuator_audit_emu.npz")) as d:
        for k, v in now.items():
            assert np.array_equal(d[case + "_" + k], v), k
    N, x, dt, _ = mg.case_inputs(case, GOLDEN)
    ar.assert_matches(now, ar.audit(N, x, dt))
