"""GPU tests of the actuator audit (include/landing_nlp.h landing_actuator_*, landing_pipeline_screened_pairs_batch; kernel csrc/actuator_kernels.hip) with
the product library: the cases of tests/test_actuator_audit_cpu.py against tests/actuator_reference.py on the device, the device against the host
emulation's recorded outputs (tests/golden/actuator_audit_emu.npz, which the CPU suite holds against the emulation), the screened chain
(pipeline.RefineChain(screen=...)) against the unscreened one, and the screened data generation.  Small shapes; the chain cases solve 16 drop states."""
import json

import numpy as np
import pytest

import actuator_reference as ar
from conftest import GOLDEN, lc
from make_golden_actuator import CASES, case_inputs

pytestmark = pytest.mark.gpu
_libs = {}


@pytest.fixture(scope="module")
def gpu():
    """N -> (LandingLib, Rbd) on device 0, one context per horizon"""
    def get(N):
        if N not in _libs:
            L = lc("capi").LandingLib(N, device=0)
            _libs[N] = (L, lc("rbd").Rbd(L))
        return _libs[N]
    yield get
    for L, _ in _libs.values():
        L.close()
    _libs.clear()


def _T(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda")


def audit_device(R, x, dt, stride, screen=None, full=True):
    import torch
    B, N = x.shape[0], R.L.N
    f64, i32 = dict(device="cuda", dtype=torch.float64), dict(device="cuda", dtype=torch.int32)
    mk = lambda: torch.full((B, N, 12), float("nan"), **f64) if full else None
    o = dict(tau=mk(), jvel=mk(), volt=mk(), summary=torch.full((B, 8), float("nan"), **f64), where=torch.full((B, 4), -9, **i32), ok=torch.full((B,), -9, **i32))
    p = lambda k: o[k].data_ptr() if o[k] is not None else 0
    dx, ddt = _T(x), _T(dt)
    R.actuator_audit_device(B, ddt.data_ptr(), stride, dx.data_ptr(), p("summary"), p("where"), p("ok"), screen=screen, d_tau=p("tau"), d_jvel=p("jvel"), d_volt=p("volt"),
                            stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items() if v is not None}


@pytest.fixture(scope="module")
def stored():
    x = ar.stored_solutions(GOLDEN)
    return x, ar.audit(20, x, ar.PRODUCTION_DT), ar.audit(20, x, ar.PRODUCTION_DT, screen=dict(drive_only=0))


def test_stored_solutions_against_the_reference_gpu(gpu, stored):
    """the seven stored solutions on the production grid: values to 1e-12, counts and where equal, the two kept sets as the reference module gives them"""
    L, R = gpu(20)
    x, ref, ref_all = stored
    got = audit_device(R, x, ar.PRODUCTION_DT, 0)
    ar.assert_matches(got, ref)
    got_all = audit_device(R, x, ar.PRODUCTION_DT, 0, screen=R.actuator_screen(drive_only=0))
    ar.assert_matches(got_all, ref_all)
    names = np.array(ar.STORED)
    assert list(names[ref_all["ok"] == 1]) == ["kd2"] and list(names[got_all["ok"] == 1]) == ["kd2"]
    assert list(names[ref["ok"] == 1]) == ["a", "m", "g", "kd1", "kd2"] and list(names[got["ok"] == 1]) == ["a", "m", "g", "kd1", "kd2"]
    host = R.actuator_audit(x, ar.PRODUCTION_DT)      # landing_actuator_audit_host: bit for bit the device form
    for k in got:
        assert np.array_equal(host[k], got[k]), k


@pytest.mark.parametrize("N", [2, 3, 20, 64])
@pytest.mark.parametrize("grid", ["B1", "rows", "shared"])
def test_small_shapes_against_the_reference_gpu(gpu, N, grid):
    L, R = gpu(N)
    B = 1 if grid == "B1" else 3
    x = ar.random_states(N, B, seed=100 + N)
    dt = ar.random_dt(N, B, seed=N)
    if grid == "shared":
        dt = dt[1].copy()
    got = audit_device(R, x, dt, N if dt.ndim == 2 else 0)
    ar.assert_matches(got, ar.audit(N, x, dt))
    assert (got["jvel"][:, N - 1] == 0).all() and (got["jvel"][:, :N - 1] != 0).all()


@pytest.mark.parametrize("case", sorted(CASES))
def test_device_against_the_emulation_gpu(gpu, case):
    """the same inputs through the product library and through the host emulation (recorded): summary counts, where and ok equal; values to 1e-12
    (sincos may differ in the last bit)"""
    N, x, dt, stride = case_inputs(case, GOLDEN)
    L, R = gpu(N)
    got = audit_device(R, x, dt, stride)
    with np.load(GOLDEN + "/actuator_audit_emu.npz") as d:
        emu = {k: d[case + "_" + k] for k in ("tau", "jvel", "volt", "summary", "where", "ok")}
    ar.assert_matches(got, emu)


def test_edge_rules_gpu(gpu, stored):
    """zero forces and the exact tie; a NaN member among three; drive_only, tau_ratio_max and jvel_max each on its own; NULL outputs; B = 0; the refused
    arguments"""
    N = 3
    L, R = gpu(N)
    X = np.zeros((12, N + 1)); J = np.tile(np.tile([0.0, -np.pi / 4, np.pi / 2], 4)[:, None], (1, N)); U = np.zeros((24, N))
    x = ar.pack(X, J, U)[None, :].copy()
    for joint in (10, 4, 1):
        x[0, 12 * (N + 1) + 12 * 2 + joint] += 0.125
    dt = np.array([0.05, 0.05, 0.05])
    got = audit_device(R, x, dt, 0)
    ar.assert_matches(got, ar.audit(N, x, dt))
    assert got["summary"][0, 3] == 0.0 and list(got["where"][0]) == [1, 1, -1, -1] and got["summary"][0, 7] == 0.0
    assert got["volt"][0, 1, 1] == got["volt"][0, 1, 4] == got["volt"][0, 1, 10] == got["summary"][0, 2] != 0.0
    L, R = gpu(20)
    xr = ar.random_states(20, 3, seed=11)
    big = R.actuator_screen(volt_max=1e9)
    xn = xr.copy(); xn[1, 12 * 21 + 40] = np.nan
    gn = audit_device(R, xn, ar.PRODUCTION_DT, 0, screen=big)
    assert list(gn["ok"]) == [1, 0, 1]
    for b in (0, 2):
        alone = audit_device(R, xr[b:b + 1], ar.PRODUCTION_DT, 0, screen=big)
        for k in alone:
            assert np.array_equal(gn[k][b], alone[k][0]), k
    xs, ref, _ = stored
    for kw in (dict(), dict(drive_only=0), dict(volt_max=30.0), dict(tau_ratio_max=0.9), dict(jvel_max=40.0, volt_max=0.0), dict(volt_max=0.0)):
        g = audit_device(R, xs, ar.PRODUCTION_DT, 0, screen=R.actuator_screen(**kw), full=False)
        assert np.array_equal(g["ok"], ar.audit(20, xs, ar.PRODUCTION_DT, screen=kw)["ok"]), kw
        assert np.array_equal(g["summary"], audit_device(R, xs, ar.PRODUCTION_DT, 0)["summary"])
    assert L.lib.landing_actuator_audit_batch(L.ctx, 0, None, 0, None, None, None, None, None, None, None, None, None, None) == 0
    d = _T(np.zeros(4096))
    assert L.lib.landing_actuator_audit_batch(L.ctx, 2, d.data_ptr(), 3, d.data_ptr(), None, None, None, None, None, d.data_ptr(), d.data_ptr(), d.data_ptr(), None) == -1
    assert L.lib.landing_actuator_audit_batch(L.ctx, 2, d.data_ptr(), 0, d.data_ptr(), None, None, None, None, None, None, d.data_ptr(), d.data_ptr(), None) == -1
    L2 = lc("capi").LandingLib(20, device=0)
    assert L2.lib.landing_actuator_audit_batch(L2.ctx, 2, d.data_ptr(), 0, d.data_ptr(), None, None, None, None, None, d.data_ptr(), d.data_ptr(), d.data_ptr(), None) == -1
    assert b"no model" in L2.lib.landing_last_error()
    L2.close()


def test_screened_pairs_against_the_unscreened_writer_gpu(gpu, stored):
    """synthetic status rows over every branch of the final-status rule: pairs, index and count bit-identical to landing_training_pairs_batch fed the
    final status with the rejected members masked out; nobody rejected = the unscreened output; everybody rejected = count 0"""
    import torch
    N = 20
    L, R = gpu(N)
    Pm, pl = lc("problem"), lc("pipeline")
    xs, _, _ = stored
    rows = [(0, 0, -1), (0, 3, -1), (0, 1, 0), (0, 0, 0), (0, 0, 2), (0, 0, 4), (0, 1, 2), (0, 3, 4), (0, 4, 0), (0, 2, -1)]
    B = 3 * len(rows)
    st3 = np.array([rows[b % len(rows)] for b in range(B)], np.int32)
    x = np.array([xs[(b // 2) % 7] for b in range(B)])
    P, _, _, _ = Pm.make_batch(B, N, 0.6, seed=3, consts=Pm.production_constants("main"), dt_grid="reference")
    fin = pl.final_status(st3)
    ref = ar.audit(N, x, ar.PRODUCTION_DT)
    dP, dx, dst = _T(P), _T(x), _T(st3)
    f64, i32 = dict(device="cuda", dtype=torch.float64), dict(device="cuda", dtype=torch.int32)

    def outs():
        return dict(pin=torch.full((B, 9), float("nan"), **f64), pout=torch.full((B, x.shape[1]), float("nan"), **f64), index=torch.full((B,), -9, **i32),
                    count=torch.full((1,), -9, **i32))

    def screened(screen):
        o = dict(outs(), summary=torch.empty(B, 8, **f64), where=torch.empty(B, 4, **i32), ok=torch.empty(B, **i32))
        R.screened_pairs(B, dP.data_ptr(), dx.data_ptr(), dst.data_ptr(), o["summary"].data_ptr(), o["where"].data_ptr(), o["ok"].data_ptr(), o["pin"].data_ptr(),
                         o["pout"].data_ptr(), o["index"].data_ptr(), o["count"].data_ptr(), screen=screen, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    def pairs(status):
        o = outs()
        ds = _T(status.astype(np.int32))
        R.training_pairs_device(B, dP.data_ptr(), dx.data_ptr(), ds.data_ptr(), o["pin"].data_ptr(), o["pout"].data_ptr(), o["index"].data_ptr(), o["count"].data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    got = screened(None)
    ar.assert_matches(got, ref)
    want = pairs(np.where((fin == 0) & (ref["ok"] == 0), 1, fin))
    assert 0 < want["count"][0] == ((fin == 0) & (ref["ok"] == 1)).sum() < (fin == 0).sum()
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    nobody, plain = screened(R.actuator_screen(volt_max=1e9)), pairs(fin)
    for k in plain:
        assert np.array_equal(nobody[k], plain[k], equal_nan=True), k
    everybody = screened(R.actuator_screen(volt_max=1e-3))
    assert everybody["count"][0] == 0 and (everybody["index"] == -1).all() and not everybody["ok"].any()


def _drop_states(B, seed):
    Pm = lc("problem")
    return Pm.make_batch(B, 20, 0.6, seed=seed, consts=Pm.production_constants("main"), dt_grid="reference")


def _run(chain, P, X0):
    import torch
    out = chain.run_device(_T(P), _T(X0))
    torch.cuda.synchronize()
    return chain.to_host(out)


def _check_screened(plain, scr, screen_kw):
    """a screened chain result against the unscreened one and the reference module"""
    for k in ("x", "status", "iters", "f", "kkt"):
        assert np.array_equal(plain[k], scr[k]), k
    ok = scr["audit_ok"]
    keep = np.nonzero((plain["final_status"] == 0) & (ok == 1))[0]
    cols = np.nonzero(np.isin(plain["index"], keep))[0]      # the unscreened pairs filtered by audit_ok
    assert scr["n_kept"] == len(keep) and np.array_equal(scr["index"], keep)
    assert np.array_equal(scr["pair_in"], plain["pair_in"][:, cols]) and np.array_equal(scr["pair_out"], plain["pair_out"][:, cols])
    ref = ar.audit(20, scr["x"], ar.PRODUCTION_DT, screen=screen_kw)
    ar.assert_matches(dict(summary=scr["audit"], where=scr["audit_where"], ok=ok), ref)
    return ok


def test_screened_chain_against_the_unscreened_chain_gpu():
    """RefineChain(N = 20, screen = default) on 16 drop states of the production grid: x, status, iters bit-identical to the chain without screen; the
    screened pairs = the unscreened pairs filtered by audit_ok; every member's audit = the reference module's on the returned x; volt_max = 1e9 writes
    exactly the unscreened pairs.  Where the default screen rejects none or all of the 16, volt_max = the median of the batch's entry-4 values (from the
    reference module on the unscreened result) is run too, so that both outcomes occur."""
    pl = lc("pipeline")
    P, X0, _, _ = _drop_states(16, 20211)
    c0 = pl.RefineChain(20, device=0)
    plain = _run(c0, P, X0)
    assert "audit" not in plain and plain["n_kept"] > 0
    mk = c0.R.actuator_screen

    def with_screen(screen):
        c = pl.RefineChain(20, device=0, screen=screen)
        r = _run(c, P, X0)
        c.close()
        return r
    ok = _check_screened(plain, with_screen(mk()), {})
    r = with_screen(mk(volt_max=1e9))
    assert _check_screened(plain, r, dict(volt_max=1e9)).all()
    for k in ("pair_in", "pair_out", "index", "n_kept"):
        assert np.array_equal(r[k], plain[k]), k
    if ok.all() or not ok.any():
        med = float(np.median(ar.audit(20, plain["x"], ar.PRODUCTION_DT)["summary"][:, 3]))
        ok = _check_screened(plain, with_screen(mk(volt_max=med)), dict(volt_max=med))
    c0.close()
    assert ok.any() and not ok.all()


def test_screened_data_generation_gpu(tmp_path):
    """dataset.generate_streamed(refine=True, screen=...), two batches of 8: the shard = the unscreened run's shard with the rejected columns removed; the
    member log carries the audit's summary and ok.  The threshold lies between the two middle entry-4 values of the unscreened run's columns (reference module), so that some are removed."""
    ds, rbd, capi = lc("dataset"), lc("rbd"), lc("capi")
    kw = dict(dt_grid="reference", law="main", refine=True, seed0=4100)
    r0 = ds.generate_streamed(20, 2, 8, tmp_path / "plain", **kw)
    with np.load(tmp_path / "plain.npz") as d:
        pin, pout = d["input"], d["output"]
    M = pout.shape[1]
    assert M == r0["samples_written"] >= 2
    nX, nU = 12 * 21, 24 * 20
    x = np.concatenate([pout[:nX], pout[nX + nU:], pout[nX:nX + nU]]).T      # [X; U; jpos] columns -> the refinement's [X; jpos; U] rows
    s4 = ar.audit(20, x, ar.PRODUCTION_DT)["summary"][:, 3]
    med = float(np.sort(s4)[(M - 1) // 2:(M - 1) // 2 + 2].mean())      # (between two members' values: no member sits on the threshold)
    ref_ok = ar.audit(20, x, ar.PRODUCTION_DT, screen=dict(volt_max=med))["ok"]
    assert 0 < ref_ok.sum() < M
    L = capi.LandingLib(20, device=0)
    screen = rbd.Rbd(L).actuator_screen(volt_max=med)
    L.close()
    r1 = ds.generate_streamed(20, 2, 8, tmp_path / "screened", log_path=tmp_path / "log.jsonl", screen=screen, **kw)
    with np.load(tmp_path / "screened.npz") as d:
        assert np.array_equal(d["input"], pin[:, ref_ok == 1]) and np.array_equal(d["output"], pout[:, ref_ok == 1])
    assert r1["samples_written"] == ref_ok.sum() and r1["status_counts"] == r0["status_counts"]
    recs = [json.loads(l) for l in open(tmp_path / "log.jsonl")]
    assert len(recs) == 16 and all(set(capi.AUDIT_SUMMARY) | {"ok", "batch"} <= set(r) for r in recs)
    kept = [r for r in recs if r["status"] == 0]
    assert [r["ok"] for r in kept] == list(ref_ok)
    assert np.abs(np.array([r["volt_drive"] for r in kept]) - s4).max() <= 1e-12 * max(1.0, s4.max())
