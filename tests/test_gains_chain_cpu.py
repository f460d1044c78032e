"""Tracking gains straight from a solved batch: landing_sample_reference_kernel and the entry points around it,
through tests/emu (the same kernel sources compiled for the host).

  * the resampler against oracle/vbl_oracle.py::sample_reference (quadruped_SRBM_NLP.m:487-499), on a uniform time grid whose samples
    fall exactly on knots and into the extrapolated tail, and on a different non-uniform grid per member;
  * landing_tracking_gains_batch = landing_sample_reference_batch + landing_riccati_gains_batch, bit for bit;
  * status masking, both parameter layouts, the host-pointer twin, argument errors.

Tolerance of the interpolation: 1e-13 * max |knot value| per entry (ki * a + (1 - ki) * b is two multiplies and one add, with or without
contraction a handful of ulps of the larger knot value); held forces are copies and must be bit-equal."""
import numpy as np
import pytest

from conftest import lc
from emu_support import build_emu

N, B = 6, 3
NX = 36 * N + 12
DT6 = np.array([0.05, 0.02, 0.02, 0.05, 0.1, 0.2])      # the production pattern (coarse, fine around touch-down, coarse tail) at N = 6


@pytest.fixture(scope="module")
def emu():
    return build_emu()


@pytest.fixture(scope="module")
def lib(emu):
    L = lc("capi").LandingLib(N, lib_path=emu)
    yield L
    L.close()


ptr = lambda a: a.ctypes.data          # the emulation's "device" memory is host memory


def _integer_batch():
    """x [B, nx] in the solver's layout with X = 0, 1, 2, ... and U = 0, 1, 2, ... column-major (as test_vbl.test_sample_reference_grid), shifted per member"""
    return np.stack([np.concatenate([np.arange(12 * (N + 1), dtype=float), np.arange(24 * N, dtype=float)]) + 1000.0 * b for b in range(B)])


def _params(L, dts, fill=7.0):
    """p [B, np] of the context's layout: dt at its place, every other entry `fill`"""
    o_dt = 12 * (N + 1) + (24 * N if L.form.run_cost == 2 else 0)
    p = np.full((B, L.np_), fill)
    p[:, o_dt:o_dt + N] = dts
    return p


def _oracle(x, dts, dt_r, n):
    from oracle import vbl_oracle as vo
    Pm = lc("problem")
    xs, fs = [], []
    for b in range(x.shape[0]):
        Xs, Us = Pm.split_solution(N, x[b])
        xd, ud = vo.sample_reference(Xs, Us, np.concatenate([[0.0], np.cumsum(dts[b])]), dt_r, n)
        xs.append(xd); fs.append(ud)
    return np.array(xs), np.array(fs)


def _check_resampler(L, dts, dt_r, n):
    x = _integer_batch()
    p = _params(L, dts)
    xref = np.full((B, n, 24), np.nan); fref = np.full((B, n, 12), np.nan)
    L.sample_reference_device(B, ptr(x), ptr(p), dt_r, n, ptr(xref), ptr(fref))
    xo, fo = _oracle(x, dts, dt_r, n)
    for b in range(B):
        assert np.max(np.abs(xref[b] - xo[b])) <= 1e-13 * np.max(np.abs(x[b])), (b, np.max(np.abs(xref[b] - xo[b])))
    assert np.array_equal(fref, fo)
    return xref, fref


def test_resampler_uniform_grid(lib):
    """dt = 0.1, dt_r = 0.05, n = 13: every second sample sits on a knot (same comparison outcome as the oracle's), the last two lie
    beyond t*(N-1) = 0.5 and extrapolate the second-to-last interval with a negative weight"""
    n = 13
    xref, fref = _check_resampler(lib, np.full((B, N), 0.1), 0.05, n)
    x = _integer_batch()
    Pm = lc("problem")
    X0, U0 = Pm.split_solution(N, x[0])
    assert np.array_equal(xref[0, 0, :12], X0[:, 0]) and np.array_equal(xref[0, 2, :12], X0[:, 1])      # on the knots: the knot itself
    assert np.array_equal(fref[0, n - 1], U0[12:, N - 2])                                                # the last interval is never entered
    assert xref[0, n - 1, 0] > X0[0, N - 1]                                                              # extrapolated past X*(:, N-1)
    # only one output asked for
    only = np.full((B, n, 12), np.nan)
    lib.sample_reference_device(B, ptr(x), ptr(_params(lib, np.full((B, N), 0.1))), 0.05, n, 0, ptr(only))
    assert np.array_equal(only, fref)


def test_resampler_per_member_grid(lib):
    """a different non-uniform time grid per member: the production pattern at N = 6 and two permutations of it"""
    dts = np.stack([DT6, DT6[[5, 0, 3, 1, 4, 2]], DT6[::-1]])
    _check_resampler(lib, dts, 0.02, 23)      # 0.44 s: up to the end of the horizon
    _check_resampler(lib, dts, 0.013, 70)     # more than one workgroup of 64 samples, members straddling the boundary


def test_resampler_reads_dt_of_the_other_parameter_layout(emu):
    """a run_cost = 2 context keeps dt behind Uref: the same grids give the same reference"""
    L2 = lc("capi").LandingLib(N, lib_path=emu, ccc_params=True)
    assert L2.np_ == 37 * N + 112
    dts = np.stack([DT6, DT6[[5, 0, 3, 1, 4, 2]], DT6[::-1]])
    _check_resampler(L2, dts, 0.02, 23)
    L2.close()


def _solved_like_batch(seed=5):
    """x, p of a plausible solved batch: the callers' linear references with noise and non-zero forces, dt per member"""
    Pm = lc("problem")
    rng = np.random.default_rng(seed)
    P, X0, _, _ = Pm.make_batch(B, N, 0.6, seed=2)
    x = X0 + 0.01 * rng.normal(size=X0.shape)
    for b in range(B):
        U = x[b, 12 * (N + 1):].reshape(24, N, order="F")      # (a view: writes go to x)
        U[12:] = np.tile([3.0, -2.0, 25.0], 4)[:, None] + 5 * rng.normal(size=(12, N))
    o = Pm.param_offsets(N)["dt"]
    P[1, o:o + N] = DT6; P[2, o:o + N] = DT6[::-1]
    return x, P


def _weights():
    from oracle import vbl_oracle as vo
    F, Q, R = vo.reference_weights()
    return lc("constants").composite_body_inertia()[0:3, 0:3], 8.252, Q, np.diag(R).copy(), F


def _fused(L, x, p, dt_r, n, rk4, status=None, keep_ref=True):
    Ib, mass, Q, r, F = _weights()
    out = dict(P=np.full((B, n, 24, 24), np.nan), K=np.full((B, n, 12, 24), np.nan), A=np.full((B, n, 24, 24), np.nan), B=np.full((B, n, 24, 12), np.nan))
    if keep_ref:
        out.update(xref=np.full((B, n, 24), np.nan), fref=np.full((B, n, 12), np.nan))
    L.tracking_gains_device(B, ptr(x), ptr(p), dt_r, n, Ib, mass, Q, r, F, rk4, d_status=0 if status is None else ptr(status), d_P=ptr(out["P"]), d_K=ptr(out["K"]),
                            d_A=ptr(out["A"]), d_B=ptr(out["B"]), d_xref=ptr(out["xref"]) if keep_ref else 0, d_fref=ptr(out["fref"]) if keep_ref else 0)
    return out


@pytest.mark.parametrize("rk4", [False, True])
def test_fused_call_equals_its_two_halves(lib, rk4):
    x, p = _solved_like_batch()
    dt_r, n = 0.03, 9
    Ib, mass, Q, r, F = _weights()
    xref = np.zeros((B, n, 24)); fref = np.zeros((B, n, 12))
    lib.sample_reference_device(B, ptr(x), ptr(p), dt_r, n, ptr(xref), ptr(fref))
    P = np.zeros((B, n, 24, 24)); K = np.zeros((B, n, 12, 24)); A = np.zeros((B, n, 24, 24)); Bm = np.zeros((B, n, 24, 12))
    lib.riccati_gains_device(B, n, ptr(xref), ptr(fref), Ib, mass, Q, r, F, dt_r, rk4, ptr(P), ptr(K), ptr(A), ptr(Bm))
    assert np.isfinite(P).all() and np.isfinite(K).all() and np.abs(K).max() > 0
    f = _fused(lib, x, p, dt_r, n, rk4)
    for name, ref in (("P", P), ("K", K), ("A", A), ("B", Bm), ("xref", xref), ("fref", fref)):
        assert np.array_equal(f[name], ref), name
    # reference kept in the context's block: the same gains; then a larger call (the block grows) and the first one again
    s = _fused(lib, x, p, dt_r, n, rk4, keep_ref=False)
    assert np.array_equal(s["K"], K) and np.array_equal(s["P"], P)
    _fused(lib, x, p, dt_r, 2 * n, rk4, keep_ref=False)
    s = _fused(lib, x, p, dt_r, n, rk4, keep_ref=False)
    assert np.array_equal(s["K"], K) and np.array_equal(s["P"], P)
    # the host-pointer twin
    h = lib.tracking_gains_host(x, p, dt_r, n, Ib, mass, Q, r, F, rk4, want=("P", "K", "A", "B", "xref", "fref"))
    for name, ref in (("P", P), ("K", K), ("A", A), ("B", Bm), ("xref", xref), ("fref", fref)):
        assert np.array_equal(h[name], ref), name


def test_status_masks_members(lib):
    x, p = _solved_like_batch()
    x[1, 5] = np.nan                                         # what a member that broke down (status 2) may leave behind
    dt_r, n = 0.03, 9
    xg = x.copy(); xg[1] = x[0]
    free = _fused(lib, xg, p, dt_r, n, False)                # no d_status
    st = np.array([0, 2, 0], np.int32)
    for keep_ref in (True, False):
        m = _fused(lib, x, p, dt_r, n, False, status=st, keep_ref=keep_ref)
        for name, v in m.items():
            assert np.array_equal(v[1], np.zeros_like(v[1])), name
            assert np.array_equal(v[0], free[name][0]) and np.array_equal(v[2], free[name][2]), name
    Ib, mass, Q, r, F = _weights()
    h = lib.tracking_gains_host(x, p, dt_r, n, Ib, mass, Q, r, F, status=st, want=("K", "xref"))
    assert np.array_equal(h["K"], m["K"]) and np.array_equal(h["xref"][1], np.zeros((n, 24))) and np.array_equal(h["xref"][0], free["xref"][0])


def test_gains_with_the_other_parameter_layout(emu):
    """fused call on a run_cost = 2 context: dt is read at that layout's offset, so the gains equal those of the default layout"""
    x, p = _solved_like_batch()
    o = lc("problem").param_offsets(N)["dt"]
    L2 = lc("capi").LandingLib(N, lib_path=emu, ccc_params=True)
    p2 = _params(L2, p[:, o:o + N])
    L1 = lc("capi").LandingLib(N, lib_path=emu)
    a, b = _fused(L1, x, p, 0.03, 9, False), _fused(L2, x, p2, 0.03, 9, False)
    for name in a:
        assert np.array_equal(a[name], b[name]), name
    L1.close(); L2.close()


def test_argument_errors(lib):
    x, p = _solved_like_batch()
    Ib, mass, Q, r, F = _weights()
    n = 9
    xref = np.full((B, n, 24), -3.0); fref = np.full((B, n, 12), -3.0); K = np.full((B, n, 12, 24), -3.0)
    bad = [dict(n=1), dict(dt_r=0.0), dict(dt_r=-0.02), dict(d_x=0), dict(d_p=0), dict(out=False)]
    for c in bad:
        a = dict(n=n, dt_r=0.03, d_x=ptr(x), d_p=ptr(p), out=True); a.update(c)
        rc = lib.lib.landing_sample_reference_batch(lib.ctx, B, a["d_x"] or None, a["d_p"] or None, a["dt_r"], a["n"], ptr(xref) if a["out"] else None,
                                                    ptr(fref) if a["out"] else None, None)
        assert rc == -1 and lib.lib.landing_last_error().decode().startswith("landing_sample_reference_batch: "), c
        with pytest.raises(RuntimeError, match=r"landing_tracking_gains_batch failed \(-1\): landing_tracking_gains_batch: "):
            lib.tracking_gains_device(B, a["d_x"], a["d_p"], a["dt_r"], a["n"], Ib, mass, Q, r, F, d_K=ptr(K) if a["out"] else 0,
                                      d_xref=ptr(xref) if a["out"] else 0, d_fref=ptr(fref) if a["out"] else 0)
        if a["d_x"] and a["d_p"]:
            with pytest.raises(RuntimeError, match=r"landing_tracking_gains_host failed \(-1\)"):
                lib.tracking_gains_host(x, p, a["dt_r"], a["n"], Ib, mass, Q, r, F, want=("K",) if a["out"] else ())
    with pytest.raises(RuntimeError, match="R must be positive"):      # the Riccati arguments are checked before the resampler runs
        lib.tracking_gains_device(B, ptr(x), ptr(p), 0.03, n, Ib, mass, Q, np.zeros(12), F, d_K=ptr(K), d_xref=ptr(xref), d_fref=ptr(fref))
    assert (xref == -3.0).all() and (fref == -3.0).all() and (K == -3.0).all()
    # an empty batch is not an error
    lib.tracking_gains_device(0, ptr(x), ptr(p), 0.03, n, Ib, mass, Q, r, F, d_K=ptr(K))
    assert (K == -3.0).all()
