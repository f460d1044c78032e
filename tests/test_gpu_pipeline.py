"""GPU tests of the drop-state chain (include/landing_nlp.h landing_pipeline_*; csrc/pipeline_kernels.hip, pipeline_capi.inc): SRBM solve ->
kinodynamic refinement -> warm re-solve -> training pairs in one library call per batch, N = 20 on the production grid.  The chain must equal its
passes called one by one, every member it keeps must be a KKT point under the oracle, the host entry point must equal the device one, and the
streamed data generation must write what one batch at a time writes."""
import numpy as np
import pytest

from conftest import lc
from test_pipeline_cpu import _mirror, assert_trig_rows_close, trig_rows

pytestmark = pytest.mark.gpu
N = 20
KKT_TOL = 1e-6


def _batch(B, law, seed):
    Pm = lc("problem")
    return Pm.make_batch(B, N, 0.6, seed=seed, consts=Pm.production_constants(law), dt_grid="reference", law=law)


@pytest.fixture(scope="module")
def chain():
    c = lc("pipeline").RefineChain(N, device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def main1024(chain):
    """one chain call on 1024 drop states of law main, seed 20211 (lam_g and the SRBM solutions asked for)"""
    import torch
    P, X0, q, qd = _batch(1024, "main", 20211)
    T = lambda a: torch.as_tensor(a, device="cuda")
    xs = torch.empty(1024, chain.L.nx, device="cuda", dtype=torch.float64)
    out = chain.run_device(T(P), T(X0), out=chain.alloc(1024, lam=True), x_srbm=xs)
    torch.cuda.synchronize()
    r = chain.to_host(out)
    r["xs"] = xs.cpu().numpy()
    return P, X0, q, qd, r


def _consts():
    mass, Ib, Ibi = lc("constants").robot_constants()
    return mass, np.asarray(Ib), np.asarray(Ibi), lc("problem").REFERENCE_DT_GRID


def _certify(x, lam, lb, ub, cost, mu):
    from oracle import kinodyn_oracle as ko
    kd = lc("kinodyn")
    mass, Ib, Ibi, dt = _consts()
    out = np.zeros((x.shape[0], 3))
    for lo in range(0, x.shape[0], 128):
        sl = slice(lo, lo + 128)
        gf = np.array([kd.terminal_cost(x[b], N, cost[b][12:], cost[b][:12])[1] for b in range(*sl.indices(x.shape[0]))])
        out[sl] = ko.kkt_batch(x[sl], lam[sl], N, dt, mass, Ib, Ibi, mu, lb[sl], ub[sl], gf)
    return out


def test_pose_kernel_on_the_device_equals_the_host_mirror(chain):
    import torch
    Pm, kd = lc("problem"), lc("kinodyn")
    B = 1024
    P, _, _, _ = _batch(B, "main", 20211)
    xs = np.random.default_rng(5).normal(size=(B, Pm.nx(N)))
    nxk, ng = kd.dims(N)
    dP, dxs = torch.as_tensor(P, device="cuda"), torch.as_tensor(xs, device="cuda")
    lb, ub, cost, x0 = (torch.full(s, float("nan"), device="cuda", dtype=torch.float64) for s in ((B, ng), (B, ng), (B, 24), (B, nxk)))
    chain.R.kinodyn_pose_device(B, dP.data_ptr(), dxs.data_ptr(), lb.data_ptr(), ub.data_ptr(), cost.data_ptr(), x0.data_ptr(),
                                stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    lb, ub, cost, x0 = (v.cpu().numpy() for v in (lb, ub, cost, x0))
    mlb, mub, mcost, mx0 = _mirror(P, xs, N)
    assert np.array_equal(x0, mx0) and np.array_equal(cost, mcost)
    t = trig_rows(N)
    rest = np.setdiff1d(np.arange(ng), t)
    assert np.array_equal(lb[:, rest], mlb[:, rest]) and np.array_equal(ub[:, rest], mub[:, rest])
    assert_trig_rows_close(lb[:, t], mlb[:, t]); assert_trig_rows_close(ub[:, t], mub[:, t])


def test_chain_equals_its_passes(chain, main1024):
    """landing_pipeline_batch == solve_device -> pose entry -> kinodyn_solve_device (cold options) -> kinodyn_solve_device (warm options, from that x)
    -> select and pairs in numpy, bit for bit in every output"""
    import torch
    P, X0, q, qd, r = main1024
    L, R = chain.L, chain.R
    kd, ds, pl, Pm = lc("kinodyn"), lc("dataset"), lc("pipeline"), lc("problem")
    B = P.shape[0]
    nxk, ng = kd.dims(N)
    f64, i32 = dict(device="cuda", dtype=torch.float64), dict(device="cuda", dtype=torch.int32)
    s = torch.cuda.current_stream().cuda_stream
    dP, dX0 = torch.as_tensor(P, **f64), torch.as_tensor(X0, **f64)
    xs, st0, it0 = torch.empty(B, L.nx, **f64), torch.empty(B, **i32), torch.empty(B, **i32)
    L.solve_device(B, dP.data_ptr(), dX0.data_ptr(), L.default_opts(), xs.data_ptr(), d_status=st0.data_ptr(), d_iters=it0.data_ptr(), stream=s)
    lb, ub, cost, x0 = torch.empty(B, ng, **f64), torch.empty(B, ng, **f64), torch.empty(B, 24, **f64), torch.empty(B, nxk, **f64)
    R.kinodyn_pose_device(B, dP.data_ptr(), xs.data_ptr(), lb.data_ptr(), ub.data_ptr(), cost.data_ptr(), x0.data_ptr(), stream=s)
    mass, Ib, Ibi, dt = _consts()
    mu = Pm.production_constants("main").mu
    passes = []
    for o, start in ((R.kinodyn_default_opts(), x0), (R.kinodyn_warm_opts(), None)):
        start = start if start is not None else passes[-1]["x"]
        p = dict(x=torch.empty(B, nxk, **f64), f=torch.empty(B, **f64), lam=torch.empty(B, ng, **f64), st=torch.empty(B, **i32), it=torch.empty(B, **i32),
                 kkt=torch.empty(B, 3, **f64))
        R.kinodyn_solve_device(B, N, lb.data_ptr(), ub.data_ptr(), cost.data_ptr(), start.data_ptr(), dt, mass, Ib, Ibi, mu, o, p["x"].data_ptr(), p["f"].data_ptr(),
                               p["lam"].data_ptr(), p["st"].data_ptr(), p["it"].data_ptr(), p["kkt"].data_ptr(), stream=s)
        passes.append(p)
    torch.cuda.synchronize()
    a, w = ({k: v.cpu().numpy() for k, v in p.items()} for p in passes)
    assert np.array_equal(r["xs"], xs.cpu().numpy())
    status3 = np.stack([st0.cpu().numpy(), a["st"], w["st"]], axis=1); iters3 = np.stack([it0.cpu().numpy(), a["it"], w["it"]], axis=1)
    take1 = (w["st"] != 0) & (a["st"] == 0)
    pick = lambda k: np.where(take1.reshape((-1,) + (1,) * (a[k].ndim - 1)), a[k], w[k])
    assert np.array_equal(r["status"], status3) and np.array_equal(r["iters"], iters3)
    for mine, theirs in (("x", "x"), ("f", "f"), ("lam_g", "lam"), ("kkt", "kkt")):
        assert np.array_equal(r[mine], pick(theirs)), mine
    fin = pl.final_status(status3)
    nX = 12 * (N + 1)
    inp, out = ds.training_pairs(N, q, qd, np.concatenate([r["x"][:, :nX], r["x"][:, nX + 12 * N:]], axis=1), fin, jpos_star=r["x"][:, nX:nX + 12 * N])
    assert r["n_kept"] == int((fin == 0).sum()) and np.array_equal(r["index"], np.nonzero(fin == 0)[0])
    assert np.array_equal(r["pair_in"], inp) and np.array_equal(r["pair_out"], out)
    print("chain of 1024 (law main): SRBM converged %d; refinement %s; re-solve %s; final %s; %d take the refinement's result" % (
        (status3[:, 0] == 0).sum(), np.bincount(a["st"], minlength=5).tolist(), np.bincount(w["st"], minlength=5).tolist(), np.bincount(fin, minlength=5).tolist(), take1.sum()))


def _check_kept(P, q, qd, r, mu):
    kd = lc("kinodyn")
    lb, ub, cost, _ = _mirror(P, r["xs"], N)
    keep = r["final_status"] == 0
    k = _certify(r["x"][keep], r["lam_g"][keep], lb[keep], ub[keep], cost[keep], mu)
    assert k.max() <= KKT_TOL * 1.0001, (k.max(axis=0), int(np.argmax(k.max(axis=1))))
    assert np.array_equal(r["pair_in"], np.concatenate([q[keep, 3:6], qd[keep]], axis=1).T)
    for j, b in enumerate(np.nonzero(keep)[0]):
        X, U, J = kd.unpack_x(r["x"][b], N)
        assert np.array_equal(r["pair_out"][:, j], np.concatenate([X.flatten(order="F"), U.flatten(order="F"), J.flatten(order="F")]))
    return keep


def test_kept_members_are_certified(main1024):
    """every kept member is a KKT point <= 1e-6 under oracle/kinodyn_oracle.py with the host mirror's bounds; pair_in = [q_init(4:6); qd_init]; pair_out
    unpacks to the member's X, U, jpos; kept >= the refinement's converged count; every member decided (0 / 3) or counted undecided, at most 0.5 %"""
    P, X0, q, qd, r = main1024
    mu = lc("problem").production_constants("main").mu
    keep = _check_kept(P, q, qd, r, mu)
    fin = r["final_status"]
    und = ~np.isin(fin, (0, 3))
    assert keep.sum() >= (r["status"][:, 1] == 0).sum()
    assert und.mean() <= 0.005, np.bincount(fin, minlength=5)
    print("law main, 1024: kept %d, certified infeasible %d, undecided %d" % (keep.sum(), (fin == 3).sum(), und.sum()))


def test_host_entry_equals_device_entry(chain, main1024):
    """landing_pipeline_21 (the 21 SRBM arguments, host arrays) on the same batch == landing_pipeline_batch, bit for bit"""
    P, X0, q, qd, r = main1024
    Pm = lc("problem")
    args = Pm.make_args21(P.shape[0], N, 0.6, seed=20211, consts=Pm.production_constants("main"), dt_grid="reference", law="main")
    assert np.array_equal(chain.L.pack_args21(args), P)
    h = chain.R.pipeline_21(args, want_lam=True)
    for k in ("x", "f", "lam_g", "status", "iters", "kkt", "pair_in", "pair_out", "n_kept"):
        assert np.array_equal(h[k], r[k]), k


def test_law_datagen(chain):
    """law datagen, 256 drop states: every kept member certified; counts printed (no threshold: the hard law is unmeasured through this path)"""
    import torch
    P, X0, q, qd = _batch(256, "datagen", 7)
    T = lambda a: torch.as_tensor(a, device="cuda")
    xs = torch.empty(256, chain.L.nx, device="cuda", dtype=torch.float64)
    out = chain.run_device(T(P), T(X0), out=chain.alloc(256, lam=True), x_srbm=xs)
    torch.cuda.synchronize()
    r = chain.to_host(out); r["xs"] = xs.cpu().numpy()
    keep = _check_kept(P, q, qd, r, lc("problem").production_constants("datagen").mu)
    print("law datagen, 256: final status counts %s, kept %d" % (np.bincount(r["final_status"], minlength=5).tolist(), keep.sum()))


def test_streamed_refined_shards(chain, tmp_path):
    """dataset.generate_streamed(refine=True): three batches of 256 (SRBM of batch i + 1 on its own stream under the refinement of batch i) write
    the shard that three landing_pipeline_batch calls give; 9 input rows, 48N + 12 output rows; normalise / denormalise with jpos round-trip"""
    ds, Pm = lc("dataset"), lc("problem")
    res = ds.generate_streamed(N, 3, 256, tmp_path / "shard", dt_grid="reference", law="main", refine=True)
    with np.load(str(tmp_path / "shard.npz")) as d:
        inp, out = d["input"], d["output"]
    cols_i, cols_o = [], []
    for i in range(3):
        P, X0, _, _ = _batch(256, "main", i)
        r = chain.run_host(P, X0)
        cols_i.append(r["pair_in"]); cols_o.append(r["pair_out"])
    assert inp.shape[0] == 9 and out.shape[0] == 48 * N + 12 and inp.shape[1] == res["samples_written"]
    assert np.array_equal(inp, np.concatenate(cols_i, axis=1)) and np.array_equal(out, np.concatenate(cols_o, axis=1))
    mass = Pm.make_batch(1, N, 0.6, seed=0, dt_grid="reference")[0][0, Pm.param_offsets(N)["mass"]]
    inp_n, out_n, stats = ds.normalise(N, inp, out, mass, with_jpos=True)
    for e in (0, out.shape[1] // 2, out.shape[1] - 1):
        X, U, J = ds.denormalise(out_n[:, e], stats, with_jpos=True)
        Xs, Us, Js = ds._split_output(N, out[:, e], True)
        m = np.ones((12, N + 1), bool); m[0:2, 0] = False
        assert np.allclose(X[m], Xs[m], atol=1e-10) and np.allclose(U[:12], Us[:12], atol=1e-10) and np.allclose(J, Js, atol=1e-10)
