"""Training-pair writer for the reference's NN warm-start pipeline.

generate_data/generate_training_data_automated.m:204-219 appends, per solved drop state,
    input  column = [q_init(4:6) ; qd_init(:)]            (9 values: rpy0, omega0, v0)
    output column = [X*(:) ; U*(:) ; jpos*(:)]
to ``training_data`` and saves it after every sample.  The SRBM stage alone produces X* and U* (pairs without
the jpos* block); the joint trajectories jpos* come from the kinodynamic refinement and its warm re-solve,
which the library chains behind the SRBM solve on the device (pipeline.RefineChain, include/landing_nlp.h
landing_pipeline_*): ``generate_streamed(..., refine=True)`` writes [X*; U*; jpos*] shards as the reference
does.  Members whose status is not CONVERGED are skipped, as the interactive "Save trajectory for training?"
prompt of the reference would.
"""
import numpy as np


def training_pairs(N, q_init, qd_init, x_star, status=None, jpos_star=None):
    """-> (input [9, M], output [12(N+1)+24N(+12N), M]) for the M accepted members, column per sample."""
    q_init = np.atleast_2d(q_init); qd_init = np.atleast_2d(qd_init); x_star = np.atleast_2d(x_star)
    keep = np.ones(x_star.shape[0], bool) if status is None else (np.asarray(status) == 0)
    inp = np.concatenate([q_init[keep, 3:6], qd_init[keep, :]], axis=1).T
    out = x_star[keep].T          # x = [X(:); U(:)] is already the column-major stacking the script writes
    if jpos_star is not None:
        out = np.concatenate([out, np.atleast_2d(jpos_star)[keep].T], axis=0)
    return inp, out


def append_shard(path, inp, out):
    """append samples to an .npz shard (the reference re-saves a growing .mat after every sample,
    generate_training_data_automated.m:214-219).  The shard is rewritten atomically: a crash mid-write leaves the
    previous file intact."""
    import os
    import tempfile
    path = str(path)
    if not path.endswith(".npz"):
        path += ".npz"            # numpy appends the suffix on save but not on load: normalise once for both
    if os.path.exists(path):
        with np.load(path) as d:
            inp = np.concatenate([d["input"], inp], axis=1)
            out = np.concatenate([d["output"], out], axis=1)
    fd, tmp = tempfile.mkstemp(suffix=".npz", dir=os.path.dirname(os.path.abspath(path)))
    try:
        with os.fdopen(fd, "wb") as fh:
            np.savez_compressed(fh, input=inp, output=out)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise
    return inp.shape[1]


# ---- the reference's .mat layout and the normalisation its NN pipeline expects ------------------------------
def save_training_mat(path, inp, out):
    """`training_data.input` / `training_data.output` as generate_training_data_automated.m:204-219 grows them (one column per
    sample).  Written as a MAT v5 file through scipy (the reference passes '-V7.3', i.e. HDF5, for which this image has no
    writer; MATLAB's `load` reads both)."""
    from scipy.io import savemat
    savemat(str(path), {"training_data": {"input": np.asarray(inp, float), "output": np.asarray(out, float)}}, do_compression=True)


def load_training_mat(path):
    from scipy.io import loadmat
    td = loadmat(str(path), squeeze_me=True, struct_as_record=False)["training_data"]
    return np.atleast_2d(td.input), np.atleast_2d(td.output)


def _split_output(N, col, with_jpos):
    nX, nU = 12 * (N + 1), 24 * N
    X = col[:nX].reshape(12, N + 1, order="F"); U = col[nX:nX + nU].reshape(24, N, order="F")
    J = col[nX + nU:nX + nU + 12 * N].reshape(12, N, order="F") if with_jpos else None
    return X, U, J


def normalise(N, inp, out, mass, with_jpos=False):
    """generate_data/data_normalization.m:38-114.  inp [9, M], out [nX + nU (+ 12N), M] -> (input_n, output_n [.. + 4, M], stats):
    z-scores of the input, the states, the foot positions (and joint angles) with MATLAB's `std(x, 0, 2)` (n-1 normalisation);
    X_norm(1:2, 1) = 0; ground-reaction forces of every leg shifted to their touch-down index td = first column with f_z > 1,
    padded with the last column, divided by the body weight; td (1-based, 4 values) appended.  Deviations, stated: a zero standard
    deviation maps to 0 instead of NaN, a leg that never loads gets td = 1 (the MATLAB script errors on both)."""
    inp = np.asarray(inp, float); out = np.asarray(out, float)
    M = out.shape[1]
    sd = lambda a: np.std(a, axis=1, ddof=1) if a.shape[1] > 1 else np.zeros(a.shape[0])
    div = lambda a, s: np.divide(a, s, out=np.zeros_like(a), where=s != 0)
    mean_in, std_in = inp.mean(axis=1), sd(inp)
    mean_out, std_out = out.mean(axis=1), sd(out)
    mX, mU, mJ = _split_output(N, mean_out, with_jpos); sX, sU, sJ = _split_output(N, std_out, with_jpos)
    stats = dict(mean_input=mean_in, std_input=std_in, mean_X=mX, mean_U=mU, mean_jpos=mJ, std_X=sX, std_U=sU, std_jpos=sJ, td_scale=1, mass=mass, N=N)
    inp_n = div(inp - mean_in[:, None], np.broadcast_to(std_in[:, None], inp.shape))
    cols = []
    for e in range(M):
        X, U, J = _split_output(N, out[:, e], with_jpos)
        Un = np.zeros_like(U); td = np.ones(4)
        for leg in range(4):
            f = U[12 + 3 * leg:15 + 3 * leg]
            hit = np.nonzero(f[2] > 1.0)[0]
            t0 = int(hit[0]) if hit.size else 0                      # 0-based; td is stored 1-based as in MATLAB
            fo = np.concatenate([f[:, t0:], np.repeat(f[:, -1:], t0, axis=1)], axis=1)
            Un[12 + 3 * leg:15 + 3 * leg] = fo / (mass * 9.81)
            td[leg] = t0 + 1
        Xn = div(X - mX, sX); Xn[0:2, 0] = 0.0
        Un[:12] = div(U[:12] - mU[:12], sU[:12])
        parts = [Xn.flatten(order="F"), Un.flatten(order="F")]
        if with_jpos:
            parts.append(div(J - mJ, sJ).flatten(order="F"))
        cols.append(np.concatenate(parts + [td]))
    return inp_n, np.array(cols).T, stats


def denormalise(nn_col, stats, with_jpos=False):
    """generate_data/data_denormalization.m:17-38: one normalised output column -> (X, U, jpos)"""
    N = stats["N"]
    Xn, Un, Jn = _split_output(N, nn_col, with_jpos)
    td = np.rint(nn_col[-4:]).astype(int)
    X = Xn * stats["std_X"] + stats["mean_X"]
    U = np.zeros((24, N))
    U[:12] = Un[:12] * stats["std_U"][:12] + stats["mean_U"][:12]
    for leg in range(4):
        fo = Un[12 + 3 * leg:15 + 3 * leg]
        t0 = td[leg] - 1
        U[12 + 3 * leg:15 + 3 * leg] = np.concatenate([np.zeros((3, t0)), fo[:, :N - t0]], axis=1) * (stats["mass"] * 9.81)
    J = Jn * stats["std_jpos"] + stats["mean_jpos"] if with_jpos else None
    return X, U, J


def write_member_log(path, status, iters, kkt, f=None, extra=None):
    """JSON lines, one record per batch member (SURVEY section 5 hook: iterations, pr_inf, du_inf, compl, status).  extra: further fields of every
    record; a list or array with one entry per member gives each record its own entry"""
    import json
    per_member = {k: np.asarray(v).tolist() for k, v in (extra or {}).items() if isinstance(v, (list, tuple, np.ndarray)) and len(v) == len(status)}
    with open(path, "a") as fh:
        for m in range(len(status)):
            rec = {"member": m, "status": int(status[m]), "iterations": int(iters[m]), "pr_inf": float(kkt[m][0]), "du_inf": float(kkt[m][1]), "compl": float(kkt[m][2])}
            if f is not None:
                rec["f"] = float(f[m])
            if extra:
                rec.update(extra)
                rec.update({k: v[m] for k, v in per_member.items()})
            fh.write(json.dumps(rec) + "\n")


def generate_streamed(N, n_batches, B, shard_path, seed0=0, T=0.6, dt_grid="uniform", law="main", opts=None, depth=2, device=0, log_path=None, refine=False, screen=None, **form):
    """The data-generation loop of generate_data/generate_training_data_automated.m:38-219 as a STREAM of batches through one GPU (round 6): the drop states of batch i + 1 are sampled on
    the host and queued (`pipeline.BatchPipeline` over the library's landing_stream_submit / _wait: one context, `depth` launches in flight) while batch i is solved; the converged members of
    every batch that leaves the pipeline are appended to the shard in the reference's layout (training_pairs / append_shard), every member is logged (write_member_log).  Returns the
    counts per status and the number of samples written.  Results per batch are bit-identical to one solve at a time (tests/test_gpu_dataset.py).
    refine=True: the whole chain per batch (SRBM solve, kinodynamic refinement, warm re-solve; `opts` a pipeline options struct, default
    landing_pipeline_opts_default), shards of [X*; U*; jpos*] -- see _generate_refined.
    screen (with refine=True): a landing_actuator_screen (rbd.Rbd.actuator_screen()); the shards then hold the members with final status 0 that also pass
    the actuator audit (landing_pipeline_screened_pairs_batch), the member log gains the audit's summary columns (capi.AUDIT_SUMMARY) and `ok`."""
    import importlib
    problem = importlib.import_module(__package__ + ".problem"); pipeline = importlib.import_module(__package__ + ".pipeline")
    consts = problem.production_constants(law) if dt_grid == "reference" else None
    if screen is not None and not refine:
        raise ValueError("the actuator screen audits refined trajectories: refine=True")
    if refine:
        return _generate_refined(problem, pipeline, consts, N, n_batches, B, shard_path, seed0, T, dt_grid, law, opts, device, log_path, screen)
    pipe = pipeline.BatchPipeline(N, depth=depth, device=device, opts=opts, **form)
    meta, counts, written = {}, {}, 0

    def take(res):
        nonlocal written
        q, qd = meta.pop(res["tag"])
        inp, out = training_pairs(N, q, qd, res["x"], res["status"])
        if inp.shape[1]:
            written = append_shard(shard_path, inp, out)
        if log_path:
            write_member_log(log_path, res["status"], res["iters"], res["kkt"], res["f"], extra={"batch": int(res["tag"])})
        for s in res["status"]:
            counts[int(s)] = counts.get(int(s), 0) + 1
    try:
        for i in range(n_batches):
            P, X0, q, qd = problem.make_batch(B, N, T, seed=seed0 + i, consts=consts, dt_grid=dt_grid, law=law)
            meta[i] = (q, qd)
            done = pipe.submit(P, X0, tag=i)
            if done is not None:
                take(done)
        for done in pipe.drain():
            take(done)
    finally:
        pipe.close()
    return dict(status_counts=counts, samples_written=written, batches=n_batches)


def _generate_refined(problem, pipeline, consts, N, n_batches, B, shard_path, seed0, T, dt_grid, law, opts, device, log_path, screen=None):
    """generate_streamed(refine=True): the SRBM solve of batch i + 1 is launched on its own stream before batch i is refined on another
    (landing_pipeline_refine_batch; its host loop synchronises its own stream only, and the SRBM solver's workspace is not the refinement's, so the
    two overlap on the GPU).  The SRBM outputs are double-buffered; a warm-up call with one iteration per pass sizes every workspace first, so that
    no growth (and the device-wide synchronisation it needs) lands inside the loop.  Per batch the result is bit-identical to one
    landing_pipeline_batch call.  Shards hold input [9, M] and output [48N + 12, M] = [X*(:); U*(:); jpos*(:)]; counts are of the final status."""
    import importlib
    import torch
    chain = pipeline.RefineChain(N, device=device, opts=opts, screen=screen)
    dev, o = chain.dev, chain.opts
    f64, i32 = dict(device=dev, dtype=torch.float64), dict(device=dev, dtype=torch.int32)
    s_srbm, s_ref = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    slots = [dict(xs=torch.empty(B, chain.L.nx, **f64), st=torch.empty(B, **i32), it=torch.empty(B, **i32), ev=torch.cuda.Event()) for _ in range(2)]
    out = chain.alloc(B)
    counts, written = {}, 0

    def batch(i):
        return problem.make_batch(B, N, T, seed=seed0 + i, consts=consts, dt_grid=dt_grid, law=law)

    def launch_srbm(i, P, X0):
        s = slots[i % 2]
        with torch.cuda.stream(s_srbm):
            s["P"], s["X0"] = torch.as_tensor(P, **f64), torch.as_tensor(X0, **f64)
            chain.L.solve_device(B, s["P"].data_ptr(), s["X0"].data_ptr(), o.srbm, s["xs"].data_ptr(), d_status=s["st"].data_ptr(), d_iters=s["it"].data_ptr(),
                                 stream=s_srbm.cuda_stream)
            s["ev"].record(s_srbm)

    try:
        batches = {0: batch(0)}
        w = type(o).from_buffer_copy(o)      # warm-up: the shapes of the loop, one iteration per pass
        w.srbm.max_iter = w.refine.max_iter = w.resolve.max_iter = 1
        with torch.cuda.stream(s_ref):
            chain.run_device(torch.as_tensor(batches[0][0], **f64), torch.as_tensor(batches[0][1], **f64), out=out, stream=s_ref, opts=w)
        torch.cuda.synchronize(dev)
        launch_srbm(0, *batches[0][:2])
        for i in range(n_batches):
            if i + 1 < n_batches:
                batches[i + 1] = batch(i + 1)
                launch_srbm(i + 1, *batches[i + 1][:2])      # batch i + 1's SRBM solve runs under batch i's refinement
            s = slots[i % 2]
            s_ref.wait_event(s["ev"])
            chain.refine_device(s["P"], s["xs"], s["st"], s["it"], out=out, stream=s_ref)
            s_ref.synchronize()
            res = chain.to_host(out)
            batches.pop(i)
            if res["n_kept"]:
                written = append_shard(shard_path, res["pair_in"], res["pair_out"])
            extra = {"batch": i}
            if screen is not None:
                capi = importlib.import_module(__package__ + ".capi")
                extra.update({n: res["audit"][:, j] for j, n in enumerate(capi.AUDIT_SUMMARY)}, ok=res["audit_ok"])
            if log_path:
                write_member_log(log_path, res["final_status"], res["iters"].sum(axis=1), res["kkt"], res["f"], extra=extra)
            for v in res["final_status"]:
                counts[int(v)] = counts.get(int(v), 0) + 1
    finally:
        torch.cuda.synchronize(dev)
        chain.close()
    return dict(status_counts=counts, samples_written=written, batches=n_batches)
