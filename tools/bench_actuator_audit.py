#!/usr/bin/env python3
"""Device time of the actuator audit (include/landing_nlp.h landing_actuator_audit_batch; csrc/actuator_kernels.hip) and of the pair writer behind it
(landing_pipeline_screened_pairs_batch) at N = 20, B = 1024: HIP events around each call, a warm-up, the median of --runs calls.  The members are the
stored refined trajectories of tests/golden tiled to B (the audit's time does not depend on the values); dt comes from the members' p, as the chain
passes it.  Algorithmic bytes per member: (48N + 12 + N) * 8 read, plus the outputs asked for; the fraction is of the 8 TB/s HBM figure the other
profiles use.  Writes one JSON object to --out and prints it.  The chain's time per batch to set it beside: tools/bench_refine_chain.py.

    python tools/bench_actuator_audit.py [--B 1024] [--runs 50] [--out profiles/actuator_audit.json]"""
import argparse, importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=1024); ap.add_argument("--runs", type=int, default=50); ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actuator_audit.json"))
a = ap.parse_args()
import torch
import actuator_reference as ar
P_ = importlib.import_module("landing-controller_amd.problem"); pl = importlib.import_module("landing-controller_amd.pipeline")
N, B, HBM = 20, a.B, 8e12
chain = pl.RefineChain(N, device=0)
L, R = chain.L, chain.R
f64, i32 = dict(device="cuda", dtype=torch.float64), dict(device="cuda", dtype=torch.int32)
nxk = 48 * N + 12
xs = ar.stored_solutions(os.path.join(ROOT, "tests", "golden"))
x = torch.as_tensor(np.ascontiguousarray(xs[np.arange(B) % len(xs)]), **f64)
P = torch.as_tensor(P_.make_batch(B, N, 0.6, seed=20211, consts=P_.production_constants("main"), dt_grid="reference")[0], **f64)
o_dt = P_.param_offsets(N)["dt"]
st3 = torch.zeros(B, 3, **i32)      # every member converged: the pair writer moves the most it can
full = [torch.empty(B, N, 12, **f64) for _ in range(3)]
summ, where, ok = torch.empty(B, 8, **f64), torch.empty(B, 4, **i32), torch.empty(B, **i32)
pin, pout, idx, cnt = torch.empty(B, 9, **f64), torch.empty(B, nxk, **f64), torch.empty(B, **i32), torch.empty(1, **i32)
fin = torch.zeros(B, **i32)
s = torch.cuda.current_stream().cuda_stream
d_dt = P.data_ptr() + 8 * o_dt
wide = R.actuator_screen(volt_max=1e9)


def median_ms(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); e1.synchronize()
        t.append(e0.elapsed_time(e1))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


def row(fn, bytes_member):
    med, lo, hi = median_ms(fn)
    return dict(median_ms=med, min_ms=lo, max_ms=hi, algorithmic_bytes=bytes_member * B, achieved_GBps=bytes_member * B / (med * 1e-3) / 1e9,
                fraction_of_hbm=bytes_member * B / (med * 1e-3) / HBM)


rd = (48 * N + 12 + N) * 8
summary_bytes = 8 * 8 + 4 * 4 + 4
pair_bytes = 2 * nxk * 8 + 2 * 9 * 8 + 2 * 4      # the pair kernel reads x and p's 9 values, writes both columns; the scan reads and writes 4 bytes a member
res = dict(what="actuator audit and screened pair writer, N = %d, B = %d, HIP events, median of %d calls after %d warm-up calls" % (N, B, a.runs, a.warmup),
           device=torch.cuda.get_device_name(0), hbm_reference_Bps=HBM,
           audit_summary_only=row(lambda: R.actuator_audit_device(B, d_dt, int(L.np_), x.data_ptr(), summ.data_ptr(), where.data_ptr(), ok.data_ptr(), stream=s), rd + summary_bytes),
           audit_all_outputs=row(lambda: R.actuator_audit_device(B, d_dt, int(L.np_), x.data_ptr(), summ.data_ptr(), where.data_ptr(), ok.data_ptr(), d_tau=full[0].data_ptr(),
                                                                 d_jvel=full[1].data_ptr(), d_volt=full[2].data_ptr(), stream=s), rd + summary_bytes + 3 * 12 * N * 8),
           screened_pairs_all_kept=row(lambda: R.screened_pairs(B, P.data_ptr(), x.data_ptr(), st3.data_ptr(), summ.data_ptr(), where.data_ptr(), ok.data_ptr(), pin.data_ptr(),
                                                                pout.data_ptr(), idx.data_ptr(), cnt.data_ptr(), screen=wide, stream=s), rd + summary_bytes + 12 + 4 + pair_bytes),
           screened_pairs_default_screen=row(lambda: R.screened_pairs(B, P.data_ptr(), x.data_ptr(), st3.data_ptr(), summ.data_ptr(), where.data_ptr(), ok.data_ptr(), pin.data_ptr(),
                                                                      pout.data_ptr(), idx.data_ptr(), cnt.data_ptr(), stream=s), rd + summary_bytes + 12 + 4 + pair_bytes * 5 / 7),
           unscreened_pairs=row(lambda: R.training_pairs_device(B, P.data_ptr(), x.data_ptr(), fin.data_ptr(), pin.data_ptr(), pout.data_ptr(), idx.data_ptr(), cnt.data_ptr(), stream=s),
                                pair_bytes))
R.screened_pairs(B, P.data_ptr(), x.data_ptr(), st3.data_ptr(), summ.data_ptr(), where.data_ptr(), ok.data_ptr(), pin.data_ptr(), pout.data_ptr(), idx.data_ptr(), cnt.data_ptr(), stream=s)
torch.cuda.synchronize()
res["kept_default_screen"] = int(cnt.cpu()[0])
chain.close()
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
