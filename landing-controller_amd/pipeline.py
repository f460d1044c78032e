"""Streaming batches through one GPU with several of them in flight (the data-generation use case of
generate_data/generate_training_data_automated.m:38: thousands of independent drop states, produced batch by batch).

The time of ONE batch of 1024 NLPs is set by its slowest member and by the granularity of two members per resident slot
(DESIGN.md 4.2); a second batch in flight fills the CUs that idle in its tail: 24-25 k instead of 19 k NLPs/s on one MI355X.
Rounds 3-5 did this here, with one solver context and one torch stream per lane; since round 6 the library does it itself
(landing_stream_* of include/landing_nlp.h: ONE context, the lanes and their HIP streams live behind landing_stream_submit / _wait)
and this class is the host-array convenience around it: uploads on a copy stream, the submission ordered behind them.

    pipe = BatchPipeline(N=40, depth=2)
    for P, X0 in batches:                      # numpy [B, np], [B, nx]
        done = pipe.submit(P, X0)              # returns the results of the batch that left the pipeline, or None
    for res in pipe.drain(): ...

RefineChain is the drop-state chain every production caller runs (SRBM solve -> kinodynamic refinement -> warm re-solve, the training pair;
landing_pipeline_* of include/landing_nlp.h): one context with the robot model, one library call per batch.

    chain = RefineChain(N=20)
    res = chain.run_host(P, X0)                # numpy in / out: x [B, 48N+12], status / iters [B, 3], pair_in [9, M], pair_out [48N+12, M], ...
"""
import importlib
from collections import deque

import numpy as np
import torch


class BatchPipeline:
    def __init__(self, N, depth=2, device=0, opts=None, **form):
        capi = importlib.import_module(__package__ + ".capi")
        self.N, self.depth, self.dev = N, depth, torch.device("cuda", device)
        self.lib = capi.LandingLib(N, device=device, **form)
        self.S = self.lib.stream(depth)
        self.copy = torch.cuda.Stream(device=self.dev)
        self.opts = opts or self.lib.default_opts()
        self.inflight = deque()
        self.n_submitted = 0

    def _collect(self):
        ticket, tag, b = self.inflight.popleft()
        self.S.wait(ticket)                    # host waits for that submission only; the later ones keep the GPU busy
        return dict(tag=tag, x=b["x"].cpu().numpy(), f=b["f"].cpu().numpy(), status=b["st"].cpu().numpy(), iters=b["it"].cpu().numpy(), kkt=b["kkt"].cpu().numpy())

    def submit(self, P, X0, tag=None):
        out = self._collect() if len(self.inflight) >= self.depth else None
        lib, B = self.lib, P.shape[0]
        f64 = dict(device=self.dev, dtype=torch.float64)
        with torch.cuda.stream(self.copy):
            b = dict(p=torch.as_tensor(np.ascontiguousarray(P), **f64), x0=torch.as_tensor(np.ascontiguousarray(X0), **f64),
                     x=torch.empty(B, lib.nx, **f64), f=torch.empty(B, **f64), kkt=torch.empty(B, 3, **f64),
                     st=torch.empty(B, device=self.dev, dtype=torch.int32), it=torch.empty(B, device=self.dev, dtype=torch.int32))
        ticket = self.S.submit(B, b["p"].data_ptr(), b["x0"].data_ptr(), self.opts, b["x"].data_ptr(), b["f"].data_ptr(), 0, b["st"].data_ptr(), b["it"].data_ptr(),
                               b["kkt"].data_ptr(), in_stream=self.copy.cuda_stream)
        self.inflight.append((ticket, self.n_submitted if tag is None else tag, b))
        self.n_submitted += 1
        return out

    def drain(self):
        outs = []
        while self.inflight:
            outs.append(self._collect())
        return outs

    def close(self):
        self.S.sync(); self.S.close(); self.lib.close()


def final_status(status3):
    """final status of each member from the pass columns [B, 3] = SRBM | refinement | warm re-solve (landing_pipeline_final_status): the re-solve's
    outcome if it converged, else the refinement's if that converged, else the re-solve's; the refinement's where the re-solve did not run (-1)"""
    s = np.asarray(status3)
    s1, s2 = s[:, 1], s[:, 2]
    return np.where(s2 < 0, s1, np.where((s2 == 0) | (s1 == 0), 0, s2)).astype(np.int32)


class RefineChain:
    """The drop-state chain on one device: a context with the 'mc3D' model (rbd.Rbd) and the library's landing_pipeline_batch /
    landing_pipeline_refine_batch.  Device tensors in / out (run_device, refine_device: torch tensors, no host copy inside), or numpy (run_host).
    screen: a landing_actuator_screen (rbd.Rbd.actuator_screen()).  With one, the chain runs without its pair outputs and the pairs are written by
    landing_pipeline_screened_pairs_batch on the same stream: the members with final status 0 that also pass the actuator audit; the outputs gain
    audit [B, 8], audit_where [B, 4] and audit_ok [B].  screen=None: the chain's own pair writer, nothing else."""

    def __init__(self, N, device=0, opts=None, screen=None):
        capi = importlib.import_module(__package__ + ".capi"); rbd = importlib.import_module(__package__ + ".rbd")
        self.N, self.dev = N, torch.device("cuda", device)
        self.L = capi.LandingLib(N, device=device)
        self.R = rbd.Rbd(self.L)
        self.opts = opts if opts is not None else self.R.pipeline_opts()
        self.screen = screen
        self.nxk, self.ngk = 48 * N + 12, 48 + 141 * (N - 1) + 117

    def alloc(self, B, lam=False):
        """output tensors of one batch"""
        f64, i32 = dict(device=self.dev, dtype=torch.float64), dict(device=self.dev, dtype=torch.int32)
        o = dict(x=torch.empty(B, self.nxk, **f64), f=torch.empty(B, **f64), kkt=torch.empty(B, 3, **f64), status=torch.empty(B, 3, **i32),
                 iters=torch.empty(B, 3, **i32), pair_in=torch.empty(B, 9, **f64), pair_out=torch.empty(B, self.nxk, **f64), index=torch.empty(B, **i32),
                 count=torch.zeros(1, **i32), lam_g=torch.empty(B, self.ngk, **f64) if lam else None)
        if self.screen is not None:
            o.update(audit=torch.empty(B, 8, **f64), audit_where=torch.empty(B, 4, **i32), audit_ok=torch.empty(B, **i32))
        return o

    def _outs(self, o):
        lam = dict(d_lam=o["lam_g"].data_ptr() if o["lam_g"] is not None else 0)
        if self.screen is not None:      # the pairs come from _screened_pairs, behind the chain
            return lam
        return dict(lam, d_in=o["pair_in"].data_ptr(), d_out=o["pair_out"].data_ptr(), d_index=o["index"].data_ptr(), d_count=o["count"].data_ptr())

    def _screened_pairs(self, P, o, st):
        if self.screen is not None:
            self.R.screened_pairs(P.shape[0], P.data_ptr(), o["x"].data_ptr(), o["status"].data_ptr(), o["audit"].data_ptr(), o["audit_where"].data_ptr(),
                                  o["audit_ok"].data_ptr(), o["pair_in"].data_ptr(), o["pair_out"].data_ptr(), o["index"].data_ptr(), o["count"].data_ptr(),
                                  screen=self.screen, stream=st.cuda_stream)

    def run_device(self, P, X0, out=None, x_srbm=None, stream=None, opts=None):
        """landing_pipeline_batch on device tensors P [B, np], X0 [B, 36N+12]; returns the output dict (queued on `stream`, not synchronised)"""
        B = P.shape[0]
        out = out or self.alloc(B)
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self.R.pipeline_device(B, P.data_ptr(), X0.data_ptr(), opts or self.opts, out["x"].data_ptr(), out["f"].data_ptr(), out["status"].data_ptr(),
                               out["iters"].data_ptr(), out["kkt"].data_ptr(), d_x_srbm=x_srbm.data_ptr() if x_srbm is not None else 0, stream=st.cuda_stream,
                               **self._outs(out))
        self._screened_pairs(P, out, st)
        return out

    def refine_device(self, P, XS, srbm_status=None, srbm_iters=None, out=None, stream=None, opts=None):
        """landing_pipeline_refine_batch behind SRBM solutions XS [B, 36N+12] already on the device (their status / iterations fill column 0)"""
        B = P.shape[0]
        out = out or self.alloc(B)
        st = stream if stream is not None else torch.cuda.current_stream(self.dev)
        self.R.pipeline_refine_device(B, P.data_ptr(), XS.data_ptr(), opts or self.opts, out["x"].data_ptr(), out["f"].data_ptr(), out["status"].data_ptr(),
                                      out["iters"].data_ptr(), out["kkt"].data_ptr(), d_srbm_status=srbm_status.data_ptr() if srbm_status is not None else 0,
                                      d_srbm_iters=srbm_iters.data_ptr() if srbm_iters is not None else 0, stream=st.cuda_stream, **self._outs(out))
        self._screened_pairs(P, out, st)
        return out

    @staticmethod
    def to_host(out):
        """device outputs -> numpy; the pairs cut to the kept columns (pair_in [9, M], pair_out [48N+12, M], index [M])"""
        r = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
        m = int(r.pop("count")[0])
        r.update(pair_in=r["pair_in"][:m].T.copy(), pair_out=r["pair_out"][:m].T.copy(), index=r["index"][:m].copy(), n_kept=m)
        r["final_status"] = final_status(r["status"])
        return r

    def run_host(self, P, X0, lam=False):
        """numpy P [B, np], X0 [B, 36N+12] -> the chain's results as numpy (one batch, synchronised)"""
        f64 = dict(device=self.dev, dtype=torch.float64)
        dP, dX0 = torch.as_tensor(np.ascontiguousarray(P), **f64), torch.as_tensor(np.ascontiguousarray(X0), **f64)
        out = self.run_device(dP, dX0, out=self.alloc(P.shape[0], lam))
        torch.cuda.synchronize(self.dev)
        return self.to_host(out)

    def close(self):
        self.L.close()
