"""Development probe: diff the solver workspace of two builds after K iterations (which phase goes wrong first)."""
import importlib, sys, os, numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
capi = importlib.import_module("landing-controller_amd.capi"); problem = importlib.import_module("landing-controller_amd.problem")
N = 40; K = int(sys.argv[2]) if len(sys.argv) > 2 else 1
P, X0, _, _ = problem.make_batch(1, N, 0.6, seed=20211)
def run(lib_path):
    L = capi.LandingLib(N, 0, lib_path=lib_path)
    o = L.default_opts(); o.max_iter = K
    L.solve_host(P, X0, o)
    return L.debug_workspace(1)[0], L
a, L = run(None); b, _ = run(sys.argv[1])
layout = L.workspace_offsets()      # the one description of carve() for Python (capi.workspace_offsets)
assert layout["total"] == len(a) == len(b), (layout["total"], len(a), len(b))
for nm, part in layout.items():
    if nm == "total":
        continue
    off, sz = part
    da, db = a[off:off + sz], b[off:off + sz]
    with np.errstate(all='ignore'):
        bad = ~(np.isclose(da, db, rtol=1e-9, atol=1e-12) | (np.isnan(da) & np.isnan(db)))
    print('%-5s size %6d  differing %6d  first %s' % (nm, sz, bad.sum(), np.nonzero(bad)[0][:6].tolist()))
print('exit record', dict(zip(capi.EXIT_RECORD, a[layout["rec"][0]:])), '|', dict(zip(capi.EXIT_RECORD, b[layout["rec"][0]:])))
print('total', layout['total'], len(a))
