"""Records tests/golden/wb_backtrack.npz: the numpy oracle's (oracle/wb_oracle.py) step lengths and cost histories of the backtracking cases of
tests/wb_reference.py (LOOP_CASES), so that the GPU tests need not run the oracle (25 s per case: Richardson-extrapolated derivatives at every knot).
tests/test_wb_kernels_cpu.py runs the oracle itself and checks that the record still equals it.      python tests/make_golden_wb.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402,F401  (puts the repository root on the path)
import wb_reference as wr  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name, semi in wr.LOOP_CASES:
        al, hist = wr.loop_oracle(wr.LOOP_LISTS[name], semi)
        key = "%s_%s" % (name, "semi" if semi else "expl")
        out[key + "_alpha"], out[key + "_cost"] = al, hist
        print(key, al.tolist())
    np.savez(os.path.join(conftest.GOLDEN, wr.LOOP_GOLDEN), **out)
