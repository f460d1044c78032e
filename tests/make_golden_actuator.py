"""Writes tests/golden/actuator_audit_emu.npz: the outputs of landing_actuator_audit_batch on the HOST EMULATION (tests/emu) for the cases below, which the
GPU suite holds the product library against (tests/test_gpu_actuator_audit.py) and the CPU suite holds the emulation against
(tests/test_actuator_audit_cpu.py, bit for bit: a change of the kernel that changes a number shows there first).  Inputs are rebuilt from seeds
(tests/actuator_reference.py), only outputs are stored.  Run:  python tests/make_golden_actuator.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import actuator_reference as ar      # noqa: E402
from emu_support import emu_landing_lib      # noqa: E402

CASES = {"stored": 20, "n2": 2, "n3": 3, "n20": 20, "n64": 64}      # name -> N


def case_inputs(case, golden):
    """-> N, x [B, 48N+12], dt, dt_stride: the seven stored solutions on the production grid, or three random members with a grid each"""
    N = CASES[case]
    if case == "stored":
        return N, ar.stored_solutions(golden), ar.PRODUCTION_DT.copy(), 0
    return N, ar.random_states(N, 3, seed=500 + N), ar.random_dt(N, 3, seed=600 + N), N


def emulation_outputs(case, golden, libs=None):
    """the case through the emulated library -> dict of tau, jvel, volt, summary, where, ok"""
    import importlib
    N, x, dt, stride = case_inputs(case, golden)
    L = emu_landing_lib(N)
    R = importlib.import_module("landing-controller_amd.rbd").Rbd(L)
    B = x.shape[0]
    o = dict(tau=np.zeros((B, N, 12)), jvel=np.zeros((B, N, 12)), volt=np.zeros((B, N, 12)), summary=np.zeros((B, 8)), where=np.zeros((B, 4), np.int32), ok=np.zeros(B, np.int32))
    a = lambda k: o[k].ctypes.data
    R.actuator_audit_device(B, dt.ctypes.data, stride, x.ctypes.data, a("summary"), a("where"), a("ok"), d_tau=a("tau"), d_jvel=a("jvel"), d_volt=a("volt"))
    L.close()
    return o


if __name__ == "__main__":
    golden = os.path.join(HERE, "golden")
    out = {}
    for case in sorted(CASES):
        out.update({case + "_" + k: v for k, v in emulation_outputs(case, golden).items()})
    np.savez_compressed(os.path.join(golden, "actuator_audit_emu.npz"), **out)
    print("wrote", len(out), "arrays")
