"""Writes the reference-held kinodynamic fixtures as plain arrays.  Data only; run in the build container where /root/reference exists:
python tests/make_golden_n1.py

tests/golden/n1_kinodyn_solutions.npz: the two kinodynamic solutions the reference keeps beside its test scripts
(optimizations/landing/test_scripts/1.5msDrop30Pitch.mat and prevSoln.mat: X_star [12, 21], U_star [24, 20] = [c; f], jpos_star [12, 20]),
tags a and b, both on the uniform grid dt = 0.03.

tests/golden/n1_kinodyn_multipliers.npz: X_star, U_star, jpos_star and KNITRO's own multipliers lam_g_star [2844] (= ng of 20 intervals;
landing_optimization.m:386,395) of
  tag m  optimizations/landing/main_scripts/prevSoln.mat     -- a solve of the production problem (production grid, mu 0.75) to KNITRO's
         default tolerances: the pin of tests/test_kd_multipliers_cpu.py
  tag g  optimizations/landing/generate_solver/prevSoln.mat  -- stopped at feastol 1e-4 / 4 s wall clock: a feasibility fixture only.

A file whose stored arrays already equal the reference's is left untouched (an npz carries the time it was written)."""
import os

import numpy as np
import scipy.io as sio

REF = "/root/reference/optimizations/landing"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _write(name, out):
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        with np.load(path) as old:
            if sorted(old.files) == sorted(out) and all(old[k].dtype == out[k].dtype and np.array_equal(old[k], out[k]) for k in out):
                return
    np.savez(path, **out)


out = {}
for tag, name in (("a", "1.5msDrop30Pitch.mat"), ("b", "prevSoln.mat")):
    d = sio.loadmat(os.path.join(REF, "test_scripts", name))
    out["X_" + tag], out["U_" + tag], out["J_" + tag] = d["X_star"], d["U_star"], d["jpos_star"]
_write("n1_kinodyn_solutions.npz", out)

out = {}
for tag, folder in (("m", "main_scripts"), ("g", "generate_solver")):
    d = sio.loadmat(os.path.join(REF, folder, "prevSoln.mat"))
    out["X_" + tag], out["U_" + tag], out["J_" + tag], out["lam_" + tag] = d["X_star"], d["U_star"], d["jpos_star"], d["lam_g_star"][:, 0]
_write("n1_kinodyn_multipliers.npz", out)
