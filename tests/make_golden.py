#!/usr/bin/env python3
"""Generate tests/golden/* from the REFERENCE itself (run in the build container only).

Sources (all under /root/reference, never copied into the repo):
  * oracle/_ref/liblanding_ref.so  = optimizations/landing/codegen_casadi/landingCtrller_IPOPT.c
    compiled by oracle/Makefile; called through its CasADi external ABI -> n20_eval.npz, n20_ref_seeded.npz,
    n20_patterns.npz (casadi_s4/casadi_s5 via nlp_*_sparsity_out).
  * optimizations/landing/test_scripts/1.5msDrop30Pitch.mat (X_star, U_star) -> n20_golden_1p5ms30pitch.npz
  * optimizations/landing/data/*.mat (stored N=40 SRBM-CCC solutions)        -> n40_golden.npz
The fixtures are data (inputs + the reference's outputs); this script is committed with them.
"""
import importlib
import json
import os
import sys

import numpy as np
import scipy.io as sio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.oracle import RefOracle, build  # noqa: E402

lc_problem = importlib.import_module("landing-controller_amd.problem")
lc_const = importlib.import_module("landing-controller_amd.constants")
REF = "/root/reference/optimizations/landing"
OUT = os.path.join(ROOT, "tests", "golden")


def ref_seeded(R):
    """n20_ref_seeded.npz: the reference's outputs on the seeded random draws of tests/test_oracle.py (seed 7, lam_f 1.3)"""
    rng = np.random.default_rng(7)
    out = {}
    for i in range(3):
        x = rng.normal(size=R.nx) * 0.7
        p = rng.uniform(0.3, 2.0, size=R.np_)
        lam = rng.normal(size=R.ng)
        _, _, gx, gp = R.grad(x, p, 1.3, lam)
        for k, v in dict(x=x, p=p, lam_g=lam, g=R.g(x, p), jac=R.jac_g(x, p)[1], hess=R.hess_l(x, p, 1.3, lam), grad_gamma_x=gx, grad_gamma_p=gp).items():
            out[f"c{i}_{k}"] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, "n20_ref_seeded.npz"), **out)


def realistic_p20(q_init, qd_init, q_term_ref, QN, mu, l_leg_max, f_max, q_min_z, q_term_min_z, dt=0.03):
    N = 20
    mass, Ib, Ib_inv = lc_const.robot_constants()
    Xref = np.zeros((12, N + 1))
    for i in range(6):
        Xref[i] = np.linspace(q_init[i], q_term_ref[i], N + 1)
        Xref[6 + i] = np.linspace(qd_init[i], 0.0, N + 1)
    return lc_problem.pack_params(
        N, Xref, np.full(N, dt), [-10, -10, q_min_z, -10, -10, -10], [10, 10, 1.0, 10, 10, 10],
        [-10, -10, -10, -40, -40, -40], [10, 10, 10, 40, 40, 40], q_init, qd_init,
        [-10, -10, q_term_min_z, -0.1, -0.1, -10], [10, 10, 5, 0.1, 0.1, 10],
        [-10, -10, -10, -40, -40, -40], [10, 10, 10, 40, 40, 40], QN, mu, l_leg_max, f_max, mass, Ib, Ib_inv)


def main():
    build()
    os.makedirs(OUT, exist_ok=True)
    R = RefOracle()
    rng = np.random.default_rng(20211)

    # ---- patterns -----------------------------------------------------------------
    _, _, ci5, r5 = R.sparsity("nlp_jac_g", "out", 1)
    _, _, ci4, r4 = R.sparsity("nlp_hess_l", "out", 0)
    np.savez_compressed(os.path.join(OUT, "n20_patterns.npz"), jac_colind=ci5, jac_row=r5, hess_colind=ci4, hess_row=r4)

    # ---- golden N=20 trajectory ---------------------------------------------------
    d = sio.loadmat(f"{REF}/test_scripts/1.5msDrop30Pitch.mat", squeeze_me=True)
    Xs, Us = d["X_star"], d["U_star"]
    xg = np.concatenate([Xs.flatten(order="F"), Us.flatten(order="F")])
    pg = realistic_p20(Xs[:6, 0], Xs[6:, 0], [0, 0, 0.2, 0, 0, 0], [0, 0, 100, 100, 100, 0, 10, 10, 10, 10, 10, 10],
                       0.75, 0.4, 500.0, 0.075, 0.15)
    np.savez_compressed(os.path.join(OUT, "n20_golden_1p5ms30pitch.npz"), x=xg, p=pg, f_ref=R.f(xg, pg), g_ref=R.g(xg, pg))

    # ---- seeded evaluation cases ---------------------------------------------------
    cases = []
    # 0: generic random point (exercises every term)
    cases.append((rng.normal(size=R.nx) * 0.5, rng.uniform(0.5, 1.5, size=R.np_)))
    # 1: the golden trajectory, realistic p
    cases.append((xg.copy(), pg.copy()))
    # 2: steep pitch (near the Euler singularity region the callers sample, +-60 deg), perturbed refs
    q0 = np.array([0, 0, 0.62, 0.2, -np.pi / 3, -0.2]); qd0 = np.array([0.4, -0.3, 0.5, 0.8, -0.9, -4.0])
    p2, x2, _, _ = None, None, None, None
    p2 = realistic_p20(q0, qd0, [0, 0, 0.25, 0, 0, 0], [0, 0, 100, 10, 10, 0, 10, 10, 10, 10, 10, 10], 0.75, 0.4, 500.0, 0.075, 0.15)
    Xref = p2[:252].reshape(12, 21, order="F")
    Uref = np.zeros((24, 20))
    for k in range(20):
        Rm = lc_problem.rpy_to_rot_xyz(Xref[3:6, k])
        for leg in range(4):
            Uref[3 * leg:3 * leg + 3, k] = Xref[0:3, k] + Rm @ (lc_problem.SIDE_SIGN[3 * leg:3 * leg + 3] * np.array([0.2, 0.2, -0.3]))
        Uref[12:, k] = rng.uniform(-20, 60, size=12)
    x2 = np.concatenate([Xref.flatten(order="F"), Uref.flatten(order="F")]) + rng.normal(size=R.nx) * 0.02
    cases.append((x2, p2))
    out = {}
    for i, (x, p) in enumerate(cases):
        lam = rng.normal(size=R.ng)
        lam_f = float(rng.uniform(0.5, 2.0))
        f, gf = R.grad_f(x, p)
        g, jac = R.jac_g(x, p)
        hess = R.hess_l(x, p, lam_f, lam)
        _, _, gx, gp = R.grad(x, p, lam_f, lam)
        for k, v in dict(x=x, p=p, lam_g=lam, lam_f=lam_f, f=f, grad_f=gf, g=g, jac=jac, hess=hess, grad_gamma_x=gx, grad_gamma_p=gp).items():
            out[f"c{i}_{k}"] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, "n20_eval.npz"), **out)
    ref_seeded(R)

    # ---- N=40 stored solutions (feasibility goldens) ----------------------
    files = ["attitude_tilt_None", "pitch_0_vX", "pitch_30_vX", "pitch_45_vX", "pitch_60_vX", "pitch_45_vY", "vZ_-3_roll", "vZ_-3_vX", "vZ_-3_vY"]
    xs, names = [], []
    for fn in files:
        dd = sio.loadmat(f"{REF}/data/{fn}.mat", squeeze_me=True, struct_as_record=False)["opt_sol"]
        sols = np.atleast_1d(dd)
        pick = [0, len(sols) - 1] if len(sols) > 1 else [0]
        for j in pick:
            s = sols[j]
            U = np.vstack([s.p_star, s.f_star])
            xs.append(np.concatenate([s.X_star.flatten(order="F"), U.flatten(order="F")]))
            names.append(f"{fn}[{j}]")
    np.savez_compressed(os.path.join(OUT, "n40_golden.npz"), x=np.array(xs), names=np.array(names))

    # ---- constants -------------------------------------------------------------------
    mass, Ib, Ib_inv = lc_const.robot_constants()
    with open(os.path.join(OUT, "constants.json"), "w") as fh:
        json.dump({"mass": mass, "Ib": Ib.tolist(), "Ib_inv": Ib_inv.tolist(),
                   "survey_a15": {"mass": 8.252, "Ib": [0.0575773, 0.2340090, 0.2796738], "Ib_inv": [17.37747, 4.27334, 3.57755]}}, fh, indent=1)
    for fn in sorted(os.listdir(OUT)):
        print(fn, os.path.getsize(os.path.join(OUT, fn)))


if __name__ == "__main__":
    main()
