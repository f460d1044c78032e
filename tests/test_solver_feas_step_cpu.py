"""CPU tests (host emulation, tests/emu) of the Newton step landing_ipm_kernel takes INSIDE its feasibility phase, and of what it does with it: the state the phase
starts from, the step (dx, ds, equality multipliers), the update of s, n, q and of the four bound multipliers per row, and the two step lengths -- against
tests/elastic_newton_reference.py, one sparse unsymmetric solve of the elastic problem's full primal-dual system that shares nothing with the kernel's row elimination
(el_step / el_point_side: sigma = z / D), condensation and Riccati sweep.  tests/feas_step_harness.py has the construction and the tolerances (none fitted: the step keeps
newton_reference's 16 x, everything else is that bound propagated through the row's linear dependence on ds, plus 4 eps of the terms).

A solve is stopped inside the phase with landing_debug_iter_cap (include/landing_nlp.h): max_iter = M, feas_phase = 1, feas_jam = 0, cap = M + 1 + j stops after j steps
of the phase; runs j and j + 1 share their trajectory.  THE PHASE ENDS AT ITERATION 2 M (lim = it + max_iter at the entry, which the cap does not lift), so a run with
max_iter = M holds the pairs (j, j + 1) with M + 2 + j <= 2 M only: M = 2 the first step, M = 12 j in {0, 1, 2, 5}; the pairs j = 12 and j = 25 come from M = 27.

Configurations: the N = 20 production grid with the 12 locally infeasible + 4 converging members of tests/test_gpu_certificates.py, feas_rho 1000 and 10; the N = 40
running-cost form (Hc zeroed at the entry, no objective in the terminal stage), members 0..2 of make_batch(16, 40, 0.6, seed 20211).

Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the emulation (bound 16), dx / ds / y:
    named, rho 1000, M = 2      0.13   / 0.13   / 0.028     16 pairs            named, rho 10, M = 2       0.046 / 0.046 / 0.043    16 pairs
    named, rho 1000, M = 12     0.089  / 0.24   / 0.018     64 pairs            named, rho 10, M = 12      0.43  / 1.3   / 0.18     64 pairs
    named, rho 1000, M = 27     0.24   / 0.21   / 0.018     16 pairs (members 0..7; all 16 by hand: 0.24 / 0.21 / 0.074, 27 pairs, 5 skipped)
    running cost, N = 40, M = 2 0.0012 / 0.0012 / 0.0018     3 pairs            running cost, N = 40, M = 12   0.0071 / 0.0073 / 0.0048   12 pairs
No pair is skipped in the committed cases.  With all 16 named members at M = 27 (by hand, and on the device) the four CONVERGING members skip 5 pairs: (100000, 0) at j = 12 and
all four at j = 25 have been handed back by the phase (record feas = 0) or have converged (member (100000, 0): status 0 after 48 iterations); all twelve locally
infeasible members contribute a checked pair at j = 25.  Normwise backward error of the kernel's step (printed with -s): <= 3.4e-17.
The ratios are small because the yardsticks are large: the full elastic system is worse conditioned than the normal iteration's (rho / mu across its rows), and an
unrefined LU of it errs by 1e-11 .. 1e-9 where the kernel, which eliminates every row exactly, errs by 1e-13 .. 1e-12.  The device's figures are in
tests/test_gpu_solver_feas_step.py.

What these tests catch (each change applied alone to a scratch copy of the emulation, never committed):
    (a) `sg += z / a` instead of `z / D` in el_point_side          the row-algebra check (sigma) and EVERY step test run on it (named rho 1000 M = 2, 12, 27: dx off by 1e-2 .. 1)
    (b) the sign of sd in `rh` flipped for the upper side             the row-algebra check (rho) and every step test run on it (the same three; dx off by 0.1 .. 1)
    (c) `S.ks.feas ? 0.0 :` removed from qn2 (terminal stage)         every step test run on it: named rho 1000 M = 2, 12, 27 and the running-cost form (dx off by 1e-2 .. 0.1)
    (d) Hc not zeroed at the entry                                    the running-cost test (dx off by 1e-4 against a bound of 3e-11); the plain-form tests do not run that line
    (e) `n * rn` dropped from el_step                                 the row-algebra check ONLY (dz off by 9.9); named rho 1000 M = 12 and rho 10 M = 12 PASS -- as expected: the update
                                                                      keeps z + w = rho, so rn is rounding on a trajectory
(run on: (a), (b) row algebra + named rho 1000 M in {2, 12, 27}; (c) those three step tests + running cost; (d) running cost; (e) row algebra + named M = 12 at both rho.)
"""
import ctypes as C

import numpy as np
import pytest

import elastic_newton_reference as er
import feas_step_harness as F
import solver_step_harness as H
from conftest import lc
from emu_support import build_emu

EPS = np.finfo(float).eps
ALL16 = list(range(16))


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


def test_row_algebra_against_a_dense_solve(emu_lib):
    """el_step and el_point_side on their own (landing_emu_el_row, emulation build only) against the three equations of a side solved densely in np.longdouble, at 1000
    random positive states with z + w != rho: the update keeps z + w = rho unless the band clamps, so a trajectory hardly ever exercises the n (z + w - rho) term.
    Tolerance: 64 eps of the sum of the absolute terms of each output's closed formula (elastic_newton_reference.row_algebra_dense).  Worst measured: 2.4 eps (rho; dz 2.1, the others <= 1.6).
    Against the condition sums |A^-1| |r| of the dense solve -- printed, not asserted -- the closed formula loses up to 7e12 eps (dn; dw 9e7, da 5e12; dz, sigma, rho as above): it divides by w first, which is not
    backward stable at states with w << z; the solvers' trajectories stay far from those (the update checks of this file hold 4 eps of the terms there)."""
    lib = lc("capi").load(emu_lib)
    rng = np.random.default_rng(5)
    worst, wcond = {}, {}
    for i in range(1000):
        a, n = 10.0 ** rng.uniform(-6, 2, 2); z, w = 10.0 ** rng.uniform(-6, 3, 2)
        mu = 10.0 ** rng.uniform(-8, 0); rho = (10.0, 1000.0)[i % 2]; ds = (-1.0) ** rng.integers(2) * 10.0 ** rng.uniform(-6, 1); sd = (1.0, -1.0)[(i // 2) % 2]
        assert abs(z + w - rho) > 1e-3
        out = (C.c_double * 6)()
        lib.landing_emu_el_row(sd, a, n, z, w, mu, rho, ds, out)
        val, mag, cond = er.row_algebra_dense(sd, a, n, z, w, mu, rho, ds)
        for k, got in zip(("dz", "dw", "dn", "da", "sig", "rho"), out):
            d = abs(np.longdouble(got) - val[k])
            e = float(d / (EPS * mag[k])); worst[k] = max(worst.get(k, 0.0), e); wcond[k] = max(wcond.get(k, 0.0), float(d / (EPS * cond[k])))
            assert e <= 64.0, (i, k, got, float(val[k]), e, dict(sd=sd, a=a, n=n, z=z, w=w, mu=mu, rho=rho, ds=ds))
    print("row algebra: worst error in eps of the term sums", {k: round(v, 2) for k, v in worst.items()}, "| in eps of the condition sums", {k: float("%.3g" % v) for k, v in wcond.items()})


def _js(M):
    return F.pairs_within(M) if M < 27 else [12, 25]


# (rho, M, members of the batch of 16): the emulation runs ~4 iterations a second at N = 20, so the long runs (M = 27: up to 54 iterations, six caps) take the first eight
# of the twelve locally infeasible members only; the device tests run all 16 (M = 27 at rho = 1000 only: at rho = 10 the phase hands most members back before step 25)
NAMED_CASES = [(1000.0, 2, ALL16), (1000.0, 12, ALL16), (1000.0, 27, ALL16[:8]), (10.0, 2, ALL16), (10.0, 12, ALL16)]


@pytest.mark.parametrize("case", NAMED_CASES, ids=["rho%g-M%d" % c[:2] for c in NAMED_CASES])
def test_phase_steps_of_the_named_members(emu_lib, tmp_path, case):
    """N = 20 production grid, the 12 + 4 named members: entry state (j = 0), first step, and the pairs (j, j + 1), j in {1, 2, 5} (M = 12) and {12, 25} (M = 27).
    Conditions: every skip is printed with its reason; at most one pair in five is skipped per configuration; at least six locally infeasible members contribute a
    checked pair at j = 25 (emulation, all twelve run once by hand: all twelve do)."""
    from oracle.oracle import Oracle
    rho, M, members = case
    N = 20
    O = Oracle(N)
    P, X0, runs = F.emu_runs_parallel(dict(N=N, batch="named", form="plain"), members, {M: F.caps_of(M, _js(M))}, tmp_path, rho=rho)
    L = lc("capi").LandingLib(N, lib_path=emu_lib)
    res = F.check_config(O, P, F.feas_opts(L, M, rho), M, _js(M), runs[M], "named rho %g M %d" % (rho, M))
    L.close()
    total = res["checked"] + len(res["skipped"])
    assert total == len(members) * len(res["by_j"]) and len(res["skipped"]) * 5 <= total, (M, res["skipped"])
    if M == 27:
        assert len(res["by_j"][25]) >= 6, res["by_j"]


def test_phase_steps_of_the_running_cost_form(emu_lib, tmp_path):
    """N = 40, running-cost form, members 0..2, M in {2, 12}: the entry zeroes the constant running-cost Hessian Hc and the terminal stage carries no objective"""
    from oracle.oracle import Oracle
    N = 40
    O = Oracle(N, run_cost=H.RUN_COST)
    spec = dict(N=N, batch=dict(seed=20211, B=16), form="rc")
    plan = {M: F.caps_of(M, F.pairs_within(M)) for M in (2, 12)}
    P, X0, runs = F.emu_runs_parallel(spec, [0, 1, 2], plan, tmp_path)
    L = lc("capi").LandingLib(N, lib_path=emu_lib, run_cost=H.RUN_COST)
    for M in (2, 12):
        res = F.check_config(O, P, F.feas_opts(L, M), M, F.pairs_within(M), runs[M], "rc N 40 M %d" % M)
        total = res["checked"] + len(res["skipped"])
        assert total == 3 * len(res["by_j"]) and len(res["skipped"]) * 5 <= total, (M, res["skipped"])
    L.close()
