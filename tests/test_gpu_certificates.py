"""GPU tests of what LANDING_INFEASIBLE claims (run with -m gpu): a KKT point of the elastic problem with positive violation (include/landing_nlp.h) -- held to
those conditions with the multipliers the kernel returns, by tests/certificate_reference.py (bounds derived from the stop test, none fitted to a solver)."""
import numpy as np
import pytest

import certificate_reference as cr
from conftest import lc

pytestmark = pytest.mark.gpu
KKT_TOL = 1e-6
N = 20
# members of the reference's production problem (data-generation law) that the CPU port certifies locally infeasible (tests/test_certificates_cpu.py) ...
NAMED = [(100000, m) for m in (40, 120, 131, 154, 252, 592)] + [(3, m) for m in (7, 63, 76, 95, 187, 189)]
CONVERGING = [(100000, m) for m in (0, 1, 2, 3)]      # ... and four that it solves


def test_named_certificates_are_elastic_kkt_points_and_reproducible(oracle_mod):
    """The 12 members the CPU port certifies + 4 it solves, ONE batch of 16 through landing_ipm_kernel (N = 20, max_iter 300, default options):
    every member ends with status 0, 3 or 4; every converged member is a KKT point <= 1e-6 under the oracle; EVERY certificate passes the six residuals of
    the elastic problem's KKT conditions (rho, tol, feas_cert from the options struct) and reports kkt[1] <= tol; at least 6 of the 12 named members are
    certificates (the port: 12 of 12 -- the kernel's rounding may take single members down another path, tests/test_solver_cpu.py on member 40);
    the same batch a second time gives identical bits.
    MI355X: 12 of the 12 named members certified (146 .. 372 iterations; member (100000, 40) after 372, the port after 162), the 4 others converge; worst over the 12:
    E 6.4e-7  S 8.3e-8  |lam| <= 1000  rho - |lam| 2.8e-4 (bound on that row 2.8e-3)  C 1.0e-7."""
    Pm = lc("problem")
    O = oracle_mod.Oracle(N)
    batches = {seed: Pm.make_batch(1024, N, 0.6, seed=seed, consts=Pm.production_constants("datagen"), dt_grid="reference", law="datagen")[:2] for seed in (100000, 3)}
    P = np.array([batches[s][0][m] for s, m in NAMED + CONVERGING]); X0 = np.array([batches[s][1][m] for s, m in NAMED + CONVERGING])
    L = lc("capi").LandingLib(N, device=0)
    o = L.default_opts(); o.max_iter = 300
    r = L.solve_host(P, X0, o)
    again = L.solve_host(P, X0, o)
    L.close()
    print("status %s iterations %s" % (r["status"], r["iters"]))
    assert np.isin(r["status"], (0, 3, 4)).all(), r["status"]
    for b in np.nonzero(r["status"] == 0)[0]:
        assert O.kkt(r["x"][b], P[b], r["lam_g"][b]).max() <= KKT_TOL * 1.0001, b
    W = cr.Worst()
    for b in np.nonzero(r["status"] == 3)[0]:
        res = cr.srbm_certificate(O, r["x"][b], P[b], r["lam_g"][b], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=r["kkt"][b, 0])
        print("   %s: %s" % ((NAMED + CONVERGING)[b], {n: "%.2e (%.2e)" % (res[n]["value"], res[n]["bound"]) for n in cr.NAMES}))
        assert cr.failed(res) == [], (b, res)
        assert r["kkt"][b, 1] <= o.tol * 1.0001
        W.add(res)
    print("landing_ipm_kernel, named members:", W)
    assert (r["status"][:12] == 3).sum() >= 6, r["status"]
    for k in ("x", "lam_g", "kkt", "status", "iters", "f"):
        assert np.array_equal(r[k], again[k]), k


def test_short_horizon_certificate_is_an_elastic_kkt_point(oracle_mod):
    """N = 16 on a uniform grid (the batch of test_gpu_solver.py::test_solver_other_horizons_and_limits, which holds one locally infeasible member): default
    options, library defaults for max_iter; the certificate passes the six residuals.  MI355X: 1 certificate, E 2.0e-10  S 1.3e-11  rho - |lam| 6.3e-5  C 1.0e-7."""
    O = oracle_mod.Oracle(16)
    L = lc("capi").LandingLib(16, device=0)
    P, X0, _, _ = lc("problem").make_batch(6, 16, 0.6, seed=4)
    o = L.default_opts()
    r = L.solve_host(P, X0)
    L.close()
    cert = np.nonzero(r["status"] == 3)[0]
    assert len(cert) >= 1, r["status"]
    W = cr.Worst()
    for b in cert:
        res = cr.srbm_certificate(O, r["x"][b], P[b], r["lam_g"][b], o.feas_rho, o.tol, feas_cert=o.feas_cert, kkt0=r["kkt"][b, 0])
        assert cr.failed(res) == [], (b, res)
        assert r["kkt"][b, 1] <= o.tol * 1.0001
        W.add(res)
    print("landing_ipm_kernel, N = 16:", W)
