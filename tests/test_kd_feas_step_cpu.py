"""CPU tests (host emulation, tests/emu) of the Newton step the kinodynamic refinement solver takes INSIDE its feasibility phase (landing_kd_head_kernel: entry, el_init_row,
kd_feas_point_pass; landing_kd_iter_kernel: el_step over the rows, step bounds, the accept pass's multiplier update): entry state, step, update and step lengths against
tests/elastic_newton_reference.py.  The SRBM solver's counterpart is tests/test_solver_feas_step_cpu.py; read its docstring and tests/feas_step_harness.py for the
construction (landing_debug_iter_cap, the pairs a run with max_iter = M can hold) and the tolerances.  J and H of the reference are the product's function layer at the
state (kd_step_harness.check_pair's default; tests/test_kd_step_cpu.py holds that layer against the oracle).

Portfolio off; members of kd_step_harness.emu_member (gentle drops: none is certified by the presolve; one that were would be left out).  The emulation runs this solver
at about one iteration a second at N = 2 and 0.1 at N = 20, so the CPU cases are N = 2 and 3 with M = 12 (entry, first step, j in {1, 2, 5}) and N = 20 with M = 2 (entry
and first step); the later steps of N = 20 (j in {1, 2, 5}) and the pairs j = 12, 25 at N = 2 are on the device (tests/test_gpu_kd_feas_step.py, which also says why
N = 20 holds no pair j = 12 or 25: its members converge before a phase could reach them).  Every emulation run of the file starts at once, one
process per member.

Worst measured ratio error / max(e_aug, e_cond, 1e-15) on the emulation (bound 16), dx / ds / y, none skipped:
    N = 2, M = 12    12.9 / 12.9 / 13.2     (12 pairs; member 0, j = 1: errors of 3e-12 against yardsticks of 2e-13 -- the short horizon of kd_step_harness.SHORT_LATER_FACTOR)
    N = 3, M = 12    0.90 / 0.90 / 0.90     (members 0..2 measured: 12 pairs; the test runs members 0, 1)
    N = 20, M = 2    0.24 / 0.24 / 0.014    (1 pair)
    N = 2, M = 27    0.24 / 0.29 / 0.13     (j in {12, 25}, members 0, 1: 4 pairs; run once by hand, not part of the file: three minutes of emulation)
"""
from concurrent.futures import ThreadPoolExecutor

import pytest

import feas_step_harness as F
import kd_feas_step_harness as KF
import kd_step_harness as KH
from emu_support import build_emu

# (N, M, members)
CASES = [(2, 12, [0, 1, 2]), (3, 12, [0, 1]), (20, 2, [0])]


@pytest.fixture(scope="module")
def emu_runs(tmp_path_factory):
    """case -> (problems, X0, opts, {cap: run}); the six member processes of the file run side by side (the threads only wait for them)"""
    build_emu()
    tmp = tmp_path_factory.mktemp("kd_feas_emu")
    with ThreadPoolExecutor(len(CASES)) as ex:
        out = list(ex.map(lambda c: KF.emu_runs_parallel(c[0], c[2], c[1], F.caps_of(c[1], F.pairs_within(c[1])), tmp), CASES))
    return {c[:2]: r for c, r in zip(CASES, out)}


@pytest.mark.parametrize("case", CASES, ids=["N%d-M%d" % c[:2] for c in CASES])
def test_phase_steps_are_newton_steps_of_the_elastic_problem(emu_runs, case):
    """entry state (j = 0) and the pairs (j, j + 1); a pair is skipped only when the member did not stop at both caps or a record says feas = 0, every skip is printed
    with its reason, at most one pair in five is skipped"""
    N, M, members = case
    js = F.pairs_within(M)
    probs, X0, opts, runs = emu_runs[(N, M)]
    res = KF.check_config(probs, opts, M, js, runs, "kd N %d M %d" % (N, M))
    total = res["checked"] + len(res["skipped"])
    assert len(res["members"]) >= 1 and total == len(res["members"]) * len(js) and len(res["skipped"]) * 5 <= total, res["skipped"]
