"""CPU test (no GPU): rearranging the memory accesses of the phases between the two sweeps does not change a bit of the iterates, nor one
of the sweep counters, nor the path a single step takes through the line search.

The derivative phase of landing_ipm_kernel reads the multipliers of the J^T y task and of the two Hessian tasks from a copy in LDS that all
256 threads write at the top of the iteration (boundary rows at 0..35, stage k at 36 + 105 k, laid over [G | P | A1 | A^], which are dead
there) at horizons up to 44; longer horizons read the workspace as before.  Operands, operations and the association of every sum are what
they were, so the host emulation of the kernel (tests/emu) must reproduce what the emulation of the commit BEFORE the change computed
(tests/golden/between_sweeps_parent.npz, tests/make_golden_between_sweeps.py): x, f, lam_g, iters, status, kkt, the sweep counters and the
accept counters, np.array_equal, for every member of every case.  N = 2, 3, 5 (running cost), 6: four members; N = 44 and 45, the two sides
of the copy's limit: two members.  The feasibility phase is on and the iteration limit low, so the members go on inside the phase; a stale
or misplaced multiplier there or in a back-tracked iteration would show as it does anywhere else.
By the emulation's own accept counters the cases together take a fused first trial by the swap, back-track a line search, accept with the
slack correction and step inside the feasibility phase; the test asserts that, so it cannot silently stop covering them.
(That the device reads the LDS slots the copy wrote is tests/test_gpu_solver_between_sweeps.py.)"""
import numpy as np
import pytest

from emu_support import build_emu
import make_golden_between_sweeps as rec


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


@pytest.fixture(scope="module")
def golden():
    return np.load(rec.GOLDEN)


def test_the_cases_are_the_ones_the_fixture_was_recorded_for(golden):
    assert {name: c[0] for name, c in rec.CASES.items()} == {"n2": 2, "n3": 3, "n5rc": 5, "n6": 6, "n44": 44, "n45": 45}
    assert rec.CASES["n5rc"][3] is rec.RC and all(c[3] is None for n, c in rec.CASES.items() if n != "n5rc")
    assert all(c[2] == (2 if c[0] >= 44 else 4) for c in rec.CASES.values())
    total = sum(golden[name + "_acc"].sum(axis=0) for name in rec.CASES)
    print("accept counters of the parent over all cases (swap, swap under the clip rule, first trial rejected, back-tracked, slack correction, fallback, phase):", total.tolist())
    for what, slots in rec.COVER.items():
        assert total[list(slots)].sum() > 0, "no case of the fixture shows a " + what


@pytest.mark.parametrize("name", list(rec.CASES))
def test_between_sweeps_equals_the_parent_bit_for_bit(emu_lib, golden, name):
    B = rec.CASES[name][2]
    out, cov, acc = rec.run_case(emu_lib, name)
    print(name, "status", out["status"], "iters", out["iters"], "sweeps", cov[:, 0].tolist(), "accepts", acc.tolist())
    for k in rec.KEYS:
        want = golden[name + "_" + k]
        assert out[k].shape == want.shape and out[k].shape[0] == B, k
        for m in range(B):      # every member, every field
            assert np.array_equal(out[k][m], want[m]), "%s: %s of member %d differs" % (name, k, m)
    assert np.array_equal(cov, golden[name + "_cov"]), "sweeps / eliminations attempted / succeeded differ from the parent's"
    assert np.array_equal(acc, golden[name + "_acc"]), "the steps took other paths through the line search than the parent's"
    assert (out["iters"] >= 1).all() and (cov[:, 0] >= 1).all(), "the members took no steps"
