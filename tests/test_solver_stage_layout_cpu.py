"""CPU test (no GPU): the operand layout of the backward sweep does not change a bit of the iterates.

block_eliminate reads the condensed stage array in elimination order with gamma as the spare column of G, p as the spare column of P and b
as the spare column of A^, so that every operand fetch is a per-lane base plus a constant; the host's assembly tables write G and gamma
there.  Operands, operations and their order are what they were, so the host emulation of the kernel (tests/emu) must reproduce the
results recorded from the emulation of the commit BEFORE the change (tests/golden/stage_layout_parent.npz, tests/make_golden_stage_layout.py):
x, lam_g, iters, status and kkt, np.array_equal, for every member of every case -- none is skipped.  The cases: a 3-stage horizon (first /
penultimate / last stage type only), a 6-stage horizon stopped at its iteration limit, N = 20 with the defaults, the running-cost form, and
members that enter the feasibility phase.  The counters of the run itself confirm what the cases are there for: sweeps that failed and were
repeated with a larger delta_w (delta sits on the diagonal of the re-laid array) and steps inside the feasibility phase."""
import numpy as np
import pytest

from emu_support import build_emu
import make_golden_stage_layout as rec


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


@pytest.fixture(scope="module")
def golden():
    return np.load(rec.GOLDEN)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_iterates_equal_the_parent_layout_bit_for_bit(emu_lib, golden, name):
    out, cov = rec.run_case(emu_lib, name)
    print(name, "status", out["status"], "iters", out["iters"], "[attempted, succeeded, feasibility steps]", cov.tolist())
    B = rec.CASES[name][2]
    for k in rec.KEYS:
        want = golden[name + "_" + k]
        assert out[k].shape == want.shape and out[k].shape[0] == B, k
        for m in range(B):      # every member, every field
            assert np.array_equal(out[k][m], want[m]), "%s: %s of member %d differs" % (name, k, m)
    # what the case is there for
    if name in ("n20", "rc", "feas", "short"):
        assert (cov[:, 0] > cov[:, 1]).any(), "no sweep failed: the delta_w retry is not exercised"
    if name in ("feas", "short"):
        assert (cov[:, 2] > 0).all(), "a member did not enter the feasibility phase"
    if name == "mid":
        assert (out["status"] == 1).all() and (out["iters"] == 7).all()
