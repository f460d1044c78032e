"""CPU test (no GPU): the resident stage loop of the backward sweep does not change a bit of the iterates, nor one of its counters.

riccati_backward eliminates the last stage out of line and runs the stages N - 2 .. 0 in ONE loop with the elimination inlined; the lane
constants (columns, LDS bases, masks) are formed once per sweep, the record base, delta_w, the assembly context and the loop condition are
uniform values, and the profile timers live in a second instance of the loop.  Operands, operations and their order are what they were, so
the host emulation of the kernel (tests/emu) must reproduce what the emulation of the commit BEFORE the change computed
(tests/golden/stage_loop_parent.npz, tests/make_golden_stage_loop.py): x, lam_g, iters, status, kkt and the sweep counters, np.array_equal,
for every member of every case.  The cases are the shortest loops: N = 2 (the last stage plus one trip of the loop), N = 4, and N = 5 with
the running cost; all stop at an iteration limit of 16.

What the cases are there for is asserted from the run's own counters (make_golden_stage_loop.abandoned): every member of n2 abandons sweeps
at the LAST stage (each abandoned sweep attempted exactly one elimination: partial == F < 2 F) and retries with a larger delta_w; members
of n4 abandon sweeps INSIDE the loop ((partial - F) % N != 0: eliminations that ones and N + 1s cannot add up to).  A sweep abandoned at
the foot block of stage 0 (partial > N F) does not occur within 16 iterations of these members and is not asserted.
Both instances of the loop are run: with the profile buffer set (timed) and unset, with equal outputs."""
import numpy as np
import pytest

from emu_support import build_emu
import make_golden_stage_loop as rec


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


@pytest.fixture(scope="module")
def golden():
    return np.load(rec.GOLDEN)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_stage_loop_equals_the_parent_sweep_bit_for_bit(emu_lib, golden, name):
    N, _, B, _ = rec.CASES[name]
    out, cov = rec.run_case(emu_lib, name)
    F, part = rec.abandoned(cov, N)
    print(name, "status", out["status"], "iters", out["iters"], "sweeps", cov[:, 0].tolist(), "abandoned", F.tolist(), "partial", part.tolist())
    for k in rec.KEYS:
        want = golden[name + "_" + k]
        assert out[k].shape == want.shape and out[k].shape[0] == B, k
        for m in range(B):      # every member, every field
            assert np.array_equal(out[k][m], want[m]), "%s: %s of member %d differs" % (name, k, m)
    assert np.array_equal(cov, golden[name + "_cov"]), "sweeps / eliminations attempted / succeeded differ from the parent's"
    # the untimed instance of the loop (no profile buffer) computes the same
    plain, _ = rec.run_case(emu_lib, name, profile=False)
    for k in rec.KEYS:
        assert np.array_equal(plain[k], out[k]), "%s: %s differs between the timed and the untimed loop" % (name, k)
    # what the case is there for, from the run's own counters
    assert (F >= 0).all() and (part >= F).all() and (part <= (N + 1) * F).all()
    assert (cov[:, 0] - F >= out["iters"] - 1).all(), "fewer complete sweeps than steps"
    if name == "n2":
        assert (F > 0).all() and (part < 2 * F).all(), "no sweep abandoned at the last stage"
        assert (cov[:, 0] > out["iters"]).all(), "no delta_w retry"
    if name == "n4":
        assert (F > 0).all(), "no abandoned sweep"
        assert ((part - F) % N != 0).any(), "no sweep abandoned inside the stage loop"
        assert (cov[:, 0] > out["iters"]).all(), "no delta_w retry"
