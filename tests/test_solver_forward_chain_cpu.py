"""CPU test (no GPU): taking LDS round trips off the forward recursion and the assembly hooks does not change a bit of the iterates, nor
one of the sweep counters.

forward_pass forms its lane constants and the record base once per sweep, reads the bias of a row with the row and turns the two cases of a
row (state row / c+ row, 0 behind the last stage) into selects; the assembly hooks of the backward sweep fetch their term and combine words
one block step early and store b and the gradient of the running cost there; the 8-lane sum goes through lane_sum8_head (DPP on the
device, __shfl_xor in this emulation).  Operands, operations and the association of every sum
are what they were, so the host emulation of the kernel (tests/emu) must reproduce what the emulation of the commit BEFORE the change
computed (tests/golden/forward_chain_parent.npz, tests/make_golden_forward_chain.py): x, lam_g, iters, status, kkt and the sweep counters,
np.array_equal, for every member of every case.  The horizons N = 2, 3, 5 (running cost) and 6 are no multiples of the forward loop's
unroll factor 4: they run its clamped prefetches and its `k < N` guards; four members, 12 iterations each.
Both instances of the backward loop are run: with the profile buffer set (timed) and unset, with equal outputs.
(The DPP controls themselves exist on the device only: tests/test_gpu_solver_forward_chain.py.)"""
import numpy as np
import pytest

from emu_support import build_emu
import make_golden_forward_chain as rec


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


@pytest.fixture(scope="module")
def golden():
    return np.load(rec.GOLDEN)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_forward_chain_equals_the_parent_bit_for_bit(emu_lib, golden, name):
    N, _, B, _ = rec.CASES[name]
    assert N % 4 != 0 and B == 4 and rec.LIMIT == 12
    out, cov = rec.run_case(emu_lib, name)
    print(name, "status", out["status"], "iters", out["iters"], "sweeps", cov[:, 0].tolist(), "attempted", cov[:, 1].tolist(), "ok", cov[:, 2].tolist())
    for k in rec.KEYS:
        want = golden[name + "_" + k]
        assert out[k].shape == want.shape and out[k].shape[0] == B, k
        for m in range(B):      # every member, every field
            assert np.array_equal(out[k][m], want[m]), "%s: %s of member %d differs" % (name, k, m)
    assert np.array_equal(cov, golden[name + "_cov"]), "sweeps / eliminations attempted / succeeded differ from the parent's"
    assert (out["iters"] >= 1).all() and (cov[:, 0] >= out["iters"] - 1).all(), "the members took no steps: the forward recursion did not run"
    # the untimed instance of the backward loop (no profile buffer) computes the same
    plain, _ = rec.run_case(emu_lib, name, profile=False)
    for k in rec.KEYS:
        assert np.array_equal(plain[k], out[k]), "%s: %s differs between the timed and the untimed loop" % (name, k)
