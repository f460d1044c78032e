"""GPU test (MI355X): the product library hands the solver kernel the tables the host emulation builds.

The tables hold offsetof values of the kernel's LDS block, so they are the same in both builds only if the host pass of the device compiler
lays that block out as g++ does.  Device counterpart of tests/test_solver_tables_cpu.py, against the same fixture
(tests/golden/solver_tables_parent.npz, recorded from the host emulation): the digests of ctab, ccomb, ctype and rterm as the context holds
them on the device, their lengths and c_ml / c_mid / rlen, for a three-stage horizon, N = 20, and N = 20 with the running cost.
(The product library of the commit the fixture was recorded from gives these digests on the MI355X too, so they have no keys of their own.)"""
import numpy as np
import pytest

import make_golden_solver_tables as rec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", ["n3", "n20", "rc20"])
def test_gpu_tables_equal_the_recorded_ones(name):
    got = rec.record(None, name)      # (the product library)
    print(name, {k: int(got[k]) for k in rec.SCALARS}, {k: int(got[k + "_bytes"]) for k in rec.TABLES})
    rec.assert_equals_fixture(got, np.load(rec.GOLDEN), name)
