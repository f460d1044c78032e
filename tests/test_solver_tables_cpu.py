"""CPU test (no GPU): the tables the host hands the solver kernel are, byte for byte, the ones it handed before build_tables was rewritten.

landing_debug_solver_tables returns what a context holds for the kernel: ctab / ccomb / ctype with c_ml and c_mid (assembly of a stage inside
the backward sweep) and rterm with rlen (row products).  tests/golden/solver_tables_parent.npz (tests/make_golden_solver_tables.py) holds
their SHA-256, byte lengths and the ints, and ctype in full, recorded from the emulation library of the commit BEFORE the rewrite.  Every case
and every table is compared -- none is skipped: the short horizons (2 and 3 stage types, the first middle stage, the first c_mid = 1), the
long ones (rterm's 16-bit fields) and the two running-cost forms."""
import numpy as np
import pytest

from emu_support import build_emu
import make_golden_solver_tables as rec


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu()


@pytest.fixture(scope="module")
def golden():
    return np.load(rec.GOLDEN)


@pytest.mark.parametrize("name", list(rec.CASES))
def test_tables_equal_the_parents_byte_for_byte(emu_lib, golden, name):
    got = rec.record(emu_lib, name)
    print(name, {k: int(got[k]) for k in rec.SCALARS}, {k: int(got[k + "_bytes"]) for k in rec.TABLES})
    rec.assert_equals_fixture(got, golden, name)


def test_the_cases_are_what_they_are_there_for(golden):
    ntypes = {n: len(set(golden[n + "_ctype"].tolist())) for n in rec.CASES}
    assert ntypes["n2"] == 2 and ntypes["n3"] == 3 and golden["n2_c_mid"] == 0 and golden["n3_c_mid"] == 0
    assert golden["n4_c_mid"] == 0 and golden["n6_c_mid"] == 1
    for a, b in (("n4", "n20"), ("n20", "n40"), ("n40", "n96")):      # ctab / ccomb are those of the stage types: the same from N = 4 on
        assert golden[a + "_ctab_sha256"] == golden[b + "_ctab_sha256"] and golden[a + "_ccomb_sha256"] == golden[b + "_ccomb_sha256"]
        assert golden[a + "_rterm_sha256"] != golden[b + "_rterm_sha256"]
    assert golden["rc20_ctab_sha256"] != golden["n20_ctab_sha256"]
