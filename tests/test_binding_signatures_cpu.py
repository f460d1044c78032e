"""The ctypes binding against the header it mirrors (no GPU): capi.SIGNATURES has every prototype of include/landing_nlp.h with the same number and
kinds of parameters and the same kind of return value; capi.load alone applies it; the ten struct mirrors equal the header's structs field for field;
and no other module of the package declares a signature.  The header is read by tests/header_decls.py."""
import ctypes as C
import glob
import os
import re

import pytest

import header_decls as H
from conftest import ROOT, lc
from emu_support import EMU_LIB, build_emu

PKG = os.path.join(ROOT, "landing-controller_amd")
MIRRORS = dict(landing_form="LandingForm", landing_solver_opts="SolverOpts", landing_args21="Args21", landing_args25="Args25", landing_rbd_model="RbdModel",
               landing_kinodyn_params="KinodynParams", landing_kinodyn_form="KinodynForm", landing_pipeline_opts="PipelineOpts",
               landing_actuator_model="ActuatorModel", landing_actuator_screen="ActuatorScreen")


def _kind(t):
    """the header_decls kind of a ctypes restype / argtype"""
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return "pointer"
    return {C.c_int: "int", C.c_double: "double", C.c_longlong: "long long"}[t]


def test_parser_reads_every_prototype_of_the_header():
    """the names followed by `(` anywhere in the header (what test_library_exports_every_declared_symbol looks for) are exactly the parsed prototypes"""
    names = set(re.findall(r"\b(landing_[a-z0-9_]+)\s*\(", open(H.HEADER).read()))
    assert set(H.prototypes()) == names and len(names) >= 102
    assert sorted(H.struct_names()) == sorted(MIRRORS)


def test_table_matches_every_prototype():
    table, protos = lc("capi").SIGNATURES, H.prototypes()
    assert sorted(table) == sorted(protos), set(table) ^ set(protos)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert [_kind(t) for t in argtypes] == params, name
        assert _kind(restype) == ret and (ret != "pointer" or restype in (C.c_void_p, C.c_char_p)), name


def test_load_alone_declares_every_entry_point():
    build_emu()
    capi = lc("capi")
    lib = capi.load(EMU_LIB)      # a fresh CDLL: nothing any wrapper class has done to another one shows here
    for name in H.prototypes():
        fn, (restype, argtypes) = getattr(lib, name), capi.SIGNATURES[name]
        assert fn.argtypes is not None and list(fn.argtypes) == argtypes and fn.restype is restype, name
    for name, (restype, argtypes) in capi.EMU_HOOKS.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name
    nx, ng = C.c_longlong(), C.c_longlong()
    for N in (2, 6, 20, 64):      # rbd.py sizes its arrays with kinodyn.dims
        assert lib.landing_kinodyn_nlp_dims(N, C.byref(nx), C.byref(ng)) == 0 and (nx.value, ng.value) == lc("kinodyn").dims(N), N


def _layout(t):
    """(base type, array extents outermost first) of a field's type"""
    ext = []
    while hasattr(t, "_length_"):
        ext.append(t._length_)
        t = t._type_
    return t, ext


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_struct_mirror_equals_the_header(struct):
    capi = lc("capi")
    known = {h: getattr(capi, m) for h, m in MIRRORS.items()}      # a struct inside a struct stands for its own (separately checked) mirror
    want, mirror = H.header_struct(struct, known), known[struct]
    assert [n for n, _ in mirror._fields_] == H._header_fields(struct)
    for (n, t), (_, tw) in zip(mirror._fields_, want._fields_):
        assert _layout(t) == _layout(tw), (struct, n)
    assert C.sizeof(mirror) == C.sizeof(want)
    if struct in ("landing_form", "landing_solver_opts"):
        assert C.sizeof(mirror) == dict(landing_form=320, landing_solver_opts=336)[struct]


def test_signatures_are_declared_in_capi_only():
    pat = re.compile(r"\.argtypes|\.restype")
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        hits = [line.strip() for line in open(path) if pat.search(line)]
        if os.path.basename(path) != "capi.py":
            assert not hits, (path, hits)
            continue
        # the loops of load() over the two tables, and the HIP runtime's own hipMemcpy in the workspace copy
        assert all(h.startswith("fn.restype, fn.argtypes = ") or h.startswith("hip.hipMemcpy.argtypes = ") for h in hits), hits
        assert sum(h.startswith("hip.hipMemcpy") for h in hits) == 1 and len(hits) == 3, hits
