"""What include/landing_nlp.h declares, read with regular expressions (test helper; the package has no header parser): the fields of its
structs and the prototypes of its functions."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "landing_nlp.h")
SCALARS = {"int": C.c_int, "double": C.c_double, "long long": C.c_longlong}


def _source():
    """the header without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _struct_body(struct_name):
    m = re.search(r"typedef struct \{([^{}]*)\} " + struct_name + ";", _source())
    assert m, struct_name
    return m.group(1)


def _fields(struct_name):
    """(field name, base type's name, is a pointer, array extents outermost first) of every field, in order"""
    out = []
    for decl in _struct_body(struct_name).split(";"):
        decl = re.sub(r"\bconst\b", "", decl).strip()
        if decl:
            base, rest = re.match(r"(long long|\w+)\s*(.*)", decl, flags=re.S).groups()
            for v in rest.split(","):
                out.append((re.sub(r"\[.*\]", "", v).strip("* \n"), base, v.strip().startswith("*"), [int(e) for e in re.findall(r"\[(\d+)\]", v)]))
    return out


def _header_fields(struct_name):
    """the field names of a struct, in order"""
    return [f[0] for f in _fields(struct_name)]


def struct_names():
    return re.findall(r"typedef struct \{[^{}]*\} (\w+);", _source())


def header_struct(struct_name, known):
    """a ctypes.Structure built from the header's fields alone: int / double / long long, pointers (`const double *a, *b`), arrays
    (`double E[18][9]`) and structs declared earlier (`known`: name -> class)"""
    fields = []
    for name, base, ptr, extents in _fields(struct_name):
        t = SCALARS.get(base) or known[base]
        t = C.POINTER(t) if ptr else t
        for ext in reversed(extents):
            t = t * ext
        fields.append((name, t))
    return type(struct_name, (C.Structure,), {"_fields_": fields})


def _kind(decl):
    """'pointer' for anything with * or [, otherwise the scalar type's name"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in re.sub(r"\bconst\b", "", decl).split()]
    for k in ("long long", "int", "double", "void"):
        if " ".join(words[:len(k.split())]) == k:
            return k
    raise AssertionError("unreadable declaration: %r" % decl)


def prototypes():
    """dict function name -> (return kind, [parameter kinds]) of every `ret name(params);` outside the typedefs"""
    src = re.sub(r"typedef struct \{[^{}]*\} \w+;", "", _source())
    out = {}
    for ret, name, params in re.findall(r"^((?:const\s+)?[\w ]+?[\s*]+)(landing_\w+)\s*\(([^()]*)\)\s*;", src, flags=re.M):
        params = [p.strip() for p in params.split(",")]
        out[name] = (_kind(ret), [] if params == ["void"] or params == [""] else [_kind(p) for p in params])
    return out
