"""The tests' own reading of include/f16_hip.h: the one header parser of the suite.  It shares no code with the binding's
(f16_mpc_oop_py_amd/cabi.py) on purpose -- the tests compare what the two make of the same text."""
import ctypes
import os
import re

from conftest import REPO

SCALAR = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
          "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}
RETURNED = {"void": None, "const char *": ctypes.c_char_p, **SCALAR}
STRUCT = {"f16_qp_settings": "QPSettings", "f16_mpc_weights": "MPCWeights", "f16_cost_weights": "CostWeights", "f16_gain_grid": "GainGrid",
          "f16_wind": "Wind", "f16_ens": "Ens"}                                  # the C struct -> its class in f16_mpc_oop_py_amd.lib


def header(comments=False):
    """the text of include/f16_hip.h, by default without its /* */ comments"""
    src = open(os.path.join(REPO, "include", "f16_hip.h")).read()
    return src if comments else re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared_symbols():
    src = "\n".join(l for l in header().splitlines() if not l.lstrip().startswith("#"))
    return sorted(set(re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{]*\)\s*;", src)) - {"defined"})


def declaration(name):
    """(return type, parameter list) of `name` as include/f16_hip.h declares it"""
    m = re.search(r"^[ \t]*([\w \t\*]+?)\s*\b%s\s*\(([^;{]*)\)\s*;" % name, header(), flags=re.M)
    assert m, f"{name} is not declared in include/f16_hip.h"
    return " ".join(m.group(1).split()), [" ".join(p.split()) for p in m.group(2).split(",")]


def header_parameters(name):
    """the parameter list of `name` as include/f16_hip.h declares it"""
    return declaration(name)[1]


def names(symbol):
    """the parameter names of `symbol` in the order of include/f16_hip.h"""
    return [p.replace("*", " ").split()[-1] for p in header_parameters(symbol)]


def kind(param, lib):
    """the ctypes type the binding has to give the parameter `param` (`const double *x`, `int hold`, `const f16_ens *h_ens`)"""
    words = [w for w in param.replace("*", " * ").split() if w != "const"][:-1]
    if "*" not in words:
        return SCALAR[words[0]]
    if words.count("*") == 2:
        return ctypes.POINTER(ctypes.c_void_p)
    return ctypes.POINTER(getattr(lib, STRUCT[words[0]])) if words[0] in STRUCT else ctypes.c_void_p


def struct_fields(name):
    """the members of `typedef struct name { ... } name;` -> [(member, ctypes type)]: a pointer member is an address"""
    body, out = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (name, name), header()).group(1), []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        base, rest = line.replace("const ", "").split(None, 1)
        for d in rest.split(","):
            member, n = re.fullmatch(r"\s*\*?\s*(\w+)\s*(?:\[(\d+)\])?\s*", d).groups()
            out.append((member, ctypes.c_void_p if "*" in d else SCALAR[base] * int(n) if n else SCALAR[base]))
    return out


def defines():
    """name -> value of every object-like `#define F16_* <value>` (not the include guard, not F16_ST_ENV_STATE(k))"""
    found = re.findall(r"^#define[ \t]+(F16_\w+)[ \t]+(\(?[0-9a-fx<>() u\-]+\)?)[ \t]*$", header(), flags=re.M)
    return {name: eval(value.replace("u", "")) for name, value in found}
