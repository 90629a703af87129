"""CPU-side checks of the drop-in boundary: the library loads and exports every symbol include/f16_hip.h declares, and the Python
binding (f16_mpc_oop_py_amd/cabi.py -> lib.py) gives every function, struct and constant what the header says -- the header read
here by the tests' own parser (tests/header_cases.py), which shares nothing with the binding's."""
import ctypes
import os

import pytest

from conftest import REPO
from header_cases import RETURNED, STRUCT, declaration, declared_symbols, defines, kind, struct_fields

# sizeof on the LP64 ABI, from the header by hand: 6 doubles + 5 ints (68 -> 72); an int padded to 8 + 120 doubles; 22 doubles (the
# plant's static_assert); 4 doubles + 2 ints; 5 pointers, an int padded to 8, a uint64, a uint32 padded to 8; 6 pointers + 2 longs
SIZEOF = {"f16_qp_settings": 72, "f16_mpc_weights": 968, "f16_cost_weights": 176, "f16_gain_grid": 40, "f16_wind": 64, "f16_ens": 64}
ERRORS = {"F16_OK": 0, "F16_EINVAL": -1, "F16_EHIP": -2, "F16_ENOGPU": -3}     # the constants lib.py has no name for


def test_library_exports_every_declared_symbol():
    from f16_mpc_oop_py_amd import cabi, lib
    so = lib.build()
    L = ctypes.CDLL(so)
    syms = declared_symbols()
    assert "Nlplant" in syms and "atmos" in syms and "f16_rollout" in syms and len(syms) >= 77
    assert {"f16_debug_elem_sincos", "f16_debug_elem_trig_carry", "f16_debug_elem_atmos", "f16_debug_elem_rcp", "f16_debug_elem_tan",
            "f16_debug_air_triple"} <= set(syms)
    missing = [s for s in syms if not hasattr(L, s)]
    assert not missing, missing
    assert set(cabi.functions()) == set(syms)


def test_every_signature_of_the_binding_is_the_header_s():
    """argtypes, restype and parameter names of ALL declared functions: on the handle lib.load() returns, on a plain CDLL, and on the
    plant-only strict library, where a symbol it lacks is skipped and still raises"""
    from f16_mpc_oop_py_amd import cabi, lib
    lib.build()
    handles = (lib.load(), cabi.declare(ctypes.CDLL(lib.SO_PATH)), cabi.declare(ctypes.CDLL(lib.build_strict())))
    for s in declared_symbols():
        res, params = declaration(s)
        params = [] if params == ["void"] else params
        assert [n for _, n in cabi.functions()[s][1]] == [p.replace("*", " ").split()[-1] for p in params], s
        for L in handles:
            if L is handles[2] and not hasattr(L, s):
                continue
            assert list(getattr(L, s).argtypes) == [kind(p, lib) for p in params], (s, params)
            assert getattr(L, s).restype == RETURNED[res], (s, res)
    assert hasattr(handles[2], "f16_rollout") and not hasattr(handles[2], "f16_mpc_batch")
    with pytest.raises(AttributeError):
        handles[2].f16_mpc_batch(None)


def test_every_struct_of_the_binding_is_the_header_s():
    from f16_mpc_oop_py_amd import cabi, lib
    assert set(cabi.structs()) == set(STRUCT) == set(SIZEOF)
    flat = lambda fields: [(n, getattr(t, "_type_", t), getattr(t, "_length_", None)) for n, t in fields]      # name, type, array length
    for cname, pyname in STRUCT.items():
        cls = getattr(lib, pyname)
        assert flat(cls._fields_) == flat(struct_fields(cname)) == flat(cabi.structs()[cname]), cname
        assert ctypes.sizeof(cls) == SIZEOF[cname] and cname in cls.__doc__, cname


def test_python_constants_equal_the_header():
    """Every object-like #define of include/f16_hip.h -- error codes, status bits, behaviour flags, step rules, the gain-table width
    -- as the Python binding spells it."""
    from f16_mpc_oop_py_amd import cabi, lib
    val = defines()
    assert len(val) >= 22 and cabi.constants() == val and {k: val[k] for k in ERRORS} == ERRORS
    assert set(lib.F16_ST) == {"ALPHA1", "ALPHA2", "BETA", "EL", "ENVELOPE", "NONFINITE", "QP_MAXITER", "QP_INFEASIBLE"}
    for k, v in lib.F16_ST.items():
        assert val["F16_ST_" + k] == v, k
    assert val["F16_ST_LOOP_STALL"] == lib.F16_ST_LOOP_STALL and lib.F16_ST_ENV_STATE(3) == 1 << 11
    names = {"F16_ST_" + k for k in lib.F16_ST} | {k for k in vars(lib) if k in val}
    assert names == set(val) - set(ERRORS)                                        # (a new #define needs a name in lib.py, or a place above)
    for k in names - {"F16_ST_" + k for k in lib.F16_ST}:                         # LOOP_STALL, QP_SOFT_ACTIVE, F16_FLAG_*, F16_INT_*, F16_GS_ENTRIES
        assert val[k] == getattr(lib, k), k
    assert lib.INTEGRATORS == {"euler": val["F16_INT_EULER"], "rk4": val["F16_INT_RK4"]}


@pytest.mark.parametrize("text", ["int f16_new_call(f16_ctx *ctx, float gain, void *stream);", "int f16_new_call(f16_ctx *ctx, double weights[9]);",
                                  "int f16_new_call(f16_ctx *ctx, double);", "long long f16_new_call(void);",
                                  "typedef struct f16_new_call { float gain; } f16_new_call;", "#define F16_NEW_CALL 1.5\n"],
                         ids=["parameter-type", "array-parameter", "unnamed-parameter", "return-type", "member-type", "constant"])
def test_what_the_type_rule_does_not_cover_is_an_error_that_names_the_declaration(text):
    """an unknown parameter type; declarations that do not split into (type, name) pairs; an unknown return type, member type and
    constant: no default stands in for any of them"""
    from f16_mpc_oop_py_amd import cabi
    ok = cabi.parse("typedef struct f16_ctx f16_ctx;\nint f16_new_call(f16_ctx *ctx, double gain, void *stream);\n#define F16_NEW (1u << 4)\n")
    assert [t for t, _ in ok[0]["f16_new_call"][1]] == [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p] and ok[2] == {"F16_NEW": 16}
    with pytest.raises(ValueError, match="(?i)f16_new_call"):
        cabi.parse("typedef struct f16_ctx f16_ctx;\n" + text)


def test_no_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from f16_mpc_oop_py_amd import F16Batch, lib
    with pytest.raises(lib.F16HipError):
        F16Batch([[0.0] * 18])


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(REPO, "f16_mpc_oop_py_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")):
                txt = open(os.path.join(root, f)).read()
                for needle in ("import oracle", "from oracle", "oracle/", "libf16_oracle", "f16o_"):
                    assert needle not in txt, (root, f, needle)
