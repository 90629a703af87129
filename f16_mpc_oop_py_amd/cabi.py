"""The C-ABI of libf16hip.so as include/f16_hip.h declares it: every signature, struct layout and constant the Python side uses is
read from the header (once, at import) and written down nowhere else.  `declare(handle)` puts the signatures on a ctypes handle.

The type rule, stated once:
  int, long, double, unsigned, uint32_t, uint64_t, int32_t, size_t     their ctypes
  a pointer to a struct the header defines with a body                  POINTER(<the Structure that @structure bound to it>)
  T **                                                                  POINTER(c_void_p)
  every other pointer (to a scalar, void, an opaque handle)             c_void_p
  a `void` parameter list                                               []
  returned: void -> None, const char * -> c_char_p, a scalar as above
Anything else -- a type, or a declaration that does not split into these -- is a ValueError that names the declaration: a wrong
argument list shifts raw device pointers, so nothing here falls back to a default."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "f16_hip.h")
SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "double": ctypes.c_double, "unsigned": ctypes.c_uint, "uint32_t": ctypes.c_uint32,
           "uint64_t": ctypes.c_uint64, "int32_t": ctypes.c_int32, "size_t": ctypes.c_size_t}


def _ctype(text, structs, decl, returned=False):
    """one C type -> its ctypes type by the rule above; a pointer to a struct with a body stays the struct's NAME until functions()"""
    base, stars = " ".join(w for w in text.replace("*", " ").split() if w != "const"), text.count("*")
    if stars == 0 and base in SCALARS:
        return SCALARS[base]
    if returned and (base, stars) in (("void", 0), ("char", 1)):
        return ctypes.c_char_p if stars else None
    if not returned and stars == 1 and structs.get(base):
        return base
    if not returned and stars in (1, 2) and (base in SCALARS or base in structs or base == "void"):
        return ctypes.c_void_p if stars == 1 else ctypes.POINTER(ctypes.c_void_p)
    raise ValueError(f"include/f16_hip.h: the type rule does not cover `{' '.join(text.split())}` in `{decl}`")


def parse(text):
    """the text of a header -> (functions, structs, constants), each a dict in header order"""
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))       # a comment is one space, as the preprocessor has it
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(F16_\w+)[ \t]+(\S[^\n]*?)[ \t]*$", text, flags=re.M):
        plain = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uU]\b", r"\1", value)            # object-like and with a value: not NAME(k), not the include guard
        if not re.fullmatch(r"(0[xX][0-9a-fA-F]+|\d+|<<|[()\s|+-])+", plain):
            raise ValueError(f"include/f16_hip.h: `#define {name} {value}` is not an integer expression")
        constants[name] = int(eval(plain, {"__builtins__": {}}))
    code = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    block = re.search(r'extern\s+"C"\s*\{(.*)\}', code, flags=re.S)
    structs = {}                                                   # name -> _fields_; None for an opaque `typedef struct N N;`

    def typedef(m):
        name, body, fields = m.group(1), m.group(2), []
        for member in filter(None, (" ".join(s.split()) for s in (body or "").split(";"))):
            decl = f"struct {name} {{ {member}; }}"
            t = re.fullmatch(r"(?:const )?(\w+) (.+)", member)
            if not t or t.group(1) not in SCALARS:
                raise ValueError(f"include/f16_hip.h: the type rule does not cover the member `{decl}`")
            for d in t.group(2).split(","):
                f = re.fullmatch(r"\s*(\*)?\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
                if not f or (f.group(1) and f.group(3)):
                    raise ValueError(f"include/f16_hip.h: cannot split the member `{decl}`")
                c = ctypes.c_void_p if f.group(1) else SCALARS[t.group(1)]           # a pointer member is an address
                fields.append((f.group(2), c * int(f.group(3)) if f.group(3) else c))
        structs[name] = None if body is None else fields
        return ""
    code = re.sub(r"\btypedef\s+struct\s+(\w+)\s*(?:\{([^{}]*)\}\s*)?\1\s*;", typedef, block.group(1) if block else code)
    functions = {}
    for decl in filter(None, (" ".join(s.split()) for s in code.split(";"))):
        m = re.fullmatch(r"([^()]*[\s*])(\w+) ?\(([^()]*)\)", decl)
        params = m and [re.fullmatch(r"(.*[\s*])(\w+)", p.strip()) for p in m.group(3).split(",") if m.group(3).strip() != "void"]
        if not m or not all(params):
            raise ValueError(f"include/f16_hip.h: cannot split the declaration `{decl}`")
        functions[m.group(2)] = (_ctype(m.group(1), structs, decl, True), [(_ctype(p.group(1), structs, decl), p.group(2)) for p in params])
    return functions, {k: v for k, v in structs.items() if v is not None}, constants


_FUNCTIONS, _STRUCTS, _CONSTANTS = parse(open(HEADER).read())
_CLASSES = {}


def structs():
    """C struct name -> ctypes _fields_ list, for every `typedef struct N { ... } N;` (the opaque handles have no body)"""
    return _STRUCTS


def constants():
    """name -> int, for every object-like `#define F16_* <integer expression>`"""
    return _CONSTANTS


def structure(cname):
    """Class decorator: the ctypes.Structure below IS the header's struct `cname` -- it gets _fields_ from structs(), and a parameter
    declared as a pointer to `cname` becomes POINTER(that class)."""
    def bind(cls):
        cls._fields_ = _STRUCTS[cname]
        _CLASSES[cname] = cls
        return cls
    return bind


def functions():
    """name -> (restype, [(ctype, parameter name), ...]) for every function the header declares, in header order"""
    resolve = lambda t: ctypes.POINTER(_CLASSES[t]) if isinstance(t, str) else t      # (KeyError: no @structure class for that struct)
    return {name: (res, [(resolve(t), p) for t, p in params]) for name, (res, params) in _FUNCTIONS.items()}


def declare(L):
    """argtypes and restype of every declared function that the ctypes handle `L` exports.  A symbol `L` lacks (the plant-only
    strict build, an older library loaded for an A/B run) is skipped: calling it raises AttributeError, as ctypes has it."""
    for name, (res, params) in functions().items():
        if hasattr(L, name):
            getattr(L, name).restype, getattr(L, name).argtypes = res, [t for t, _ in params]
    return L
