"""The mfx_* C ABI as ctypes sees it, read once from include/magent_amd.h.

    prototypes()   {name: (restype, [argtypes])} of every ``ret mfx_name(args);`` the header declares
    struct(name)   the ctypes.Structure of a ``typedef struct mfx_name { ... } mfx_name;``
    bind(dll)      set argtypes / restype on every declared function the library exports
    ptr(t)         the address of a tensor's (or numpy array's) data, None for None
    stream()       torch's current stream as a hipStream_t

The mapping rule: a scalar becomes the ctypes type of the same C type, ``const char *`` becomes c_char_p, and every
other pointer or array parameter -- whatever it points to -- becomes c_void_p, which takes None, an int, a c_void_p,
byref(x), a POINTER instance or a ctypes array.  With argtypes set a bare Python int reaches a pointer, size_t or
int64_t parameter whole (without them ctypes passes it as a C int: the upper half of an address is lost silently),
and a uint32_t parameter wraps modulo 2^32 by itself.  A type outside the tables raises at parse time, naming the
function and the parameter: nothing is guessed.  A new entry point needs only its prototype in the header.
"""
import ctypes
import os
import re

HEADER = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "include",
                                       "magent_amd.h"))

_C = ctypes
_SCALARS = {"int": _C.c_int, "unsigned": _C.c_uint, "bool": _C.c_bool, "float": _C.c_float, "double": _C.c_double,
            "size_t": _C.c_size_t, "long long": _C.c_longlong, "int8_t": _C.c_int8, "uint8_t": _C.c_uint8,
            "int16_t": _C.c_int16, "uint16_t": _C.c_uint16, "int32_t": _C.c_int32, "uint32_t": _C.c_uint32,
            "int64_t": _C.c_int64, "uint64_t": _C.c_uint64}
_DECL = re.compile(r"([\w\s]+?)([\s*]*)\b(\w+)\s*(\[\d*\])?")


class HeaderError(ValueError):
    pass


def _ctype(decl, structs, where, param=True):
    """One declarator ('const float *d_view', 'long long n', 'size_t bytes[5]') -> (name, ctypes type)."""
    m = _DECL.fullmatch(re.sub(r"\bconst\b", " ", decl).strip())
    if m:
        base, stars, array = " ".join(m.group(1).split()), m.group(2).count("*"), bool(m.group(4))
        if not stars and not array:
            if base in _SCALARS:
                return m.group(3), _SCALARS[base]
        elif base == "char" and stars == 1 and not array:
            return m.group(3), _C.c_char_p
        elif (base in _SCALARS or base in structs or base in ("void", "char")) and (param or not array):
            return m.group(3), _C.c_void_p          # (an array is a pointer only as a parameter)
    raise HeaderError("%s: no ctypes mapping for the type of '%s'" % (where, " ".join(decl.split())))


def parse(text):
    """(prototypes, struct bodies) of header text: {name: (restype, [argtypes])}, {name: 'field declarations'}."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    bodies = dict(re.findall(r"typedef\s+struct\s+(mfx_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S))
    text = re.sub(r"typedef\s+struct\s+(mfx_\w+)\s*\{.*?\}\s*\1\s*;", "", text, flags=re.S)
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w ]*?[\s*]+)(mfx_\w+)\s*\(([^()]*)\)\s*;", text):
        _, restype = _ctype(ret + " " + name, bodies, name + ": the return value")
        if restype is _C.c_void_p:
            raise HeaderError("%s: no ctypes mapping for the return type '%s'" % (name, ret.strip()))
        args = [] if args.strip() == "void" else args.split(",")
        protos[name] = (restype, [_ctype(a, bodies, name)[1] for a in args])
    if len(protos) != len(set(re.findall(r"\b(mfx_\w+)\s*\(", text))):
        raise HeaderError("a declaration of %s is not of the form 'ret name(args);'"
                          % sorted(set(re.findall(r"\b(mfx_\w+)\s*\(", text)) - set(protos)))
    return protos, bodies


_PARSED = None
_STRUCTS = {}


def _header():
    global _PARSED
    if _PARSED is None:
        with open(HEADER) as f:
            _PARSED = parse(f.read())
    return _PARSED


def prototypes():
    return _header()[0]


def fields(body, structs, where):
    """The _fields_ list of a struct body: 'const float *view, *feat; int32_t a, b;' is split per declarator."""
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *rest = stmt.split(",")
        out.append(_ctype(first, structs, where, param=False))
        base = _DECL.fullmatch(re.sub(r"\bconst\b", " ", first).strip()).group(1)
        out += [_ctype(base + " " + r, structs, where, param=False) for r in rest]
    return out


def struct(name):
    """The ctypes.Structure class of the header's struct `name` (made on first use: a struct nothing asks for, such
    as mfx_score_record with its inline arrays, is never mapped)."""
    if name not in _STRUCTS:
        bodies = _header()[1]
        _STRUCTS[name] = type(name, (_C.Structure,), {"_fields_": fields(bodies[name], bodies, "struct " + name)})
    return _STRUCTS[name]


def bind(dll):
    """Declare every header function `dll` exports.  One the library lacks (an older build loaded for an A/B run) is
    skipped -- reaching for it raises AttributeError as before -- and so is one whose argtypes are set already
    (magent.gridworld declares two itself).  No errcheck: check() turns a return code into EngineError."""
    for name, (restype, argtypes) in prototypes().items():
        fn = getattr(dll, name, None)
        if fn is not None and fn.argtypes is None:
            fn.argtypes, fn.restype = argtypes, restype
    return dll


def ptr(t):
    """The data address of a torch tensor or a numpy array; None (a null pointer) for None."""
    if t is None:
        return None
    return t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data


_current_stream = None


def stream():
    """torch's current stream as the hipStream_t the entry points take (torch is imported on the first call)."""
    global _current_stream
    if _current_stream is None:
        from torch.cuda import current_stream as _current_stream
    return _current_stream().cuda_stream
