"""The ctypes binding of libryolo_hip.so, read from include/ryolo_params.h and include/ryolo.h: the headers are the only statement of the
C ABI.  This is a reader of the subset of C those two headers use, not a C parser: whatever it does not recognise raises AbiError.

  typedef struct X { ... } X;    -> STRUCTS["X"], a ctypes.Structure: every pointer field a c_void_p, arrays innermost dimension last
  int ryolo_x(T a, ...);         -> PROTOTYPES["ryolo_x"], the argtypes list (every entry point returns int)

Arguments: a scalar maps by SCALARS; `const Block* p` is POINTER(Block); every other pointer is a raw address, c_void_p, EXCEPT that an
entry point without a ryolo_stream_t argument launches nothing, so its scalar pointers are host out-parameters: POINTER(scalar).  What the
header cannot say (host arrays handed to an entry point that does take a stream, a device table of blocks) is listed in OVERRIDES.
"""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
           "unsigned": C.c_uint, "signed char": C.c_byte, "unsigned char": C.c_ubyte, "unsigned short": C.c_ushort, "uint8_t": C.c_ubyte}
_P3 = C.POINTER(C.c_void_p * 3)
OVERRIDES = {
    ("ryolo_decode", "anchors_host"): C.POINTER(C.c_float),                    # host array of na * 3 floats
    ("ryolo_loss_owner_grids", "owner"): _P3,                                  # host arrays of device pointers, one per scale
    ("ryolo_loss_match_records", "count"): _P3,
    ("ryolo_loss_match_records", "rec"): _P3,
    ("ryolo_loss_grad_scale_multi", "grads"): C.POINTER(C.c_void_p * 8),       # host arrays of count <= 8 pointers / lengths
    ("ryolo_loss_grad_scale_multi", "n"): C.POINTER(C.c_int64 * 8),
    ("ryolo_pack_weights", "table_dev"): C.c_void_p,                           # the PackEntry table lives on the device
}
_DIMS = r"((?:\s*\[\s*\d+\s*\])*)"


class AbiError(ValueError):
    pass


def _clean(text):
    """Comments out, the C++ guard out, `#define NAME integer` substituted; every other preprocessor line must be a known harmless one."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef __cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$", " ", text, flags=re.S | re.M)
    defines, out = {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            out.append(line)
            continue
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+(-?\d+)\s*", line)
        if m:
            defines[m.group(1)] = m.group(2)
        elif not re.fullmatch(r"\s*#\s*(ifndef\s+\w+|define\s+\w+|endif|include\s*[<\"][\w./]+[>\"])\s*", line):
            raise AbiError(f"preprocessor line not understood: {line.strip()!r}")
    text = "\n".join(out)
    for name, value in defines.items():
        text = re.sub(rf"\b{name}\b", value, text)
    return text


def _declarations(text):
    """The top-level declarations, each up to its `;` outside braces."""
    depth, start = 0, 0
    for k, ch in enumerate(text):
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            yield " ".join(text[start:k].split())
            start = k + 1
    if depth or text[start:].strip():
        raise AbiError(f"unterminated declaration: {' '.join(text[start:].split())[:80]!r}")


def _base(spec, scalars, structs, what):
    """`const T **` -> (T, 2); T must be void or a name this reader knows."""
    stars = spec.count("*")
    name = " ".join(w for w in spec.replace("*", " ").split() if w != "const")
    if name != "void" and name not in scalars and name not in structs:
        raise AbiError(f"unknown type {name!r} in {what!r}")
    return name, stars


def _fields(body, scalars, structs, where):
    fields = []
    for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
        first, *more = [d.strip() for d in decl.split(",")]
        m = re.fullmatch(r"(.*[\s*])([A-Za-z_]\w*)" + _DIMS, first)
        if not m:
            raise AbiError(f"field not understood in {where}: {decl!r}")
        name, stars = _base(m.group(1), scalars, structs, decl)
        if (stars and more) or (name == "void" and not stars):
            raise AbiError(f"field not understood in {where}: {decl!r}")
        ctype = C.c_void_p if stars else scalars.get(name) or structs[name]
        for d in [m.group(2) + m.group(3)] + more:
            m = re.fullmatch(r"([A-Za-z_]\w*)" + _DIMS, d)
            if not m:
                raise AbiError(f"field not understood in {where}: {decl!r}")
            t = ctype
            for dim in reversed(re.findall(r"\d+", m.group(2))):
                t = t * int(dim)
            fields.append((m.group(1), t))
    return fields


def _argtypes(func, params, scalars, structs, used):
    has_stream = re.search(r"\bryolo_stream_t\b", params) is not None
    out = []
    for p in [q.strip() for q in params.split(",")]:
        m = re.fullmatch(r"(.*[\s*])([A-Za-z_]\w*)", p)
        if not m:
            raise AbiError(f"argument not understood in {func}: {p!r}")
        name, stars = _base(m.group(1), scalars, structs, f"{func}({p})")
        if (func, m.group(2)) in OVERRIDES:
            used.add((func, m.group(2)))
            out.append(OVERRIDES[func, m.group(2)])
        elif not stars:
            if name not in scalars:
                raise AbiError(f"{func}: {name!r} by value is not supported ({p!r})")
            out.append(scalars[name])
        elif stars == 1 and name in structs:
            out.append(C.POINTER(structs[name]))
        elif stars == 1 and name in scalars and not has_stream:
            out.append(C.POINTER(scalars[name]))
        else:
            out.append(C.c_void_p)
    return out


def parse(text, scalars=None, structs=None, used=None):
    """(structs, prototypes) declared by `text`; `scalars` / `structs` carry the names earlier headers declared and are extended in place
    (`#define` constants are not carried: they hold inside the header that defines them, and a later header that uses one raises);
    `used` collects the OVERRIDES keys that matched an argument."""
    scalars = dict(SCALARS) if scalars is None else scalars
    structs = {} if structs is None else structs
    used = set() if used is None else used
    protos = {}
    for decl in _declarations(_clean(text)):
        m = re.fullmatch(r"typedef struct (\w+) \{(.*)\} (\w+)", decl)
        if m and m.group(1) == m.group(3):
            structs[m.group(1)] = type(m.group(1), (C.Structure,), {"_fields_": _fields(m.group(2), scalars, structs, m.group(1))})
            continue
        m = re.fullmatch(r"typedef ((?:un)?signed \w+|\w+) (\w+)", decl)
        if m and m.group(1) in scalars:
            scalars[m.group(2)] = scalars[m.group(1)]
            continue
        m = re.fullmatch(r"typedef struct \w+ ?\* ?(\w+)", decl)                # an opaque handle (ryolo_stream_t), passed as an address
        if m:
            scalars[m.group(1)] = C.c_void_p
            continue
        m = re.fullmatch(r"int (ryolo_\w+) ?\((.*)\)", decl)
        if not m or m.group(1) in protos:
            raise AbiError(f"declaration not understood: {decl[:120]!r}")
        protos[m.group(1)] = _argtypes(m.group(1), m.group(2), scalars, structs, used)
    return structs, protos


def _load():
    scalars, structs, used = dict(SCALARS), {}, set()
    parse(open(os.path.join(INCLUDE, "ryolo_params.h")).read(), scalars, structs, used)
    structs, protos = parse(open(os.path.join(INCLUDE, "ryolo.h")).read(), scalars, structs, used)
    if set(OVERRIDES) - used:
        raise AbiError(f"OVERRIDES name arguments that include/ryolo.h does not declare: {sorted(set(OVERRIDES) - used)}")
    return structs, protos


STRUCTS, PROTOTYPES = _load()
