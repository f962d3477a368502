"""Test infrastructure: what the public headers under include/ say, in the terms ``_hip.HEADERS`` is written in.  Plain text processing of the
headers' C (prototypes on any number of lines, ``typedef struct`` bodies, ``#define``s of integers); tests/test_abi.py holds the assertions."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "long long": ctypes.c_longlong, "unsigned int": ctypes.c_uint}
RETURNS = dict(SCALARS, **{"const char*": ctypes.c_char_p, "void": None})
STRUCTS = {"aesr_pack_job": "PackJob", "aesr_prep_job": "PrepJob", "aesr_triplet_desc": "TripletDesc", "aesr_wgrad_reduce_job": "WgradReduceJob"}
_STRUCT_RE = r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;"


def headers():
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def _text(header):
    hdr = open(os.path.join(INCLUDE, header)).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def declared(header):
    """Names of the functions a header declares."""
    return set(re.findall(r"\b(aesr_[a-z0-9_]+)\s*\(", _text(header)))


def _ctype(text):
    """'const float *' -> 'const float*': one space between words, none before a star."""
    return re.sub(r"\s*\*\s*", "*", " ".join(text.split()))


def _fields(body):
    """'const float* w; int a, b;' -> [('const float*', 'w'), ('int', 'a'), ('int', 'b')]"""
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = [d.strip() for d in stmt.split(",")]
        m = re.fullmatch(r"(.*?)(\w+)", first, flags=re.S)
        out += [(_ctype(m.group(1)), n) for n in [m.group(2)] + more]
    return out


def structs(header):
    """struct name -> [(C type, field name), ...] of every ``typedef struct`` of a header."""
    return {name: _fields(body) for body, name in re.findall(_STRUCT_RE, _text(header), flags=re.S)}


def prototypes(header):
    """name -> (return type, [(C type, parameter name), ...]) of every function a header declares."""
    text = re.sub(r"//[^\n]*", "", _text(header))
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)          # preprocessor lines with their continuations
    text = re.sub(_STRUCT_RE, "", text, flags=re.S)
    text = re.sub(r'extern\s+"C"\s*\{', "", text)
    out = {}
    for stmt in text.split(";"):
        m = re.fullmatch(r"[\s}]*(.*?)\b(aesr_[a-z0-9_]+)\s*\((.*)\)\s*", stmt, flags=re.S)
        if m is None:
            assert "aesr_" not in stmt or "(" not in stmt, "%s: not understood: %r" % (header, stmt)
            continue
        params = m.group(3).strip()
        out[m.group(2)] = (_ctype(m.group(1)), [] if params == "void" else _fields(params.replace(",", ";")))
    return out


def defines(header):
    """name -> value of every ``#define`` of a header whose value is an integer or +, -, * of integers and earlier such names."""
    out = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S[^\n]*)$", _text(header), flags=re.M):
        value = re.sub(r"\b[A-Za-z_]\w*\b", lambda m: str(out.get(m.group(0), m.group(0))), value)
        if re.fullmatch(r"[\d\s()*+-]+", value):
            out[name] = int(eval(value))          # digits, brackets and three operators: nothing to run
    return out


def _image(pointee, hip):
    """ctypes type of what a pointer points to, or None where only c_void_p can bind it."""
    if pointee.endswith("*"):
        return ctypes.c_void_p
    return getattr(hip, STRUCTS[pointee]) if pointee in STRUCTS else SCALARS.get(pointee)


def compatible(ctype, bound, hip):
    """Whether ctypes type ``bound`` may stand for a parameter the header declares as ``ctype``.  Scalars map exactly (SCALARS).  A pointer is
    bound as c_void_p, as c_char_p where it points to char or void, or as POINTER(image of the pointee) -- POINTER(c_void_p) for a pointer to
    a pointer, the structure of ``_hip`` for one of the four structs."""
    ctype = _ctype(re.sub(r"\bconst\b", "", ctype))
    if not ctype.endswith("*"):
        return ctype in SCALARS and bound is SCALARS[ctype]
    pointee = ctype[:-1]
    if bound is ctypes.c_void_p:
        return True
    if bound is ctypes.c_char_p:
        return pointee in ("char", "void")
    image = _image(pointee, hip)
    return image is not None and bound is ctypes.POINTER(image)
