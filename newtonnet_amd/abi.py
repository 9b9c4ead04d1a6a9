"""The C ABI of libnewtonnet_hip.so as ctypes, derived from include/newtonnet_hip.h: the header is its only statement.

The header's vocabulary is small -- integer #defines, anonymous enums, typedef'd structs of fixed-width scalars, pointers, arrays
and earlier structs by value, and prototypes over the same types -- and parse() refuses anything outside it instead of guessing.
Adding an entry point takes a declaration in the header and a definition in csrc/: nothing here, nothing in hip.py."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'include', 'newtonnet_hip.h')


class HipLibraryError(RuntimeError):
    pass


_SCALARS = {'int': C.c_int32, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint8_t': C.c_uint8, 'size_t': C.c_size_t,
            'float': C.c_float, 'double': C.c_double}
_POINTEES = ('void', 'char')   # type names that may only stand behind a pointer
# struct-pointer parameters that stay c_void_p: the table lives in DEVICE memory and callers pass its address (tensor.data_ptr())
DEVICE_TABLE_PARAMS = {('nnhip_wgrad_batch', 0), ('nnhip_colsum_batch', 0)}

_INT = r'\(?\s*(-?(?:0[xX][0-9a-fA-F]+|[1-9]\d*|0))\s*\)?'
_FLOAT = r'-?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?f?'
_DECLARATOR = re.compile(r'((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)')
_STATEMENT = re.compile(r'\s*(?:(extern\s*"C"\s*\{)|(\})|enum\s*\{([^{}]*)\}\s*;|typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;|([^;{}]+);)')
_PROTOTYPE = re.compile(r'(const\s+char\s*\*\s*|\w+\s+)(\w+)\s*\((.*)\)', re.S)


def _refuse(text):
    raise HipLibraryError(f'include/newtonnet_hip.h: no ctypes binding can be derived for `{" ".join(text.split())}`')


def parse(text):
    """(constants, structs, functions) of a header text: {name: int}, {name: ctypes.Structure subclass} in header order, and
    {name: (restype, argtypes)}."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    consts, structs, funcs = {}, {}, {}
    for line in re.findall(r'^[ \t]*#[^\n]*', text, re.M):
        d = re.fullmatch(r'#\s*define\s+(\w+)(?:\s+(\S.*?))?\s*', line.strip())
        if d and d.group(2) is not None and re.fullmatch(_INT, d.group(2)):
            consts[d.group(1)] = int(re.fullmatch(_INT, d.group(2)).group(1), 0)
        elif d and (d.group(2) is None or re.fullmatch(_FLOAT, d.group(2))):
            pass                      # the include guard; a float constant stays a literal on the Python side
        elif not re.match(r'\s*#\s*(ifndef|ifdef|endif|include)\b', line):
            _refuse(line)
    text = re.sub(r'^[ \t]*#[^\n]*', ' ', text, flags=re.M)

    def typed(stmt):                  # "const float* a, *b[N]" -> ('float', '* a, *b[N]'); the type name must be a known one
        m = re.fullmatch(r'(?:const\s+)?(\w+)\b\s*(.*)', stmt.strip(), re.S)
        if not m or not (m.group(1) in _SCALARS or m.group(1) in _POINTEES or m.group(1) in structs):
            _refuse(stmt)
        return m.group(1), m.group(2)

    def declarator(part, stmt):       # "* const name[8][7]" -> (is a pointer, 'name', [8, 7])
        m = _DECLARATOR.fullmatch(part.strip()) or _refuse(stmt)
        extents = []
        for e in re.findall(r'\w+', m.group(3)):
            extents.append(int(e) if e.isdigit() else consts[e] if e in consts else _refuse(stmt))
        return m.group(1).count('*'), m.group(2), extents

    def struct(body, name):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(';'))):
            base, rest = typed(stmt)
            for part in rest.split(','):
                stars, member, extents = declarator(part, stmt)
                t = C.c_void_p if stars else _SCALARS.get(base) or structs.get(base) or _refuse(stmt)
                for n in reversed(extents):       # C order: T f[8][7] is (T * 7) * 8
                    t = t * n
                fields.append((member, t))
        return type(name, (C.Structure,), {'_fields_': fields})

    def prototype(stmt):
        m = _PROTOTYPE.fullmatch(stmt.strip()) or _refuse(stmt)
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        restype = C.c_char_p if ret.endswith('*') else None if ret == 'void' else _SCALARS.get(ret) or _refuse(stmt)
        argtypes = []
        for k, p in enumerate([] if params == 'void' else params.split(',')):
            base, rest = typed(p)
            stars, _, extents = declarator(rest, p)
            if not stars and not extents:
                argtypes.append(_SCALARS.get(base) or _refuse(p))
            elif base in structs and stars == 1 and not extents and (name, k) not in DEVICE_TABLE_PARAMS:
                argtypes.append(C.POINTER(structs[base]))
            else:
                argtypes.append(C.c_void_p)
        return name, (restype, argtypes)

    pos, depth = 0, 0
    while text[pos:].strip():
        m = _STATEMENT.match(text, pos) or _refuse(text[pos:pos + 120])
        pos = m.end()
        if m.group(1) or m.group(2):
            depth += 1 if m.group(1) else -1
            if depth < 0:
                _refuse('}')
        elif m.group(3) is not None:
            value = 0
            for item in filter(None, (s.strip() for s in m.group(3).split(','))):
                e = re.fullmatch(r'(\w+)(?:\s*=\s*' + _INT + ')?', item) or _refuse(item)
                value = int(e.group(2), 0) if e.group(2) else value
                consts[e.group(1)] = value
                value += 1
        elif m.group(4) is not None:
            structs[m.group(5)] = struct(m.group(4), m.group(5))
        else:
            name, sig = prototype(m.group(6))
            funcs[name] = sig
    if depth:
        _refuse('extern "C" { without its }')
    return consts, structs, funcs


def _load():
    try:
        with open(HEADER) as f:
            return parse(f.read())
    except OSError as exc:
        raise HipLibraryError(f'{HEADER} not found: the ctypes binding is derived from it') from exc


CONSTANTS, STRUCTS, FUNCTIONS = _load()


def bind(cdll, names=None):
    """Set restype / argtypes of every declared entry point (or of `names` only) on a loaded library."""
    for name in names or FUNCTIONS:
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = FUNCTIONS[name]
