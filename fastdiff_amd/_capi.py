"""ctypes binding of libfastdiff_hip.so (include/fastdiff_hip.h, fastdiff_hip_ext.h, fastdiff_hip_train.h).  No torch types cross this boundary."""
import ctypes as ct
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfastdiff_hip.so")

INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
HEADERS = ("fastdiff_hip.h", "fastdiff_hip_ext.h", "fastdiff_hip_train.h")


class HeaderError(ValueError):
    """A declaration in a public header that read_headers has no rule for."""


_VOIDP, _CHARP = (ct.c_void_p, "<u8"), (ct.c_char_p, "<u8")
_SCALARS = {"char": (ct.c_char, "S1"), "uint8_t": (ct.c_uint8, "u1"), "int16_t": (ct.c_int16, "<i2"), "int": (ct.c_int, "<i4"),
            "int32_t": (ct.c_int32, "<i4"), "unsigned": (ct.c_uint, "<u4"), "int64_t": (ct.c_int64, "<i8"), "uint64_t": (ct.c_uint64, "<u8"),
            "size_t": (ct.c_size_t, "<u8"), "float": (ct.c_float, "<f4"), "double": (ct.c_double, "<f8")}
_COMMENT = re.compile(r"/\*.*?\*/|//[^\n]*", re.S)
_DECL = re.compile(r"""\s*(?:
      \#\s*ifdef\s+__cplusplus\s+(?:extern\s+"C"\s*\{|\})\s*\#\s*endif
    | \#\s*(?:ifndef|ifdef|endif|include)\b[^\n]*
    | \#\s*define\s+(?P<define>\w+)(?P<value>[^\n]*)
    | enum\s*\w*\s*\{(?P<enum>[^{}]*)\}\s*;
    | typedef\s+struct\s+\w+\s*\{(?P<body>[^{}]*)\}\s*(?P<struct>\w+)\s*;
    | typedef\s+struct\s+\w+\s*\*\s*(?P<handle>\w+)\s*;
    | FD_API\s+(?P<sig>[^(){};\#]+)\((?P<params>[^(){};\#]*)\)\s*;
    )""", re.X)
_TYPE = re.compile(r"(const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(\w+)\s*(?:\[\s*(\w+)\s*\])?")
_LITERAL = re.compile(r"(-?)\s*(0[xX][0-9a-fA-F]+|[1-9]\d*|0)[uUlL]*")
_COUNTED = {"FD_API": re.compile(r"\bFD_API\b"), "typedef struct": re.compile(r"\btypedef\s+struct\b")}


def read_headers(sources):
    """[(file name, C text)], read in order -> (constants {name: int}, structs {name: [(field, (ctype, numpy code), array length or None)]},
    prototypes {name: (restype, argtypes)}), each in header order.

    The grammar is the one the public headers keep: `#define NAME number` (decimal or hex, u / l suffixes, `a << b`, an earlier constant;
    a define of anything else is text and is passed over), `enum [tag] { A [= number], ... };`, `typedef struct tag *handle;`,
    `typedef struct tag { type declarator, ...; ... } name;` and `FD_API type name(type declarator, ... | void);`.  A declarator is a name
    with any number of `*` / `*const` in front and, in a struct, one `[bound]` behind.  One rule maps every declaration: a handle and any
    pointer are c_void_p, except `const char *`, which is c_char_p; a scalar maps by its width and kind.  Whatever falls outside raises
    HeaderError with the file, the declaration and the token; nothing is passed over in silence."""
    consts, structs, handles, protos = {}, {}, set(), {}
    for header, raw in sources:
        text = _COMMENT.sub(" ", raw).rstrip()

        def fail(decl, why, token):
            raise HeaderError(f"{header}: {why} {token!r} in `{' '.join(decl.split())}`")

        def number(decl, expr):
            expr = expr.strip()
            terms = [t.strip() for t in (expr[1:-1] if expr.startswith("(") and expr.endswith(")") else expr).split("<<")]
            vals = []
            for term in terms:
                lit = _LITERAL.fullmatch(term)
                if len(terms) > 2 or not lit and term not in consts:
                    fail(decl, "unknown constant", term)
                vals.append(int(lit[1] + lit[2], 0) if lit else consts[term])
            return vals[0] << vals[1] if len(vals) == 2 else vals[0]

        def declare(decl, line, field=False, result=False):
            """`const float *v, *g` -> [("v", (c_void_p, "<u8"), None), ("g", ...)].  field: `[bound]` may follow; result: plain `void` may stand."""
            t = _TYPE.fullmatch(line.strip())
            if not t:
                fail(decl, "unknown declarator", line.strip())
            const, base, rest = t.groups()
            if base not in _SCALARS and base not in structs and base not in handles and base != "void":
                fail(decl, "unknown type", base)
            out = []
            for one in rest.split(","):
                d = _DECLARATOR.fullmatch(one.strip())
                if not d or d[3] is not None and not field:
                    fail(decl, "unknown declarator", one.strip())
                if d[1]:
                    kind = _CHARP if const and base == "char" and d[1].count("*") == 1 else _VOIDP
                elif base in handles:
                    kind = _VOIDP
                elif base in _SCALARS:
                    kind = _SCALARS[base]
                elif base == "void" and result:
                    kind = (None, None)
                else:
                    fail(decl, "type passed by value", base)
                out.append((d[2], kind, None if d[3] is None else number(decl, d[3])))
            return out

        pos, api_defines, before = 0, 0, (len(protos), len(structs) + len(handles))
        while pos < len(text):
            m = _DECL.match(text, pos)
            if not m:
                rest = text[pos:].lstrip()
                fail(rest.split(";")[0][:200], "no rule for the declaration that starts with", rest.split(None, 1)[0])
            pos, decl = m.end(), m[0]
            if m["define"]:
                value = m["value"].strip()
                api_defines += m["define"] == "FD_API"
                if value[:1].isdigit() or value[:1] in ("(", "-"):
                    consts[m["define"]] = number(decl, value)
            elif m["enum"] is not None:
                running = 0
                for item in filter(None, (i.strip() for i in m["enum"].split(","))):
                    name, eq, expr = (p.strip() for p in item.partition("="))
                    if not name.isidentifier():
                        fail(decl, "unknown enumerator", item)
                    consts[name] = number(decl, expr) if eq else running
                    running = consts[name] + 1
            elif m["struct"]:
                structs[m["struct"]] = [f for line in m["body"].split(";") if line.strip() for f in declare(decl, line, field=True)]
            elif m["handle"]:
                handles.add(m["handle"])
            elif m["sig"]:
                (name, (restype, _), _), = declare(decl, m["sig"], result=True)
                if name in protos:
                    fail(decl, "second declaration of", name)
                params = m["params"].strip()
                protos[name] = (restype, [] if params == "void" else [kind[0] for p in params.split(",") for _, kind, _ in declare(decl, p)])
        read = {"FD_API": len(protos) - before[0] + api_defines, "typedef struct": len(structs) + len(handles) - before[1]}
        for token, pattern in _COUNTED.items():
            if read[token] != len(pattern.findall(text)):
                raise HeaderError(f"{header}: {len(pattern.findall(text))} `{token}` tokens, but {read[token]} declarations read")
    return consts, structs, protos


CONSTANTS, _FIELDS, PROTOTYPES = read_headers([(h, open(os.path.join(INCLUDE, h)).read()) for h in HEADERS])
EXPORTS, STRUCTS = list(PROTOTYPES), tuple(_FIELDS)
_STRUCTS, _RECORDS = {}, {}


def struct(name):
    """The ct.Structure class of `typedef struct ... name;`, with the header's field names (one class per struct, made when first asked for)."""
    if name not in _STRUCTS:
        _STRUCTS[name] = type("Fd" + name[3:].title().replace("_", ""), (ct.Structure,),
                              {"_fields_": [(f, kind[0] * n if n else kind[0]) for f, kind, n in _FIELDS[name]]})
    return _STRUCTS[name]


def record(name):
    """The same struct as a numpy dtype with C alignment: device records and host tables are viewed and filled by field name."""
    if name not in _RECORDS:
        fields = [(f, "S%d" % n, ()) if kind[1] == "S1" and n else (f, kind[1], (n,) if n else ()) for f, kind, n in _FIELDS[name]]
        _RECORDS[name] = np.dtype(fields, align=True)
    return _RECORDS[name]


CONSTANTS["FD_BINS_RECORD_BYTES"] = record("fd_bins").itemsize      # the header states it as fd_bins_record_bytes()
globals().update(CONSTANTS)      # FD_OK ... FD_ERR_MISSING, FD_PCM_S16, FD_STOI_SCAN_TILE, ...: every number the headers name
FdConfig, FdStep, FdWeightRef, FdKernelStat, FdEmaItem, FdEmaHyper, FdEmaState, FdSpan, FdSpanWindow, FdRingChunk, FdTrimParams, FdPwgConfig = (
    struct(n) for n in ("fd_config", "fd_step", "fd_weight_ref", "fd_kernel_stat", "fd_ema_item", "fd_ema_hyper", "fd_ema_state", "fd_span",
                        "fd_span_window", "fd_ring_chunk", "fd_trim_params", "fd_pwg_config"))


def step_table(rows):
    """[{t, c_eps, c_div, sigma, c1, c2, c3, add_noise}] (executed first -> last) -> the fd_step array fd_sample takes."""
    steps = (FdStep * len(rows))()
    for k, row in enumerate(rows):
        steps[k] = FdStep(float(row["t"]), float(row["c_eps"]), float(row["c_div"]), float(row["sigma"]),
                          float(row["c1"]), float(row["c2"]), float(row["c3"]), int(row["add_noise"]))
    return steps


_lib = None


class FastDiffHipError(RuntimeError):
    pass


def load():
    """dlopen the HIP library.  Fails loudly: there is no Python/CPU fallback for the compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FastDiffHipError(
            f"{LIB_PATH} is missing: build it with `python -m fastdiff_amd.build` (hipcc, gfx950). "
            "fastdiff_amd has no CPU fallback.")
    lib = ct.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    """Map fd_status to the exception type the reference would raise (SURVEY 8b 'Errors')."""
    if rc >= 0:
        return rc
    msg = lib.fd_last_error(handle)
    msg = msg.decode() if msg else what
    if rc == CONSTANTS["FD_ERR_INVALID"]:
        raise AssertionError(msg)
    if rc == CONSTANTS["FD_ERR_UNSUPPORTED"]:
        raise NotImplementedError(msg)
    if rc == CONSTANTS["FD_ERR_MISSING"]:
        raise KeyError(msg)
    raise FastDiffHipError(f"{what}: {msg} (status {rc})")
