"""ctypes binding of ``libretr_hip.so`` (the gfx950 kernels; C-ABI in ``include/retr_hip.h``).

The header is the only place where a signature, a struct layout or a tuning-knob number is
written: this module parses it at import and derives every ``argtypes`` / ``restype``, the
``ctypes.Structure`` classes and the ``TUNE`` name table from it.

The product path has no fallback: if the library is missing or a CUDA/HIP device is absent,
every op raises.  Build the library with ``make`` (or ``__graft_entry__.build()``).
"""
import contextlib
import ctypes
import os
import re
import warnings

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "retr_hip.h")
LIB_PATH = os.path.join(_HERE, "libretr_hip.so")
# A/B measurements only (tools/*_micro.py, tools/ab_step.py): time a baseline build of the same
# C-ABI.  Never silent: a stray setting would swap every kernel of the process.
if os.environ.get("RETR_AB_LIB"):
    LIB_PATH = os.environ["RETR_AB_LIB"]
    import sys as _sys
    print(f"retr_amd: RETR_AB_LIB is set -- loading kernels from {LIB_PATH} instead of the "
          f"in-tree libretr_hip.so (A/B tooling only)", file=_sys.stderr)

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong,
            "unsigned long long": ctypes.c_ulonglong, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "unsigned char"}      # behind a plain void*
_DECLARATOR = re.compile(r"(.+?)([\s*]+)(\w+)\s*(?:\[\s*(\d+)\s*\])?")
_PROTOTYPE = re.compile(r"([\w\s*]+?)\b(\w+)\s*\(([^()]*)\)")


def _ctype(spelling, structs, where, returned=False):
    """The ctypes type of a C type as the header spells it ('const float*', 'long', ...)."""
    base = " ".join(w for w in spelling.replace("*", " ").split() if w != "const")
    stars = spelling.count("*")
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if stars == 0 and base == "void" and returned:
        return None
    if stars == 1 and base == "char" and returned:
        return ctypes.c_char_p
    if stars == 1 and base in structs and not returned:
        return ctypes.POINTER(structs[base])
    if stars >= 1 and base in _POINTEES and not returned:
        return ctypes.c_void_p
    raise RuntimeError(f"retr_hip.h: unknown C type {spelling.strip()!r} in `{where}`")


def _declarations(decl, structs, where):
    """[(name, ctypes type)] of one declaration: 'int M, N', 'const float *w, *bn_w',
    'float f[3]' or a single function parameter."""
    out, base = [], ""
    for piece in decl.split(","):             # later declarators share the first one's base type
        m = _DECLARATOR.fullmatch(f"{base} {piece.strip()}".strip())
        if m is None:
            raise RuntimeError(f"retr_hip.h: cannot parse `{where}`")
        base = m.group(1)
        t = _ctype(base + m.group(2), structs, where)
        out.append((m.group(3), t * int(m.group(4)) if m.group(4) else t))
    return out


def parse_header(src):
    """(functions, structs, constants) of a C header in the style of include/retr_hip.h.

    functions: name -> (restype, [(parameter name, ctypes type)]) in declaration order;
    structs: typedef name -> ctypes.Structure subclass; constants: enum members and integer
    #defines.  Text that is none of these is an error, as is a type outside the table above:
    nothing is skipped and nothing defaults to int."""
    src = re.sub(r"/\*.*?\*/|//[^\n]*", " ", src, flags=re.S)
    constants = {m.group(1): int(m.group(2), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|\d+))[ \t]*$", src, re.M)}
    src = re.sub(r"^[ \t]*#.*$", " ", src, flags=re.M)
    src = re.sub(r'extern\s+"C"\s*\{', " ", src)
    functions, structs = {}, {}

    def enum(m):
        value = -1
        for item in filter(str.strip, m.group(1).split(",")):
            name, _, given = item.partition("=")
            value = int(given, 0) if given.strip() else value + 1
            constants[name.strip()] = value
        return " "

    def struct(m):
        name, fields = m.group(2), []
        for decl in filter(str.strip, m.group(1).split(";")):
            fields += _declarations(decl, structs, f"{name}: {' '.join(decl.split())}")
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
        return " "

    src = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, src)
    src = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, src)
    *prototypes, tail = src.split(";")            # what is left: `ret name(params);` ...
    if tail.strip() not in ("", "}"):             # ... and the closing brace of extern "C"
        prototypes.append(tail)
    for text in prototypes:
        where = " ".join(text.split())
        m = _PROTOTYPE.fullmatch(where)
        if m is None:
            raise RuntimeError(f"retr_hip.h: cannot parse the declaration `{where[:200]}`")
        args = []
        if m.group(3).strip() != "void":
            for p in m.group(3).split(","):
                args += _declarations(p, structs, where)
        functions[m.group(2)] = (_ctype(m.group(1), structs, where, returned=True), args)
    return functions, structs, constants


def _read_header():
    try:
        with open(HEADER_PATH, encoding="utf-8") as f:
            return parse_header(f.read())
    except OSError as e:
        raise RuntimeError(f"retr_amd: the C-ABI header {HEADER_PATH} cannot be read ({e}); the "
                           "binding is derived from it") from e


FUNCTIONS, STRUCTS, CONSTANTS = _read_header()

F32, BF16 = CONSTANTS["RETR_DTYPE_F32"], CONSTANTS["RETR_DTYPE_BF16"]
TUNE_COUNT = CONSTANTS["RETR_TUNE_COUNT"]
# tuning knobs by name: TUNE["ATTN_MODE"] == 5
TUNE = {k[len("RETR_TUNE_"):]: v for k, v in CONSTANTS.items()
        if k.startswith("RETR_TUNE_") and k != "RETR_TUNE_COUNT"}

LinearFwdDesc = STRUCTS["retr_linear_fwd_desc"]
LinearDgradDesc = STRUCTS["retr_linear_dgrad_desc"]
LinearWgradDesc = STRUCTS["retr_linear_wgrad_desc"]
ConvWgradDesc = STRUCTS["retr_conv_wgrad_desc"]
ConvUnpackDesc = STRUCTS["retr_conv_unpack_desc"]
PosItem = STRUCTS["retr_pos_item"]
LnOut = STRUCTS["retr_ln_out"]
ConvPackDesc = STRUCTS["retr_conv_pack_desc"]
CatRowsDesc = STRUCTS["retr_cat_rows_desc"]
SlabSumDesc = STRUCTS["retr_slab_sum_desc"]
PipeItem = STRUCTS["retr_pipe_item"]

_lib = None


def load():
    """Load the kernel library (raises if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"retr_amd: native library {LIB_PATH} is missing; build it with `make` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, params) in FUNCTIONS.items():
            fn = getattr(lib, name)
            fn.argtypes = [t for _, t in params]
            fn.restype = restype
        # RETR_TUNE_<knob>=<value> in the environment presets a tuning knob (A/B runs)
        # (a malformed value or an unknown knob number is reported and skipped: it must not
        # break every import of the package)
        for k, v in os.environ.items():
            if k.startswith("RETR_TUNE_") and k[10:].isdigit():
                try:
                    val = int(v)
                except ValueError:
                    warnings.warn(f"retr_amd: ignoring {k}={v!r} (not an integer)")
                    continue
                if not 0 <= int(k[10:]) < TUNE_COUNT:
                    warnings.warn(f"retr_amd: ignoring {k}={v!r} (no tuning knob {k[10:]})")
                    continue
                lib.retr_tune(int(k[10:]), val)     # (returns the knob's previous value)
        _lib = lib
    return _lib


def exported_symbols():
    return list(FUNCTIONS)


def tune(name, value):
    """Set the tuning knob RETR_TUNE_<name>; returns its previous value."""
    if name not in TUNE:
        raise KeyError(f"no tuning knob {name!r}; the knobs are {', '.join(TUNE)}")
    return load().retr_tune(TUNE[name], value)


@contextlib.contextmanager
def tuned(**knobs):
    """``with tuned(ATTN_MODE=2, ATTN_SPLIT=1):`` sets the knobs for the block and puts back
    the values they had before, in reverse order, however the block ends."""
    previous = []
    try:
        for name, value in knobs.items():
            previous.append((name, tune(name, value)))
        yield
    finally:
        for name, value in reversed(previous):
            tune(name, value)


_probe = None


def set_probe(p):
    """Install (or remove with None) a retr_amd.probe.Probe that times selected calls."""
    global _probe
    _probe = p


def _raw_call(name, args):
    rc = getattr(load(), name)(*args)
    if rc is not None and rc != 0:   # void functions return None
        msg = load().retr_last_error()
        raise RuntimeError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")


def call(name, *args):
    if _probe is not None and name in _probe.names:
        return _probe.wrap(name, args, lambda: _raw_call(name, args))
    _raw_call(name, args)


def ptr(t):
    """Device pointer of a tensor (or None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


def require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("retr_amd ops run on the MI355X (HIP) device only; got a "
                               f"{t.device} tensor (no CPU fallback)")
