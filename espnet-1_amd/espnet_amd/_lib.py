"""ctypes binding of libespnet_amd.so (the C ABI in include/espnet_amd.h).

The argument types, the structures and the enumerators are all parsed from the header, so
the Python side and the C ABI cannot drift.  Loading fails loudly when the library is missing: there is no CPU
or PyTorch fallback for any op on the hot path.
"""
from __future__ import annotations

import ctypes
import os
import re

# torch must be loaded BEFORE libespnet_amd.so: the PyTorch-ROCm wheel bundles its own
# libamdhip64.so (soname libamdhip64.so.7).  Loading torch first makes our library's
# libamdhip64.so.7 dependency resolve to that already-loaded runtime, so torch's streams
# and allocations and our kernel launches share ONE HIP runtime in the process.
import torch  # noqa: F401,E402

_PKG = os.path.dirname(os.path.abspath(__file__))
# EA_LIB_NAME selects another in-tree build of the same library (A/B measurements)
LIB_PATH = os.path.join(_PKG, "lib", os.environ.get("EA_LIB_NAME", "libespnet_amd.so"))
HEADER = os.path.join(os.path.dirname(os.path.dirname(_PKG)), "include", "espnet_amd.h")

GEMM_PIPE = int(os.environ.get("EA_GEMM_PIPE", "1"))

_CTYPES = {
    "int": ctypes.c_int,
    "long": ctypes.c_long,
    "long long": ctypes.c_longlong,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "unsigned long long": ctypes.c_ulonglong,
    "unsigned int": ctypes.c_uint,
}


def _source(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _scalar_ctype(base: str, decl: str):
    if base not in _CTYPES:
        raise TypeError(f"unsupported C type in header: {decl!r}")
    return _CTYPES[base]


def _member_fields(decl: str):
    """One struct member declaration -> [(name, ctype)]: a scalar, a comma list
    (`int B, T2;`), fixed arrays (`int nI[2], nJ[2];`) or one pointer (-> c_void_p)."""
    text = re.sub(r"\bconst\b", "", decl).strip()
    m = re.fullmatch(r"[\w\s]+\*\s*(\w+)", text)
    if m:
        return [(m.group(1), ctypes.c_void_p)]
    first, *rest = (d.strip() for d in text.split(","))
    base, _, first = first.rpartition(" ")
    ctype = _scalar_ctype(" ".join(base.split()), decl)
    fields = []
    for d in [first] + rest:
        m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", d)
        if not m:
            raise TypeError(f"unsupported struct member in header: {decl!r}")
        fields.append((m.group(1), ctype * int(m.group(2)) if m.group(2) else ctype))
    return fields


def parse_abi(path: str = HEADER):
    """-> ({struct name: ctypes.Structure class}, {enumerator: value}) for every
    `typedef struct ea_* { ... } ea_*;` and `enum { EA_* = n, ... };` of the header."""
    src = _source(path)
    structs, enums = {}, {}
    for m in re.finditer(r"\btypedef\s+struct\s+(ea_\w+)\s*\{([^}]*)\}\s*\1\s*;", src):
        fields = [f for d in m.group(2).split(";") if d.strip() for f in _member_fields(d)]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
    for m in re.finditer(r"\benum\s*\{([^}]*)\}\s*;", src):
        for item in filter(None, (x.strip() for x in m.group(1).split(","))):
            e = re.fullmatch(r"(EA_\w+)\s*=\s*(-?\d+)", item)
            if not e:
                raise TypeError(f"unsupported enumerator in header: {item!r}")
            enums[e.group(1)] = int(e.group(2))
    return structs, enums


STRUCTS, ENUMS = parse_abi()
Epilogue, GroupGemm, ColsumProb, ReduceProb, ConvGeo, LrSchedule, _OptState = (
    STRUCTS["ea_" + n] for n in ("epilogue", "group_gemm", "colsum_prob", "reduce_prob", "conv_geo",
                                 "lr_schedule", "opt_state"))
# every enumerator under its name without the EA_ prefix: F32, BF16, ERR_BAD_ARG, ACT_*, EPI_*,
# CONV_*, SCHED_*
globals().update({k[3:]: v for k, v in ENUMS.items()})
OPT_STATE_BYTES = ctypes.sizeof(_OptState)  # ea_opt_state lives in device memory
OPT_STATE_NEXT_LR = _OptState.next_lr.offset // 4  # float index of next_lr


def _arg_ctype(decl: str):
    decl = decl.strip()
    if "ea_epilogue" in decl and "*" in decl:
        return ctypes.POINTER(Epilogue)
    if "*" in decl:
        return ctypes.c_void_p
    base = re.sub(r"\bconst\b", "", decl).strip()
    return _scalar_ctype(" ".join(base.split()[:-1]), decl)  # without the parameter name


def parse_header(path: str = HEADER):
    """-> {name: [ctypes arg types]} for every `int ea_*(...)` prototype."""
    src = _source(path)
    protos = {}
    for m in re.finditer(r"\bint\s+(ea_\w+)\s*\(([^)]*)\)\s*;", src):
        name, args = m.group(1), m.group(2)
        args = [a for a in (x.strip() for x in args.split(",")) if a and a != "void"]
        protos[name] = [_arg_ctype(a) for a in args]
    return protos


class HipError(RuntimeError):
    pass


_DT = {torch.float32: F32, torch.bfloat16: BF16}  # noqa: F821  (bound from ENUMS above)


def dt(t: torch.Tensor) -> int:
    """The EA_F32 / EA_BF16 code of a tensor's element type."""
    try:
        return _DT[t.dtype]
    except KeyError:
        raise HipError(f"unsupported dtype {t.dtype}") from None


class _Lib:
    def __init__(self):
        self._dll = None
        self.protos = parse_header()

    def load(self):
        if self._dll is None:
            if not os.path.exists(LIB_PATH):
                raise HipError(
                    f"{LIB_PATH} not found: build the HIP library first "
                    "(python espnet-1_amd/build.py). There is no CPU fallback.")
            dll = ctypes.CDLL(LIB_PATH)
            for name, argtypes in self.protos.items():
                fn = getattr(dll, name)
                fn.argtypes = argtypes
                fn.restype = ctypes.c_int
            # 256x256 GEMM tiles on the ping-pong kernel (gemm_pipe); EA_GEMM_PIPE=0 for A/B
            dll.ea_gemm_set_pipe(GEMM_PIPE)
            self._dll = dll
        return self._dll

    def __getattr__(self, name):
        if not name.startswith("ea_"):
            raise AttributeError(name)
        fn = getattr(self.load(), name)

        def call(*args):
            rc = fn(*args)
            if rc != 0:
                what = "bad argument/shape/alignment" if rc == ERR_BAD_ARG else f"hipError {rc}"
                raise HipError(f"{name} failed: {what}")
            return rc

        call.__name__ = name
        setattr(self, name, call)
        return call


lib = _Lib()
