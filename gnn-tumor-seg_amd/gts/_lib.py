"""ctypes binding of libgts_hip.so (C ABI declared in include/gts_hip.h).

There is NO CPU fallback: if the library is missing or a tensor is not on an AMD GPU the
call raises.  The oracle under /oracle is never reachable from here.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# GTS_LIB_PATH: another build of the same library (A/B runs of two builds in one session, tools/); the default is the in-tree build
LIB_PATH = os.environ.get("GTS_LIB_PATH") or os.path.join(_HERE, "libgts_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "gts_hip.h")
ABI_VERSION = 34

_p = ctypes.c_void_p
_i32 = ctypes.c_int32
_i64 = ctypes.c_int64


class GtsError(RuntimeError):
    pass


# ---------------------------------------------------------------- the header is the ABI
# what an entry point takes by value; everything with a '*' is handed over as an address
_BY_VALUE = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
             "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(GTS_\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", re.M)
_STRUCT = re.compile(r"\btypedef\s+struct\b[^{;]*\{[^{}]*\}\s*\w+\s*;")
_PROTOTYPE = re.compile(r"(?P<ret>[\w\s*]+?)\b(?P<name>\w+)\s*\((?P<args>[^()]*)\)")


def _ctype(decl, statement, returned=False):
    """ctypes type of one parameter (or return) declaration of `statement`; refuses what it does not know."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if returned and words == ["const", "char", "*"] else _p
    words = [w for w in words if w != "const"]
    if returned and words == ["void"]:
        return None
    if not returned and len(words) > 1:
        words = words[:-1]                  # the parameter's name
    if len(words) == 1 and words[0] in _BY_VALUE:
        return _BY_VALUE[words[0]]
    raise GtsError(f"gts_hip.h: cannot bind `{decl.strip()}` of `{statement}`: by value only "
                   f"{', '.join(_BY_VALUE)} are taken (a struct goes by pointer)")


def parse_header(text):
    """(signatures {name: (restype, [argtypes])}, constants {GTS_NAME: int}) of C header text: every prototype
    and every integer #define.  Strict: a declaration it cannot turn into ctypes raises GtsError."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    constants = {name: int(value) for name, value in _DEFINE.findall(text)}
    text = re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)
    text = _STRUCT.sub(" ", text)
    text = re.sub(r'\bextern\s+"C"\s*\{', " ", text)
    *statements, tail = text.split(";")
    if tail.strip() not in ("", "}"):       # the brace that closes extern "C"
        raise GtsError(f"gts_hip.h: cannot parse `{' '.join(tail.split())}`")
    signatures = {}
    for statement in statements:
        statement = " ".join(statement.split())
        m = _PROTOTYPE.fullmatch(statement)
        if m is None:
            raise GtsError(f"gts_hip.h: cannot parse `{statement}`")
        params = [a.strip() for a in m["args"].split(",")]
        if params in ([""], ["void"]):
            params = []
        if "..." in params or "" in params or "[" in m["args"]:
            raise GtsError(f"gts_hip.h: cannot bind `{statement}`: variadic, array or empty parameter")
        signatures[m["name"]] = (_ctype(m["ret"], statement, returned=True), [_ctype(a, statement) for a in params])
    return signatures, constants


_parsed = {}


def _header(path):
    if path not in _parsed:
        with open(path) as f:
            _parsed[path] = parse_header(f.read())
    return _parsed[path]


def signatures(header_path=HEADER_PATH):
    """name -> (restype, argtypes) of every entry point include/gts_hip.h declares: what load() binds."""
    return _header(header_path)[0]


def const(name):
    """Value of an integer `#define GTS_*` of include/gts_hip.h."""
    try:
        return _header(HEADER_PATH)[1][name]
    except KeyError:
        raise GtsError(f"gts_hip.h defines no integer constant {name}") from None


def declared_symbols(header_path=HEADER_PATH):
    """Every function name declared in include/gts_hip.h."""
    return sorted(signatures(header_path))


COLLATE_MAX_SCHEDULES = const("GTS_COLLATE_MAX_SCHEDULES")


class CollateMember(ctypes.Structure):
    """gts_collate_member_t (include/gts_hip.h): one member of a batch, host pointers."""
    _fields_ = [("n_nodes", _i64), ("n_edges", _i64),
                ("indptr", _p), ("indices", _p), ("t_indptr", _p), ("t_indices", _p), ("t_slot", _p), ("t_pos", _p),
                ("features", _p), ("labels", _p), ("feat_bytes", _i32), ("label_bytes", _i32),
                ("sched_rec", _p * COLLATE_MAX_SCHEDULES), ("sched_clusters", _i64 * COLLATE_MAX_SCHEDULES),
                ("sched_loc_words", _i32 * COLLATE_MAX_SCHEDULES)]


class CollateKind(ctypes.Structure):
    """gts_collate_kind_t: the limits one kind of cluster schedule was built with."""
    _fields_ = [("max_rows", _i32), ("max_srcs", _i32), ("tagged", _i32), ("reserved", _i32)]


class CollatePlan(ctypes.Structure):
    """gts_collate_plan_t: sizes and byte offsets of the collated block."""
    _fields_ = [("total_bytes", _i64), ("n_nodes", _i64), ("n_edges", _i64), ("features", _i64), ("labels", _i64),
                ("csr", _i64 * 8), ("sched", _i64 * COLLATE_MAX_SCHEDULES),
                ("sched_clusters", _i64 * COLLATE_MAX_SCHEDULES), ("sched_loc_words", _i32 * COLLATE_MAX_SCHEDULES),
                ("sched_record_words", _i32 * COLLATE_MAX_SCHEDULES)]


_lib = None


def load():
    """Load the HIP library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GtsError(
            f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "The gts operators have no CPU or PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(lib, name)  # AttributeError -> the .so is stale; surface it
        fn.argtypes, fn.restype = argtypes, restype
    if lib.gts_abi_version() != ABI_VERSION:
        raise GtsError(f"libgts_hip.so ABI {lib.gts_abi_version()} != expected {ABI_VERSION}: rebuild")
    # tuning knobs from the environment, e.g. GTS_OPTIONS="1=5,3=1" (option=value pairs, gts_set_option)
    for pair in filter(None, os.environ.get("GTS_OPTIONS", "").split(",")):
        opt, val = pair.split("=")
        if lib.gts_set_option(int(opt), int(val)) != 0:
            raise GtsError(f"GTS_OPTIONS: unknown option {opt}")
    _lib = lib
    return lib


def check(code, what):
    if code != 0:
        msg = load().gts_error_string(code)
        raise GtsError(f"{what} failed with code {code}: {msg.decode() if msg else '?'}")


def require_device(*tensors):
    """All tensors must live on one HIP device and be contiguous."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise GtsError("gts operators run on MI355X only: got a CPU tensor "
                           "(there is no CPU fallback; use the oracle in tests)")
        if not t.is_contiguous():
            raise GtsError("gts operators need contiguous tensors")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise GtsError(f"tensors on different devices: {dev} vs {t.device}")
    return dev


def ptr(t):
    return None if t is None else t.data_ptr()


def current_stream():
    import torch

    return torch.cuda.current_stream().cuda_stream
