"""ctypes binding of csrc/libwunet_hip.so (the C ABI of include/wunet_hip.h).

The header is the one declaration of that ABI: it is read here, once per process, into PROTOTYPES (what `declare` sets on a
library object) and CONSTANTS (the integer #defines the Python side needs).  Nothing is repeated by hand and nothing is generated.

There is deliberately no fallback: if the HIP library or the header is missing or fails to load the import raises, so a GPU box
can never silently run something else.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# (WUNET_LIB_PATH: measurement builds of the same library, e.g. kernel ablations - never set in production)
LIB_PATH = os.environ.get("WUNET_LIB_PATH") or os.path.join(_HERE, "csrc", "libwunet_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "wunet_hip.h")

_SCALARS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "double": ctypes.c_double, "float": ctypes.c_float,
            "long long": ctypes.c_longlong}


def _ctype(c_type, prototype, returned=False):
    """The ctypes type of one C type of the header.  Every pointer is an address (c_void_p: it takes an int, None, byref(...), a
    ctypes array or pointer instance) except a returned `const char*`, which is text.  A type outside the header's few scalars
    raises: ctypes would otherwise pass or return it as int."""
    c_type = " ".join(c_type.split())
    if "*" in c_type:
        return ctypes.c_char_p if returned and c_type.replace(" ", "") == "constchar*" else ctypes.c_void_p
    if returned and c_type == "void":
        return None
    if c_type not in _SCALARS:
        raise TypeError(f"wunet_hip.h: no ctypes mapping for the type {c_type!r} in `{prototype}`")
    return _SCALARS[c_type]


def parse_header(text):
    """(PROTOTYPES, CONSTANTS) of the header's text: name -> (restype, [argtypes]) for every prototype, name -> int for every #define
    of an integer literal (a negative one stands in parentheses; the include guard has no value and is not one).  The header is this
    project's own and regular - /* */ comments, preprocessor lines, `typedef struct` lines, one extern "C" block, named parameters -
    and a statement that is neither a typedef nor such a prototype raises."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {name: int(value.strip("()")) for name, value in
                 re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\d+|\(-\d+\))[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{|\}', "", text)
    prototypes = {}
    for statement in text.split(";"):
        statement = " ".join(statement.split())
        if not statement or statement.startswith("typedef struct "):
            continue
        m = re.fullmatch(r"([\w \*]+?) ?\b(\w+) ?\(([^()]*)\)", statement)
        if m is None:
            raise TypeError(f"wunet_hip.h: not a prototype: `{statement}`")
        restype, name, params = m.groups()
        argtypes = []
        if params.strip() != "void":
            for param in params.split(","):
                p = re.fullmatch(r"(.*?[\* ]) ?\w+", param.strip())           # the type, then the parameter's name
                if p is None:
                    raise TypeError(f"wunet_hip.h: parameter `{param.strip()}` of `{statement}` has no name or no type")
                argtypes.append(_ctype(p.group(1), statement))
        prototypes[name] = (_ctype(restype, statement, returned=True), argtypes)
    return prototypes, constants


def read_header(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} not found: the Python binding takes every signature and constant of the C ABI from it; "
                           "there is no fallback table")
    with open(path) as f:
        return parse_header(f.read())


PROTOTYPES, CONSTANTS = read_header()
EXPORTS = sorted(PROTOTYPES)


def declare(lib):
    """Attach argtypes/restypes to a loaded library object (HIP build or the test emulator build).  An entry point the object does
    not have is skipped: saved libraries of earlier versions (tools/lib_ab.sh, tools/round_vs_round.sh) lack the newer ones."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return lib


_HIP = None


def load_hip():
    """Load libwunet_hip.so or raise.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
    (or `make -C <package>/csrc -j8`)."""
    global _HIP
    if _HIP is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the MI355X HIP library has not been built "
                "(run `make -C wave-u-net-for-speech-enhancement_amd/csrc -j8`); there is no CPU fallback")
        _HIP = declare(ctypes.CDLL(LIB_PATH))
    return _HIP
