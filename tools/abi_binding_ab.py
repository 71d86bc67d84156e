#!/usr/bin/env python
"""The ctypes table of two versions of the package's _lib.py against each other, and what building it costs at import.

    python tools/abi_binding_ab.py [REV]        (REV: the git revision whose _lib.py is the base; default HEAD~1)

For a change of the binding: both modules run `declare` on a recording object that has every name of the new EXPORTS, and every
argtypes / restype that differs is printed - a POINTER(X) argument counts as c_void_p (both take an address), a restype nobody set
as c_int (what ctypes assumes).  Then the import cost, on the CPU: exec of each module's bytecode (for a _lib.py that reads
include/wunet_hip.h that is the parse) plus one `declare` on a fresh recording object, the median of 200 repeats.
Exit status 0: the tables agree except for the differences listed in EXPECTED."""
import ctypes
import os
import statistics
import subprocess
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PY = "wave-u-net-for-speech-enhancement_amd/_lib.py"
# char* buf of wunet_profile_collect: c_char_p by hand, c_void_p by the uniform pointer rule (callers pass a create_string_buffer)
EXPECTED = {("wunet_profile_collect", "argtypes[0]")}


class _Fn:
    def __init__(self):
        self.restype, self.argtypes = ctypes.c_int, None


def recorder(names):
    lib = types.SimpleNamespace()
    for name in names:
        setattr(lib, name, _Fn())
    return lib


def module(code, path):
    mod = types.ModuleType("_lib_ab")
    mod.__file__ = path                                       # (_lib.py finds the library and the header beside itself)
    exec(code, mod.__dict__)
    return mod


def norm(t):
    return ctypes.c_void_p if isinstance(t, type) and issubclass(t, ctypes._Pointer) else t


def show(t):
    return getattr(t, "__name__", repr(t))


def cost_us(source, path, names, repeats=200):
    code = compile(source, path, "exec")                      # (an import runs the cached bytecode)
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        module(code, path).declare(recorder(names))
        out.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(out)


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~1"
    path = os.path.join(ROOT, LIB_PY)
    base_src = subprocess.run(["git", "-C", ROOT, "show", f"{rev}:{LIB_PY}"], check=True, capture_output=True, text=True).stdout
    new_src = open(path).read()
    base, new = (module(compile(src, path, "exec"), path) for src in (base_src, new_src))
    names = sorted(new.EXPORTS)
    print(f"base {rev}: {len(base.EXPORTS)} exports, {len(base_src.splitlines())} lines;  new: {len(names)} exports, {len(new_src.splitlines())} lines")
    if sorted(base.EXPORTS) != names:
        print("EXPORTS differ:", sorted(set(base.EXPORTS) ^ set(names)))
    a, b = base.declare(recorder(names)), new.declare(recorder(names))
    found = set()
    for name in names:
        fa, fb = getattr(a, name), getattr(b, name)
        if norm(fa.restype) is not norm(fb.restype):
            found.add((name, "restype"))
            print(f"DIFF  {name} restype: base {show(fa.restype)}  new {show(fb.restype)}")
        if fa.argtypes is None or fb.argtypes is None or len(fa.argtypes) != len(fb.argtypes):
            found.add((name, "argtypes"))
            print(f"DIFF  {name} argtypes: base {fa.argtypes}  new {fb.argtypes}")
            continue
        for i, (ta, tb) in enumerate(zip(fa.argtypes, fb.argtypes)):
            if norm(ta) is not norm(tb):
                found.add((name, f"argtypes[{i}]"))
                print(f"DIFF  {name} argtypes[{i}]: base {show(ta)}  new {show(tb)}")
    print(f"{len(names)} entry points, {sum(len(getattr(b, n).argtypes) for n in names)} arguments: {len(found)} differing, "
          f"{len(found - EXPECTED)} unexpected, {len(EXPECTED - found)} expected and not found")
    print(f"import cost (exec of the module + declare, median of 200): base {cost_us(base_src, path, names):.0f} us, "
          f"new {cost_us(new_src, path, names):.0f} us")
    return 0 if found == EXPECTED else 1


if __name__ == "__main__":
    sys.exit(main())
