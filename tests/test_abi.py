"""-m "not gpu": the C-ABI library builds, loads on a GPU-less box and exports every symbol that
include/wunet_hip.h declares; the product path refuses to run without it and without a GPU."""
import ctypes
import importlib
import os
import re

import pytest
import torch

from conftest import PKG_NAME, ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "wunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(wunet_[a-z0-9_]+)\s*\(", src)))


def _built():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    if not os.path.exists(lib_mod.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return lib_mod


def test_header_symbols_are_exported():
    lib_mod = _built()
    lib = ctypes.CDLL(lib_mod.LIB_PATH)          # HIP runtime initialises lazily: loading needs no GPU
    names = _declared()
    assert len(names) >= 18
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/wunet_hip.h but not exported"
    assert sorted(lib_mod.EXPORTS) == names, "engine binding list and header disagree"


def _defined():
    """The integer #defines of the header by this file's own regexp (like _declared: a second, independent reading)."""
    src = open(os.path.join(ROOT, "include", "wunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {name: int(value) for name, value in re.findall(r"#define\s+(WUNET_\w+)\s+\(?(-?\d+)\)?\s*$", src, flags=re.M)}


def test_derived_signatures_carry_the_headers_types():
    """ctypes passes and returns int where nothing is declared: the 64-bit returns and the float / double / long long parameters
    are where a wrong table would truncate or pass garbage."""
    c = ctypes
    P = importlib.import_module(PKG_NAME + "._lib").PROTOTYPES
    assert len(P) == 86
    sized = [n for n in P if n.endswith("_bytes")]
    tiles = [n for n in P if n.endswith("_tile")]
    assert len(sized) == 20 and len(tiles) == 3
    other = ["wunet_profile_collect", "wunet_last_error", "wunet_destroy", "wunet_comm_destroy", "wunet_debug_set_conv_trace"]
    assert sorted(n for n in P if P[n][0] is not c.c_int) == sorted(sized + tiles + other)          # every other return is an int
    for name in sized:
        assert P[name][0] is c.c_size_t, name
    for name in tiles + ["wunet_profile_collect"]:
        assert P[name][0] is c.c_longlong, name
    for name in ("wunet_destroy", "wunet_comm_destroy", "wunet_debug_set_conv_trace"):
        assert P[name][0] is None, name
    assert P["wunet_last_error"] == (c.c_char_p, [])
    assert P["wunet_loss_scratch_bytes"] == (c.c_size_t, [])
    for name, (restype, argtypes) in P.items():
        assert restype in (c.c_int, c.c_size_t, c.c_longlong, c.c_char_p, None), name
        assert all(t in (c.c_void_p, c.c_int, c.c_size_t, c.c_double, c.c_float, c.c_longlong) for t in argtypes), name
        if restype is c.c_char_p:
            assert name == "wunet_last_error"
    mix = P["wunet_mix_windows"][1]
    assert [i for i, t in enumerate(mix) if t is c.c_float] == [6] and c.c_double not in mix
    assert all(c.c_float not in argtypes for name, (_, argtypes) in P.items() if name != "wunet_mix_windows")
    adam = P["wunet_adam_step_ex"][1]
    assert [i for i, t in enumerate(adam) if t is c.c_double] == [6, 7, 8, 9, 11, 12, 13]
    assert [i for i, t in enumerate(adam) if t is c.c_longlong] == [10]
    assert len(adam) == 19 and adam[0] is c.c_int and all(adam[i] is c.c_void_p for i in (1, 2, 3, 4, 5, 14, 15, 16, 17, 18))
    assert P["wunet_create"] == (c.c_int, [c.c_int] * 4 + [c.c_void_p])
    assert P["wunet_workspace_bytes"] == (c.c_size_t, [c.c_void_p, c.c_int])


def test_parser_refuses_what_it_cannot_map(tmp_path):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    ok, consts = lib_mod.parse_header("#define WUNET_A 3\n#define WUNET_B (-4) /* c */\n#define WUNET_GUARD\ntypedef struct s s;\n"
                                      "long long wunet_x(const float* const* p /* [n] */,\n    size_t n);\nvoid wunet_y(void);")
    assert ok == {"wunet_x": (ctypes.c_longlong, [ctypes.c_void_p, ctypes.c_size_t]), "wunet_y": (None, [])}
    assert consts == {"WUNET_A": 3, "WUNET_B": -4}
    for text in ("short wunet_x(unsigned n);", "int wunet_x(unsigned n);", "short wunet_x(int n);", "int wunet_x(int n, long m);",
                 "void wunet_x(int n, char c);", "int wunet_x(int (*callback)(int));", "int wunet_x(int);", "int wunet_count;"):
        with pytest.raises(TypeError, match="wunet_"):                 # (the message names the prototype)
            lib_mod.parse_header(text)
    with pytest.raises(RuntimeError, match="no fallback"):
        lib_mod.read_header(str(tmp_path / "wunet_hip.h"))


def test_python_constants_are_the_headers_defines():
    mod = lambda name: importlib.import_module(PKG_NAME + "." + name)          # noqa: E731
    D = _defined()
    C = mod("_lib").CONSTANTS
    assert C == D and len(D) == 24
    assert C["WUNET_E_ARG"] == -1 and C["WUNET_E_RUNTIME"] == -2 and C["WUNET_OK"] == 0
    eng = mod("engine")
    assert eng.LOSS_KINDS == {"mse": D["WUNET_LOSS_MSE"], "l1": D["WUNET_LOSS_L1"], "smooth_l1": D["WUNET_LOSS_SMOOTH_L1"]}
    assert eng.ROW_LOSS_KINDS == {"si_sdr": D["WUNET_LOSS_SI_SDR"], "snr": D["WUNET_LOSS_SNR"]}
    assert len(set(eng.LOSS_KINDS.values()) | set(eng.ROW_LOSS_KINDS.values())) == 5
    for m, name, define in [(eng, "LOSS_ROW_COEFS", "WUNET_LOSS_ROW_COEFS"), (eng, "STFT_COEFS", "WUNET_STFT_COEFS"),
                            (eng, "STFT_MAX_RESOLUTIONS", "WUNET_STFT_MAX_RESOLUTIONS"), (eng, "CSPEC_COEFS", "WUNET_CSPEC_COEFS"),
                            (eng, "MEL_COEFS", "WUNET_MEL_COEFS"), (eng, "MEL_MAX_FILTERS", "WUNET_MEL_MAX_FILTERS"),
                            (eng, "ADAM_HYPER_FLOATS", "WUNET_ADAM_HYPER_FLOATS"),
                            (mod("resample"), "MAX_RATIO", "WUNET_RESAMPLE_MAX_RATIO"), (mod("resample"), "MAX_TAPS", "WUNET_RESAMPLE_MAX_TAPS"),
                            (mod("waveform_dataset"), "SOS_MAX_LEAD", "WUNET_SOS_MAX_LEAD"),
                            (mod("waveform_dataset"), "RIR_MAX_TAPS", "WUNET_REVERB_MAX_TAPS"),
                            (mod("filters"), "MAX_SECTIONS", "WUNET_SOS_MAX_SECTIONS"),
                            (mod("parallel"), "COMM_ID_BYTES", "WUNET_COMM_ID_BYTES"), (mod("trainer"), "SDR_MAX_FILTER", "WUNET_BSS_MAX_FILTER")]:
        assert getattr(m, name) == D[define], name
    rs = mod("resample")
    assert rs.MAX_TAPS == len(rs.design(rs.MAX_RATIO, 1))                        # the longest filter resample.design makes fits the cap
    assert D["WUNET_FWD_SAVE"] == 1 and D["WUNET_FWD_PACKS_VALID"] == 2          # bits of one flag word


def test_declare_skips_what_a_library_lacks():
    """Saved libraries of earlier versions lack the newer entry points: declare neither raises nor invents them, and runs twice."""
    lib_mod = importlib.import_module(PKG_NAME + "._lib")

    class Fn:
        restype, argtypes = ctypes.c_int, None

    have = ["wunet_last_error", "wunet_workspace_bytes", "wunet_forward", "wunet_destroy"]
    old = type("OldLibrary", (), {})()
    for name in have:
        setattr(old, name, Fn())
    for _ in range(2):
        assert lib_mod.declare(old) is old
        assert sorted(vars(old)) == sorted(have)
        for name in have:
            assert (getattr(old, name).restype, getattr(old, name).argtypes) == lib_mod.PROTOTYPES[name]
    real = ctypes.CDLL(_built().LIB_PATH)
    assert lib_mod.declare(lib_mod.declare(real)) is real
    for name in lib_mod.EXPORTS:
        fn = getattr(real, name)
        assert (fn.restype, list(fn.argtypes)) == lib_mod.PROTOTYPES[name], name


def test_shape_errors_come_back_as_codes_not_crashes():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    lib = lib_mod.declare(ctypes.CDLL(lib_mod.LIB_PATH))
    h = ctypes.c_void_p()
    assert lib.wunet_create(12, 24, 4, 16000, ctypes.byref(h)) == -1          # not divisible by 2^12 (reference: 16000 fails too, unet_basic.py:86,93)
    assert b"divisible by 2^n_layers" in lib.wunet_last_error()
    assert lib.wunet_create(12, 24, 4, 12288, ctypes.byref(h)) == 0           # 3 * 2^12: rows padded to 16384 inside
    lib.wunet_destroy(h)
    assert lib.wunet_create(12, 24, 4, 2048, ctypes.byref(h)) == -1           # 2048 >> 12 = 0: deeper than log2(T)
    assert lib.wunet_create(0, 24, 4, 16384, ctypes.byref(h)) == -1
    assert lib.wunet_create(12, 24, 4, 16384, ctypes.byref(h)) == 0
    assert lib.wunet_num_conv_layers(h) == 25
    fwd, tot = lib.wunet_workspace_bytes(h, 0), lib.wunet_workspace_bytes(h, 1)
    assert 0 < fwd < tot
    lib.wunet_destroy(h)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback(pkg):
    m = pkg.Model(n_layers=2, channels_interval=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.mse_loss()(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_torch_extension_is_optional_and_exposes_the_three_calls():
    """torch_ext/wunet_torch.cpp (built by __graft_entry__.build()): when it is there it loads without a GPU and exposes the three
    per-step calls; the engine of an injected library (the emulator tests) never uses it."""
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    ext = eng_mod._load_torch_ext()
    path = os.path.join(ROOT, PKG_NAME, "torch_ext", "_wunet_torch.so")
    assert (ext is not None) == (os.path.exists(path) and not os.environ.get("WUNET_LIB_PATH") and not os.environ.get("WUNET_NO_TORCH_EXT"))
    if ext is not None:
        for name in ("forward", "backward_range", "adam_step"):
            assert callable(getattr(ext, name))
        # a CPU tensor is refused by the extension with the product path's message, before anything is enqueued
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ext.adam_step([torch.zeros(3)], [torch.zeros(3)], [torch.zeros(3)], [torch.zeros(3)], 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, None, None)


def test_loader_prefetch_registers_are_untouched_until_their_wait():
    """conv_h3u_kernel's loader waves prefetch from inline asm and order the use of the loaded registers with hand-placed waits (wunet_h3u.h):
    tools/check_h3u_isa.py compiles the kernel to gfx950 ISA (hipcc cross-compiles here) and proves for this build that no instruction
    touches a prefetch destination between its load and the wait that covers it."""
    import subprocess
    import sys
    from conftest import ROOT
    import os
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_h3u_isa.py")], capture_output=True, text=True, timeout=600)
    # conv_h3u_kernel<M_REP, COPY>: three row-block heights (M_REP = 2, 3, 4 m-tiles of 16 rows) x (eval: no operand copy | training: the loaders' stores counted in their waits)
    assert p.returncode == 0 and "6 kernels checked, 0 problems" in p.stdout, p.stdout[-2000:] + p.stderr[-500:]


def test_the_isa_checker_sees_a_touched_prefetch_register():
    """The checker must FAIL on what it guards against: the same ISA with one instruction planted that (a) overwrites a prefetch load's destination
    right behind the load, (b) reads it just before the stage barrier that does not cover it yet - the compiler-inserted copy / temporary re-use
    that tools/check_h3u_isa.py exists to catch."""
    import importlib.util
    import os
    import re
    from conftest import ROOT
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    spec = importlib.util.spec_from_file_location("check_h3u_isa", os.path.join(ROOT, "tools", "check_h3u_isa.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    name, lines = next(iter(chk.kernels(chk.compile_isa())))          # (one instantiation is enough)
    assert chk.check(name, lines) == []
    barriers = [i for i, ln in enumerate(lines) if re.search(r"s_waitcnt vmcnt\(10\) lgkmcnt\(0\)", ln)]
    # a prefetch load of the steady loop: an asm global_load_dwordx4 behind the first stage barrier
    load = next(i for i in range(barriers[0], len(lines)) if re.match(r"\s*global_load_dwordx4 v\[(\d+):\d+\], v\d+, s\[", lines[i]))
    reg = int(re.match(r"\s*global_load_dwordx4 v\[(\d+):", lines[load]).group(1))
    overwritten = lines[:load + 1] + [f"\tv_mov_b32_e32 v{reg}, 0"] + lines[load + 1:]
    errs = chk.check(name, overwritten)
    assert errs and f"v_mov_b32_e32 v{reg}, 0" in errs[0], errs[:2]
    nxt = next(b for b in barriers if b > load)                        # the barrier that ends the load's own stage: the data need not be there yet
    read_early = lines[:nxt] + [f"\tv_add_f32_e32 v{reg + 1}, v{reg + 1}, v{reg + 1}"] + lines[nxt:]
    errs = chk.check(name, read_early)
    assert errs and "v_add_f32_e32" in errs[0], errs[:2]
