#!/usr/bin/env python
"""Two builds of the emulator library (tests/emu/libwunet_emu.so) against each other, bit for bit, in one process.

    python tools/emu_lib_ab.py BASE.so [NEW.so]        (NEW defaults to tests/emu/libwunet_emu.so, built if missing)

For a refactor of the host path: both libraries run the case table below through Engine(lib=..., host_memory=True) and every
result is compared with np.array_equal - output, loss, every parameter gradient, the input gradient, the running statistics and
num_batches_tracked - and so is the text of wunet_profile_collect with the profiler on (kernel names and launch counts; the
emulator build reports no flops / bytes).  Planner switches are read when a context is planned: every run gets its own engine.
(A base library from before PlanSwitches reads WUNET_WGRAD_XCD and WUNET_A_CAP once per process: set those outside, one run each.
One from before WUNET_NO_ENC_GZ and WUNET_PA_SWAP joined them reads those two at its first backward and keeps them: its runs of their
cases have them unset - the results are to be the same bits either way.)
The auxiliary entry points (aux_cases: the losses forward and backward, the loader ops, the chunk ops, resampling, on the tests' case
tables) are compared the same way, array by array plus the profiler's text, and their refusals (refusals: one bad argument per call)
by return value and wunet_last_error().  The 12 hex digits printed per auxiliary case are a hash of the new library's arrays: two
checkouts of the Python side can be held against each other by the tool's output.  EMU_LIB_AB_AUX_ONLY=1 skips the network cases.
The fused Adam step runs through both of its C entry points on the cases and refusals of tools/adam_lib_ab.py (compare_adam).
Exit status 0: nothing differs."""
import ctypes
import hashlib
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
PKG = "wave-u-net-for-speech-enhancement_amd"
from oracle import plan                                   # noqa: E402

eng_mod = importlib.import_module(PKG + ".engine")
lib_mod = importlib.import_module(PKG + "._lib")
model_mod = importlib.import_module(PKG + ".model")
loss_mod = importlib.import_module(PKG + ".loss")

SWITCHES = ("WUNET_NO_EVOP", "WUNET_NO_SKIP_FUSE", "WUNET_H3U", "WUNET_H3_NOSPLIT", "WUNET_H3_GRID", "WUNET_H3_KTAIL", "WUNET_UPT", "WUNET_NO_E0",
            "WUNET_H3_ORDER", "WUNET_H3D_ORDER", "WUNET_H3W_ORDER", "WUNET_H3_SPS", "WUNET_H3_OLDSPLIT", "WUNET_NO_ENC_GZ", "WUNET_PA_SWAP")


def masks(n):
    """The frozen masks of tests/test_frozen_bn_emu.py's kinds: the first layer, a decoder layer's producers (the middle layer feeds
    decoder 0's upsampled half, encoder n - 1 its skip half), every layer."""
    nl = 2 * n + 1
    return {"first": [i == 0 for i in range(nl)], "producer": [i in (n - 1, n) for i in range(nl)], "all": [True] * nl}


def cases():
    """(shape, h3, mode, frozen mask name, switches).  Modes: train (saving forward + backward + input gradient), train_nosave
    (training forward, save_for_backward 0), eval, eval_cached (a second eval forward with WUNET_FWD_PACKS_VALID)."""
    out = []
    # fp32 kernels and the split kernels on the small nets; (2, 24, 1, 1024): conv_first_kernel, every level on the split path
    for shape in [(2, 4, 2, 32), (3, 8, 3, 64), (2, 24, 1, 1024)]:
        for h3 in (0, 2):
            for mode in ("train", "train_nosave", "eval", "eval_cached"):
                out.append((shape, h3, mode, None, {}))
    # levels of 1 and 2 samples: the scalar kernels (middle level of 2 samples: (3, 8, 2, 16); of 1: (4, 4, 2, 16))
    for shape in [(3, 8, 2, 16), (4, 4, 2, 16)]:
        for mode in ("train", "eval"):
            out.append((shape, 0, mode, None, {}))
    # EVOP, the skip hand-off and conv_h3u_kernel, each with its switch
    for shape, grid in [((3, 24, 3, 2048), ""), ((4, 16, 3, 4096), "8")]:
        base = {"WUNET_H3_NOSPLIT": "1"}
        if grid:
            base["WUNET_H3_GRID"] = grid
        for sw in [{}, {"WUNET_NO_EVOP": "1"}, {"WUNET_NO_SKIP_FUSE": "1"}, {"WUNET_H3U": "0"}, {"WUNET_H3U": "256,256"}]:
            for mode in ("eval", "train"):
                out.append((shape, 2, mode, None, dict(base, **sw)))
        out.append((shape, 2, "eval_cached", None, base))
        # the other planner switches (the two split-K ones without WUNET_H3_NOSPLIT, which would come first)
        grid_only = {k: v for k, v in base.items() if k != "WUNET_H3_NOSPLIT"}
        for sw in [{"WUNET_H3_KTAIL": "0"}, {"WUNET_UPT": "0"}, {"WUNET_NO_E0": "1"}, {"WUNET_H3_ORDER": "432"}, {"WUNET_H3D_ORDER": "432"},
                   {"WUNET_H3W_ORDER": "432"}]:
            for mode in ("eval", "train"):
                out.append((shape, 2, mode, None, dict(base, **sw)))
        for sw in [{"WUNET_H3_SPS": "1"}, {"WUNET_H3_OLDSPLIT": "1"}]:
            for mode in ("eval", "train"):
                out.append((shape, 2, mode, None, dict(grid_only, **sw)))
        out.append((shape, 2, "train_nosave", None, dict(base, WUNET_H3U="256,256")))
        # the backward's two elementwise switches, un-split (GZ_ENC recompute, or g stored and read back) and with split-K data gradients
        # (pass A adds the partials itself; (4, 16, 3, 4096): pieces > 1, the swapped grid)
        for sw in [{"WUNET_NO_ENC_GZ": "1"}, {"WUNET_PA_SWAP": "0"}, {"WUNET_NO_ENC_GZ": "1", "WUNET_PA_SWAP": "0"}]:
            out.append((shape, 2, "train", None, dict(base, **sw)))
            out.append((shape, 2, "train", None, dict(grid_only, **sw)))
        out.append((shape, 2, "train", None, grid_only))
    # padded lengths: every conv through conv_reduce_bn_kernel, no EVOP, no conv_h3u_kernel
    for shape, h3 in [((3, 8, 2, 96), 0), ((3, 8, 2, 96), 2), ((3, 16, 3, 768), 2), ((2, 24, 3, 1536), 2)]:
        for mode in ("train", "eval"):
            out.append((shape, h3, mode, None, {}))
    # bf16 operands
    for mode in ("train", "eval"):
        out.append(((3, 24, 3, 2048), 4, mode, None, {"WUNET_H3_NOSPLIT": "1"}))
    # frozen BatchNorm layers inside a training forward
    for shape, h3, sw in [((3, 8, 3, 64), 0, {}), ((2, 24, 1, 1024), 2, {}), ((3, 24, 3, 2048), 2, {"WUNET_H3_NOSPLIT": "1"}),
                          ((3, 24, 3, 2048), 2, {"WUNET_H3_NOSPLIT": "1", "WUNET_H3U": "256,256"})]:
        for name in ("first", "producer", "all"):
            out.append((shape, h3, "train", name, sw))
            out.append((shape, h3, "train_nosave", name, sw))
    return out


def profile_text(lib):
    buf = ctypes.create_string_buffer(1 << 16)
    lib.wunet_profile_collect(buf, len(buf))
    lib.wunet_profile_enable(0)
    return buf.value.decode()


def run_case(lib, shape, h3, mode, mask_name, switches):
    n, ci, B, T = shape
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(switches)
    eng = eng_mod.Engine(lib=lib, host_memory=True, h3=h3)
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)
    m = model_mod.Model(n_layers=n, channels_interval=ci, input_grad=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m._engine_override = eng
    res = {}
    lib.wunet_profile_enable(1)
    try:
        if mode in ("eval", "eval_cached"):
            m.eval()
            params = m._wunet_params()
            running, nbt = m._wunet_buffers()
            x = torch.from_numpy(noisy)
            with torch.no_grad():
                out, ws = eng.forward(n, ci, x, params, running, nbt, False, False)
                res["out"] = out.numpy().copy()
                if mode == "eval_cached":
                    # the engine only caches device workspaces: the second forward on the first one's packs through the C ABI
                    out2 = torch.empty_like(x)
                    with eng._using(n, ci, B, T, x.device) as h:
                        eng._check(lib.wunet_forward(h, x.data_ptr(), eng._ptrs(params), eng._ptrs(running), eng._ptrs(nbt), 0, 2,
                                                     ws.data_ptr(), out2.data_ptr(), None))
                    res["out_cached"] = out2.numpy().copy()
        else:
            m.train()
            if mask_name:
                for (_, bn), f in zip(m._leaves(), masks(n)[mask_name]):
                    bn.train(not f)
            if mode == "train_nosave":
                with torch.no_grad():
                    res["out"] = m(torch.from_numpy(noisy)).numpy().copy()
            else:
                crit = loss_mod.mse_loss()
                crit._engine_override = eng
                x = torch.from_numpy(noisy).requires_grad_(True)
                out = m(x)
                lv = crit(torch.from_numpy(clean), out)
                lv.backward()
                res["out"] = out.detach().numpy().copy()
                res["loss"] = np.float64(lv.item())
                res["grad_input"] = x.grad.numpy().copy()
                for k, p in m.named_parameters():
                    res["grad " + k] = p.grad.numpy().copy()
        for k, v in m.state_dict().items():
            if "running" in k or "num_batches" in k:
                res["buffer " + k] = v.numpy().copy()
    finally:
        res["profile"] = profile_text(lib)
    return res


# ------------------------------------------------------------------ the auxiliary entry points: losses, loader ops, chunks, resampling
CPU = torch.device("cpu")


def _loss_and_grad(crit, c, e):
    x = e.detach().clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    return {"loss": loss.detach().numpy().copy(), "grad": x.grad.numpy().copy()}


def aux_cases():
    """(label, run(engine) -> {name: array}) over the case tables of the tests (tests/*_cases.py): their shapes are the smallest at
    which these kernels can go wrong.  The losses run forward and backward; the spectral ones include a window shorter than n_fft
    (a, d) and three resolutions in one call (d: the backward accumulates)."""
    import chunks_cases as K
    import cspec_loss_cases as CS
    import estoi_cases as EC
    import mix_cases as M
    import resample_cases as RS
    import reverb_cases as RV
    import stft_loss_cases as S
    import stft_loss_ref
    import stoi_loss_cases as SL
    import stoi_ref
    out = []
    for name in S.EMU_CASES:
        rows, T, res = S.CASES[name]
        c, e = stft_loss_ref.pair(rows, T)
        out.append((f"stft_loss {name}", lambda eng, res=res, c=c, e=e: _loss_and_grad(S.criterion(eng, res), c, e)))
        for compress, weight in [k[1:] for k in CS.params((name,))]:
            out.append((f"cspec_loss {name} compress={compress} complex_weight={weight}", lambda eng, res=res, c=c, e=e, kw=dict(
                compress=compress, complex_weight=weight): _loss_and_grad(CS.criterion(eng, res, **kw), c, e)))
    rows, T, res = S.CASES["a"]
    mags = importlib.import_module(PKG + ".metrics").stft_magnitude
    out.append(("stft_magnitude a", lambda eng: {"mag": mags(stft_loss_ref.pair(rows, T)[1], *res[0], engine=eng).numpy().copy()}))
    for name in SL.CASES:
        c, e = stoi_ref.pair(*SL.CASES[name])
        fs = SL.CASES[name][2]
        out.append((f"stoi_loss {name}", lambda eng, fs=fs, c=c, e=e: _loss_and_grad(SL.make(eng, fs), c, e)))
        out.append((f"estoi_loss {name}", lambda eng, fs=fs, c=c, e=e: _loss_and_grad(EC.make_loss(eng, fs), c, e)))

    def mix(eng, name):
        m, cl, gains = M.run(eng, CPU, name)
        level = eng.apply_level(m.clone(), gains)                              # (in place on a copy: the multiply of clean_out)
        return {"mixture": m.numpy().copy(), "clean": cl.numpy().copy(), "gains": gains.numpy().copy(), "level": level.numpy().copy()}

    def reverb(eng, name):
        rev, direct = RV.run(eng, CPU, name)
        return {"reverberant": rev.numpy().copy(), "direct": direct.numpy().copy(), "alone": RV.run(eng, CPU, name, with_direct=False)[0].numpy().copy()}

    def chunks(eng, name, window):
        L, m, f, lengths = K.CASES[name]
        return {f"T={T}": K.enhance_one(eng, CPU, K.recording(T), L, m, f, window, K.Stub(L)).numpy().copy() for T in lengths}

    def resample(eng, name):
        rate_in, rate_out, T = RS.CASES[name]
        x = torch.from_numpy(np.stack([RS.signal(T), RS.signal(T, seed=1)]))
        return {"out": RS.resample_mod().resample(x, rate_in, rate_out, engine=eng).numpy().copy()}

    def resample_ragged(eng, rates):
        """RS.run_table's layout (rows at odd offsets of guarded arrays) without its oracle."""
        rs = RS.resample_mod()
        rows = [(T, rs.resampled_length(T, *rates)) for T in RS.RAGGED]
        ins, in_total = RS.odd_layout([r[0] for r in rows])
        outs, out_total = RS.odd_layout([r[1] for r in rows], first=3)
        src = np.full(in_total, K.SENTINEL, np.float32)
        for k, ((T, _), s) in enumerate(zip(rows, ins)):
            src[s:s + T] = RS.signal(T, seed=k % 3)
        table = torch.from_numpy(np.asarray([(a, T, b, To) for (T, To), a, b in zip(rows, ins, outs)], np.int64))
        out = torch.full((out_total,), K.SENTINEL)
        eng.resample_rows(torch.from_numpy(src), table, out, *rates, max(r[1] for r in rows))
        return {"out": out.numpy().copy()}

    out += [(f"mix_windows + apply_level {name}", lambda eng, name=name: mix(eng, name)) for name in M.CASES]
    out += [(f"reverb_windows {name}", lambda eng, name=name: reverb(eng, name)) for name in RV.CASES]
    out += [(f"chunk_gather + chunk_overlap_add {name} {w}", lambda eng, name=name, w=w: chunks(eng, name, w)) for name in K.CASES for w in K.WINDOWS]
    out += [(f"resample_rows {name}", lambda eng, name=name: resample(eng, name)) for name in RS.CASES]
    out += [(f"resample_rows ragged {r[0]} -> {r[1]}", lambda eng, r=r: resample_ragged(eng, r)) for r in RS.RAGGED_RATES]
    return out


def run_aux(lib, fn):
    eng = eng_mod.Engine(lib=lib, host_memory=True)
    lib.wunet_profile_enable(1)
    res = {}
    try:
        res = fn(eng)
    finally:
        res["profile"] = profile_text(lib)
    return res


def refusals():
    """(entry point, arguments): one bad argument per refusal of the auxiliary entry points; every other argument is valid (P: a zeroed,
    64-byte aligned MiB, large enough for the shapes here should a call go through).  Compared: the return value and wunet_last_error()."""
    raw = ctypes.create_string_buffer((1 << 20) + 64)
    P = (ctypes.addressof(raw) + 63) & ~63
    refusals.keep = raw
    nan, big = float("nan"), 1 << 62
    ints = lambda *v: ctypes.cast((ctypes.c_int * len(v))(*v), ctypes.c_void_p)                     # noqa: E731
    ptrs = lambda *v: ctypes.cast((ctypes.c_void_p * len(v))(*v), ctypes.c_void_p)                  # noqa: E731
    out = []
    # one resolution on 2 rows of 100 samples: n_fft 64, hop 16, window 48
    shapes = [(2, 0, 64, 16, 48), (2, 100, 60, 16, 48), (2, 100, 8192, 16, 48), (2, 100, 64, 0, 48), (2, 100, 64, 65, 48), (0, 100, 64, 16, 48),
              (2, 20, 64, 16, 48), (1 << 30, 100, 64, 16, 48), (2, 1 << 30, 64, 16, 48), (1 << 29, 256, 64, 1, 48)]
    for fam in ("stft", "cspec"):
        for R, T, N, H, W in shapes:                          # (the size queries and finalize do not take the window)
            out.append((f"wunet_{fam}_scratch_bytes", (R, T, N, H, 1)))
            out.append((f"wunet_{fam}_saved_bytes", (R, T, N, H)))
            out.append((f"wunet_{fam}_finalize", (1, ptrs(P), R, T, ints(N), ints(H)) + ((1.0, 1.0) if fam == "stft" else (0.3,)) + (P, P, None)))
    shapes += [(2, 100, 64, 16, 0), (2, 100, 64, 16, 65)]
    fwd = lambda a, b, clamp, basis, scr, sv, mag, shape=(2, 100, 64, 16, 48): ("wunet_stft_forward", (a, b) + shape + (clamp, basis, scr, sv, mag, None))   # noqa: E731
    out += [fwd(P, P, 1e-7, P, P, P, None, s) for s in shapes]
    out += [fwd(P, None, 1e-7, P, P, P, None), fwd(P, P, 1e-7, None, P, P, None), fwd(P, P, 1e-7, P + 4, P, P, None), fwd(P, P, 0.0, P, P, P, None),
            fwd(P, P, nan, P, P, P, None), fwd(P, P, 1e39, P, P, P, None), fwd(P, P, 1e-7, P, None, P, None), fwd(None, P, -1.0, P, None, None, P),
            fwd(None, P, 0.0, P, None, None, None), fwd(None, P, 0.0, P, None, P, P)]
    fin = lambda *a: ("wunet_stft_finalize", a + (None,))                      # noqa: E731
    out += [fin(0, ptrs(P), 2, 100, ints(64), ints(16), 1.0, 1.0, P, P), fin(9, ptrs(*[P] * 9), 2, 100, ints(*[64] * 9), ints(*[16] * 9), 1.0, 1.0, P, P),
            fin(1, None, 2, 100, ints(64), ints(16), 1.0, 1.0, P, P), fin(1, ptrs(P), 2, 100, None, ints(16), 1.0, 1.0, P, P),
            fin(1, ptrs(P), 2, 100, ints(64), None, 1.0, 1.0, P, P), fin(1, ptrs(P), 2, 100, ints(64), ints(16), 1.0, 1.0, None, P),
            fin(1, ptrs(P), 2, 100, ints(64), ints(16), nan, 1.0, P, P), fin(1, ptrs(P), 2, 100, ints(64), ints(16), 1.0, nan, P, P),
            fin(2, ptrs(P, None), 2, 100, ints(64, 64), ints(16, 16), 1.0, 1.0, P, P), fin(2, ptrs(P, P), 2, 100, ints(64, 60), ints(16, 16), 1.0, 1.0, P, P)]
    bwd = lambda sv, co, gl, clamp, basis, scr, g, shape=(2, 100, 64, 16, 48): ("wunet_stft_backward", (sv, co, gl) + shape + (clamp, basis, scr, g, 0, None))   # noqa: E731
    out += [bwd(P, P, P, 1e-7, P, P, P, s) for s in shapes]
    out += [bwd(None, P, P, 1e-7, P, P, P), bwd(P, None, P, 1e-7, P, P, P), bwd(P, P, None, 1e-7, P, P, P), bwd(P, P, P, 1e-7, None, P, P),
            bwd(P, P, P, 1e-7, P + 4, P, P), bwd(P, P, P, 1e-7, P, None, P), bwd(P, P, P, 1e-7, P, P, None), bwd(P, P, P, 0.0, P, P, P),
            bwd(P, P, P, nan, P, P, P)]
    # the compressed spectral loss on the same shape: 14 frames, 64 padded bins, 2 partials per block
    n_scr, n_bwd, n_sv = (1 << 20), (1 << 20), 5 * 14 * 64 * 4
    cf = lambda a, b, compress, clamp, basis, scr, nscr, sv, nsv, shape=(2, 100, 64, 16, 48): (         # noqa: E731
        "wunet_cspec_forward", (a, b) + shape + (compress, clamp, basis, scr, nscr, sv, nsv, None))
    out += [cf(P, P, 0.3, 1e-7, P, P, n_scr, P, n_sv, s) for s in shapes]
    out += [cf(P, P, 0.0, 1e-7, P, P, n_scr, P, n_sv), cf(P, P, 1.5, 1e-7, P, P, n_scr, P, n_sv), cf(P, P, nan, 1e-7, P, P, n_scr, P, n_sv),
            cf(P, P, 0.3, 0.0, P, P, n_scr, P, n_sv), cf(P, P, 0.3, 1e39, P, P, n_scr, P, n_sv), cf(None, P, 0.3, 1e-7, P, P, n_scr, P, n_sv),
            cf(P, None, 0.3, 1e-7, P, P, n_scr, P, n_sv), cf(P, P, 0.3, 1e-7, None, P, n_scr, P, n_sv), cf(P, P, 0.3, 1e-7, P + 4, P, n_scr, P, n_sv),
            cf(P, P, 0.3, 1e-7, P, None, n_scr, P, n_sv), cf(P, P, 0.3, 1e-7, P, P, 8, P, n_sv), cf(P, P, 0.3, 1e-7, P, P, n_scr, P, n_sv - 4),
            cf(P, P, 0.3, 1e-7, P, P, n_scr, None, n_sv)]
    cfin = lambda *a: ("wunet_cspec_finalize", a + (None,))                   # noqa: E731
    out += [cfin(0, ptrs(P), 2, 100, ints(64), ints(16), 0.3, P, P), cfin(9, ptrs(*[P] * 9), 2, 100, ints(*[64] * 9), ints(*[16] * 9), 0.3, P, P),
            cfin(1, None, 2, 100, ints(64), ints(16), 0.3, P, P), cfin(1, ptrs(P), 2, 100, None, ints(16), 0.3, P, P),
            cfin(1, ptrs(P), 2, 100, ints(64), None, 0.3, P, P), cfin(1, ptrs(P), 2, 100, ints(64), ints(16), 0.3, None, P),
            cfin(1, ptrs(P), 2, 100, ints(64), ints(16), -0.1, P, P), cfin(1, ptrs(P), 2, 100, ints(64), ints(16), 1.5, P, P),
            cfin(1, ptrs(P), 2, 100, ints(64), ints(16), nan, P, P), cfin(2, ptrs(P, None), 2, 100, ints(64, 64), ints(16, 16), 0.3, P, P),
            cfin(2, ptrs(P, P), 2, 100, ints(64, 60), ints(16, 16), 0.3, P, P)]
    cb = lambda sv, nsv, co, gl, compress, clamp, basis, scr, nscr, g, shape=(2, 100, 64, 16, 48): (    # noqa: E731
        "wunet_cspec_backward", (sv, nsv, co, gl) + shape + (compress, clamp, basis, scr, nscr, g, 0, None))
    out += [cb(P, n_sv, P, P, 0.3, 1e-7, P, P, n_bwd, P, s) for s in shapes]
    out += [cb(P, n_sv, P, P, 0.0, 1e-7, P, P, n_bwd, P), cb(P, n_sv, P, P, 0.3, 0.0, P, P, n_bwd, P), cb(None, n_sv, P, P, 0.3, 1e-7, P, P, n_bwd, P),
            cb(P, n_sv, None, P, 0.3, 1e-7, P, P, n_bwd, P), cb(P, n_sv, P, None, 0.3, 1e-7, P, P, n_bwd, P), cb(P, n_sv, P, P, 0.3, 1e-7, None, P, n_bwd, P),
            cb(P, n_sv, P, P, 0.3, 1e-7, P + 4, P, n_bwd, P), cb(P, n_sv, P, P, 0.3, 1e-7, P, P, n_bwd, None), cb(P, n_sv + 4, P, P, 0.3, 1e-7, P, P, n_bwd, P),
            cb(P, n_sv, P, P, 0.3, 1e-7, P, None, n_bwd, P), cb(P, n_sv, P, P, 0.3, 1e-7, P, P, 64, P)]
    # row losses (kind 3: SI-SDR)
    rf = lambda kind, eps, c, e, R, T, loss, scr: ("wunet_loss_rows_forward", (kind, 1, eps, c, e, R, T, loss, None, None, scr, None))   # noqa: E731
    rb = lambda kind, c, e, co, gl, R, T, g: ("wunet_loss_rows_backward", (kind, c, e, co, gl, R, T, g, None))                           # noqa: E731
    out += [rf(2, 1e-8, P, P, 2, 100, P, P), rf(3, 1e-8, P, P, 0, 100, P, P), rf(3, 1e-8, P, P, 2, 0, P, P), rf(3, 1e-8, P, P, 1 << 30, 100, P, P),
            rf(3, 1e-8, P, P, 2, 1 << 40, P, P), rf(3, 1e-8, None, P, 2, 100, P, P), rf(3, 1e-8, P, P, 2, 100, P, None), rf(3, -1.0, P, P, 2, 100, P, P),
            rf(3, nan, P, P, 2, 100, P, P), rb(5, P, P, P, P, 2, 100, P), rb(4, P, P, P, P, 0, 100, P), rb(4, P, P, P, P, 2, 1 << 40, P),
            rb(4, P, P, None, P, 2, 100, P), rb(4, P, P, P, P, 2, 100, None)]
    out += [("wunet_loss_rows_scratch_bytes", (0, 100)), ("wunet_loss_rows_scratch_bytes", (2, 0))]
    # the loader ops: 2 windows of 8 samples out of arrays of 64
    out += [("wunet_mix_scratch_bytes", s) for s in [(0, 8), (2, 0), (65536, 8), (2, (1 << 30) + 1)]]
    mw = lambda cl, ct, no, nt, rows, par, peak, B, L, scr, m, c: ("wunet_mix_windows", (cl, ct, no, nt, rows, par, peak, B, L, scr, m, c, None, None))   # noqa: E731
    out += [mw(P, 64, P, 64, P, P, 0.99, 0, 8, P, P, P), mw(P, 64, P, 64, P, P, 0.99, 2, 0, P, P, P), mw(P, 64, P, 64, P, P, 0.99, 65536, 8, P, P, P),
            mw(P, 1 << 40, P, 64, P, P, 0.99, 2, (1 << 30) + 1, P, P, P), mw(P, 7, P, 64, P, P, 0.99, 2, 8, P, P, P), mw(P, 64, P, 0, P, P, 0.99, 2, 8, P, P, P),
            mw(P, 1 << 60, P, 64, P, P, 0.99, 2, 8, P, P, P), mw(P, 64, P, 1 << 60, P, P, 0.99, 2, 8, P, P, P), mw(None, 64, P, 64, P, P, 0.99, 2, 8, P, P, P),
            mw(P, 64, P, 64, None, P, 0.99, 2, 8, P, P, P), mw(P, 64, P, 64, P, P, 0.99, 2, 8, None, P, P), mw(P, 64, P, 64, P, P, 0.99, 2, 8, P, P, None),
            mw(P, 64, P, 64, P, P, nan, 2, 8, P, P, P), mw(P, 64, P, 64, P, P, 0.99, 2, 8, P + 4, P, P), mw(P, 64, P, 64, P, P, 0.99, 2, 8, P, P + 4, P),
            mw(P, 64, P, 64, P, P, 0.99, 2, 8, P, P, P + 8)]
    al = lambda src, gains, B, L, dst: ("wunet_apply_level", (src, gains, B, L, dst, None))       # noqa: E731
    out += [al(P, P, 0, 8, P), al(P, P, 2, 0, P), al(P, P, 65536, 8, P), al(P, P, 2, (1 << 30) + 1, P), al(None, P, 2, 8, P), al(P, None, 2, 8, P),
            al(P, P, 2, 8, None), al(P + 4, P, 2, 8, P), al(P, P, 2, 8, P + 4)]
    rv = lambda cl, ct, rir, rt, rows, early, B, L, rev, direct: ("wunet_reverb_windows", (cl, ct, rir, rt, rows, early, B, L, rev, direct, None))   # noqa: E731
    out += [rv(P, 64, P, 64, P, 1, 0, 8, P, P), rv(P, 64, P, 64, P, 1, 2, 0, P, P), rv(P, 64, P, 64, P, 1, 65536, 8, P, P),
            rv(P, 1 << 40, P, 64, P, 1, 2, (1 << 30) + 1, P, P), rv(P, 7, P, 64, P, 1, 2, 8, P, P), rv(P, 64, P, 0, P, 1, 2, 8, P, P),
            rv(P, 1 << 60, P, 64, P, 1, 2, 8, P, P), rv(P, 64, P, 1 << 60, P, 1, 2, 8, P, P), rv(None, 64, P, 64, P, 1, 2, 8, P, P),
            rv(P, 64, None, 64, P, 1, 2, 8, P, P), rv(P, 64, P, 64, None, 1, 2, 8, P, P), rv(P, 64, P, 64, P, 1, 2, 8, None, P),
            rv(P, 64, P, 64, P, 0, 2, 8, P, P), rv(P, 64, P, 64, P, 1, 2, 8, P + 4, P), rv(P, 64, P, 64, P, 1, 2, 8, P, P + 4)]
    # the chunk ops: 2 chunks of 16 samples, margin 2, fade 4 (hop 8)
    cg = lambda flat, total, rows, n, L, chunks: ("wunet_chunk_gather", (flat, total, rows, n, L, chunks, None))          # noqa: E731
    out += [cg(P, 64, P, 0, 16, P), cg(P, 64, P, 2, 0, P), cg(P, 64, P, 1 << 31, 16, P), cg(P, 64, P, 2, (1 << 30) + 1, P), cg(P, 0, P, 2, 16, P),
            cg(P, big, P, 2, 16, P), cg(None, 64, P, 2, 16, P), cg(P, 64, None, 2, 16, P), cg(P, 64, P, 2, 16, None)]
    co = lambda ch, n, L, m, f, ramp, recs, nrec, maxlen, out_, total: ("wunet_chunk_overlap_add", (ch, n, L, m, f, ramp, recs, nrec, maxlen, out_, total, None))   # noqa: E731
    out += [co(P, 0, 16, 2, 4, P, P, 1, 24, P, 64), co(P, 2, 0, 2, 4, P, P, 1, 24, P, 64), co(P, 1 << 31, 16, 2, 4, P, P, 1, 24, P, 64),
            co(P, 2, (1 << 30) + 1, 2, 4, P, P, 1, 24, P, 64), co(P, 2, 16, -1, 4, P, P, 1, 24, P, 64), co(P, 2, 16, 2, -1, P, P, 1, 24, P, 64),
            co(P, 2, 16, 8, 0, None, P, 1, 24, P, 64), co(P, 2, 16, 2, 7, P, P, 1, 24, P, 64), co(P, 2, 16, 2, 4, None, P, 1, 24, P, 64),
            co(P, 2, 16, 2, 0, P, P, 1, 24, P, 64), co(P, 2, 16, 2, 4, P, P, 0, 24, P, 64), co(P, 2, 16, 2, 4, P, P, 1 << 31, 24, P, 64),
            co(P, 2, 16, 2, 4, P, P, 1, 0, P, 64), co(P, 2, 16, 2, 4, P, P, 1, big, P, 64), co(P, 2, 16, 2, 4, P, P, 1, 24, P, 0),
            co(P, 2, 16, 2, 4, P, P, 1, 24, P, big), co(None, 2, 16, 2, 4, P, P, 1, 24, P, 64), co(P, 2, 16, 2, 4, P, None, 1, 24, P, 64),
            co(P, 2, 16, 2, 4, P, P, 1, 24, None, 64)]
    # resampling: 2 rows, 1 / 3 with 21 taps
    rr = lambda i, it, rows, n, mo, up, down, taps, nt, o, ot: ("wunet_resample_rows", (i, it, rows, n, mo, up, down, taps, nt, o, ot, None))   # noqa: E731
    out += [rr(P, 64, P, 0, 8, 1, 3, P, 21, P, 64), rr(P, 64, P, 2, 0, 1, 3, P, 21, P, 64), rr(P, 64, P, 1 << 31, 8, 1, 3, P, 21, P, 64),
            rr(P, 64, P, 2, 8, 0, 3, P, 21, P, 64), rr(P, 64, P, 2, 8, 1, 0, P, 21, P, 64), rr(P, 64, P, 2, 8, 2, 4, P, 21, P, 64),
            rr(P, 64, P, 2, 8, 1, 100000, P, 21, P, 64), rr(P, 64, P, 2, 8, 1, 3, P, 20, P, 64), rr(P, 64, P, 2, 8, 1, 3, P, 0, P, 64),
            rr(P, 64, P, 2, 8, 1, 3, P, (1 << 24) + 1, P, 64), rr(P, 0, P, 2, 8, 1, 3, P, 21, P, 64), rr(P, big, P, 2, 8, 1, 3, P, 21, P, 64),
            rr(P, 64, P, 2, 8, 1, 3, P, 21, P, 0), rr(P, 64, P, 2, 8, 1, 3, P, 21, P, big), rr(None, 64, P, 2, 8, 1, 3, P, 21, P, 64),
            rr(P, 64, None, 2, 8, 1, 3, P, 21, P, 64), rr(P, 64, P, 2, 8, 1, 3, None, 21, P, 64), rr(P, 64, P, 2, 8, 1, 3, P, 21, None, 64)]
    out += [("wunet_resample_tile", (0, 3, 21)), ("wunet_resample_tile", (2, 4, 21)), ("wunet_resample_tile", (1, 3, 20))]
    return out


def compare_refusals(libs):
    """Every call of refusals() on both libraries, in one order: (return value, wunet_last_error()) must agree and the call be refused."""
    differing, table, seen = 0, refusals(), set()
    for name, args in table:
        got = []
        for L in libs:
            rc = getattr(L, name)(*args)
            got.append((rc, L.wunet_last_error().decode()))
        seen.add(got[1])
        refused = all((rc == 0) if name.endswith(("_bytes", "_tile")) else (rc != 0) for rc, _ in got)
        if got[0] != got[1] or not refused:
            differing += 1
            print(f"DIFF  {name}{args}: base {got[0]}  new {got[1]}{'' if refused else '  (not refused)'}")
    print(f"{len(table)} refused calls, {len(seen)} distinct (return value, message) pairs, {differing} differing")
    if os.environ.get("EMU_LIB_AB_VERBOSE"):
        for rc, msg in sorted(seen, key=str):
            print(f"      {rc}: {msg}")
    return differing


def compare_adam(libs):
    """The fused Adam step through both C entry points (tools/adam_lib_ab.py: its cases, its refusals): parameters, both moments, the
    hyper buffer and the step counter after 4 steps, array by array; the refusals by return value and message."""
    import adam_lib_ab as AB
    differing, table = 0, AB.adam_cases()
    for label, *case in table:
        a, b = (AB.run_adam(L, "cpu", *case) for L in libs)
        bad = [k for k in a if not np.array_equal(a[k], b[k])]
        print(f"{'DIFF' if bad else 'same'}  {label}  [{len(a)} arrays {AB.digest(b)}]", flush=True)
        for k in bad:
            print("      differs:", k)
        differing += bool(bad)
    ra, rb = (AB.adam_refusals(L) for L in libs)
    bad = [(x, y) for x, y in zip(ra, rb) if x != y or y[2] == "NOT REFUSED"]
    for x, y in bad:
        print(f"DIFF  {x[0]}: base {x[1:]}  new {y[1:]}")
    print(f"{len(table)} Adam cases, {len(rb)} refused Adam calls, {len(set(r[1:] for r in rb))} distinct (return value, message) pairs, "
          f"{differing + len(bad)} differing")
    return differing + len(bad)


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    base_path = os.path.realpath(sys.argv[1])
    if len(sys.argv) > 2:
        new_path = os.path.realpath(sys.argv[2])
    else:
        import emu_lib
        emu_lib.lib()
        new_path = os.path.realpath(os.path.join(ROOT, "tests", "emu", "libwunet_emu.so"))
    assert base_path != new_path, "the two libraries are one file"
    libs = [lib_mod.declare(ctypes.CDLL(p)) for p in (base_path, new_path)]
    assert libs[0]._handle != libs[1]._handle
    for L in libs:
        L.wunet_last_error.restype = ctypes.c_char_p
        L.wunet_workspace_bytes.restype = ctypes.c_size_t
    differing, kernels = 0, set()
    table = [] if os.environ.get("EMU_LIB_AB_AUX_ONLY") else cases()
    aux = aux_cases()
    for label, fn in aux:
        a, b = (run_aux(L, fn) for L in libs)
        bad = [k for k in a if k not in b or not np.array_equal(a[k], b[k])] + [k for k in b if k not in a]
        kernels.update(ln.split("\t")[0] for ln in b["profile"].splitlines())
        digest = hashlib.sha1(b"".join(np.ascontiguousarray(b[k]).tobytes() for k in sorted(b) if k != "profile")).hexdigest()[:12]
        print(f"{'DIFF' if bad else 'same'}  {label}  [{len(a) - 1} arrays {digest}, {len(a['profile'].splitlines())} kernel names]", flush=True)
        for k in bad:
            print("      differs:", k)
        differing += bool(bad)
    differing += compare_refusals(libs)
    differing += compare_adam(libs)
    for shape, h3, mode, mask_name, switches in table:
        a, b = (run_case(L, shape, h3, mode, mask_name, switches) for L in libs)
        bad = [k for k in a if k not in b or not np.array_equal(a[k], b[k])] + [k for k in b if k not in a]
        kernels.update(ln.split("\t")[0] for ln in b["profile"].splitlines())
        tag = " ".join(f"{k}={v}" for k, v in switches.items())
        print(f"{'DIFF' if bad else 'same'}  {shape} h3={h3} {mode}{' frozen=' + mask_name if mask_name else ''} {tag}  "
              f"[{len(a) - 1} arrays, {len(a['profile'].splitlines())} kernel names]", flush=True)
        for k in bad:
            print("      differs:", k)
            if k == "profile":
                print("      base:", a[k].replace("\n", " | "))
                print("      new: ", b[k].replace("\n", " | "))
        differing += bool(bad)
    print("kernel names seen:", ", ".join(sorted(kernels)))
    print(f"{len(table)} network cases, {len(aux)} auxiliary cases and the refusals: {differing} differing")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
