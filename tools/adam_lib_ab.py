#!/usr/bin/env python
"""The fused Adam step of ONE build of the library, through the C entry points, as one hash per case.

    python tools/adam_lib_ab.py LIB.so [cpu|cuda]      (cpu: an emulator library on host memory; cuda: libwunet_hip.so on the device)

For a change of the optimiser's kernels or host path: run it on the library of the parent commit and on the new one, each in a
process of its own, and compare the two outputs as text - identical lines are identical bits.  Cases (adam_cases): both entry
points (wunet_adam_step, wunet_adam_step_ex); the step count on the host and on the device; with _ex every optional part alone
(clipping, decoupled decay, the lr from device memory), none of them and all together; grad_scale 1 and 0.5; both case tables
of tests/adam_options_ref.py with its 4 steps of gradients and lrs.  Hashed per case: every parameter, both moments, the hyper
buffer (8 floats, pre-filled with a sentinel: what a call does not write stays in the hash) and the step counter.  The last line
hashes the refusals (adam_refusals: one bad argument per call) by return value and wunet_last_error().
tools/emu_lib_ab.py runs the same cases on two emulator libraries in one process and compares the arrays themselves."""
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
import adam_options_ref as R                                # noqa: E402

SENTINEL = -123.0
OPTIONS = {"none": (), "clip": ("clip",), "decay": ("decay",), "device_lr": ("lr",), "all": ("clip", "decay", "lr")}


def adam_cases():
    """(label, case table, entry point, device_step, optional parts, grad_scale)"""
    out = []
    for case in R.CASES:
        for device_step in (False, True):
            for gs in (1.0, 0.5):
                tail = f"{case} {'device' if device_step else 'host'}_step grad_scale={gs}"
                out.append((f"adam_step {tail}", case, "plain", device_step, (), gs))
                out += [(f"adam_step_ex {name} {tail}", case, "ex", device_step, parts, gs) for name, parts in OPTIONS.items()]
    return out


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]), ctypes.c_void_p)


def run_adam(lib, device, case, entry, device_step, parts, gs):
    """R.STEPS steps on `device`; returns {name: array}.  A refused call raises."""
    dev = torch.device(device)
    p = [t.clone().to(dev) for t in R.initial(case)]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    n = len(p)
    numels = (ctypes.c_size_t * n)(*[t.numel() for t in p])
    hyper = torch.full((8,), SENTINEL, device=dev)
    counter = torch.zeros((), dtype=torch.int64, device=dev)
    lr_dev = torch.zeros((), dtype=torch.float64, device=dev)
    scratch = torch.zeros(max(int(lib.wunet_adam_scratch_bytes(n)) // 8, 1), dtype=torch.float64, device=dev)
    ctr = counter.data_ptr() if device_step else None
    for it in range(R.STEPS):
        g = [t.to(dev) for t in R.gradients(case)[it]]
        lr = R.LRS[it]
        if entry == "plain":
            rc = lib.wunet_adam_step(n, _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), numels, lr, *R.BETAS, R.EPS, it + 1, gs, ctr,
                                     hyper.data_ptr() if device_step else None, None)
        else:
            lr_dev.fill_(lr)
            rc = lib.wunet_adam_step_ex(n, _ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), numels, -1.0 if "lr" in parts else lr, *R.BETAS, R.EPS, it + 1, gs,
                                        R.WEIGHT_DECAY if "decay" in parts else 0.0, R.MAX_NORM if "clip" in parts else 0.0, ctr, hyper.data_ptr(),
                                        lr_dev.data_ptr() if "lr" in parts else None, scratch.data_ptr() if "clip" in parts else None, None)
        if rc != 0:
            raise RuntimeError(f"rc={rc}: {lib.wunet_last_error().decode()}")
        if dev.type == "cuda":
            torch.cuda.synchronize()                           # (the gradients of this step are released after it)
    cat = lambda ts: torch.cat([t.reshape(-1) for t in ts]).cpu().numpy()     # noqa: E731
    return {"params": cat(p), "exp_avg": cat(m), "exp_avg_sq": cat(v), "hyper": hyper.cpu().numpy(), "counter": counter.cpu().numpy()}


def adam_refusals(lib):
    """[(label, return value, message)]: one bad argument per call of both entry points, on 1 tensor of 4 host floats (nothing is
    enqueued by a refused call; a call that goes through is reported as such and makes the comparison fail)."""
    t = [torch.zeros(4) for _ in range(4)]
    one = lambda x: _ptrs([x])                                                 # noqa: E731
    numels, huge = (ctypes.c_size_t * 1)(4), (ctypes.c_size_t * 1)(1 << 32)
    hyper, ctr, scr = torch.zeros(8), torch.zeros((), dtype=torch.int64), torch.zeros(256, dtype=torch.float64)
    H, C, S, nan = hyper.data_ptr(), ctr.data_ptr(), scr.data_ptr(), float("nan")
    A = (one(t[0]), one(t[1]), one(t[2]), one(t[3]))
    hp = (1e-3, 0.9, 0.999, 1e-8)
    plain = lambda n, a, ne, step, c, h: ("wunet_adam_step", (n,) + a + (ne,) + hp + (step, 1.0, c, h, None))                       # noqa: E731
    ex = lambda n, a, ne, step, wd, mn, c, h, s: ("wunet_adam_step_ex", (n,) + a + (ne,) + hp + (step, 1.0, wd, mn, c, h, None, s, None))   # noqa: E731
    calls = [plain(-1, A, numels, 1, None, None), plain(1, (None,) + A[1:], numels, 1, None, None), plain(1, A, None, 1, None, None),
             plain(1, A, numels, 0, None, None), plain(1, A, numels, 1, C, None), plain(1, A, huge, 1, None, None), plain(1, A, huge, 1, C, H),
             ex(-1, A, numels, 1, 0.0, 0.0, None, H, None), ex(1, A[:3] + (None,), numels, 1, 0.0, 0.0, None, H, None),
             ex(1, A, numels, 1, 0.0, 0.0, None, None, None), ex(1, A, numels, 0, 0.0, 0.0, None, H, None), ex(1, A, numels, 1, -0.1, 0.0, C, H, None),
             ex(1, A, numels, 1, nan, 0.0, C, H, None), ex(1, A, numels, 1, 0.0, nan, C, H, S), ex(1, A, numels, 1, 0.0, 1.0, C, H, None),
             ex(1, A, huge, 1, 0.01, 1.0, C, H, S)]
    out = []
    for name, args in calls:
        rc = getattr(lib, name)(*args)
        shown = tuple(a if a is None or isinstance(a, float) or (isinstance(a, int) and abs(a) < 256) else "*" for a in args)      # (no addresses)
        out.append((f"{name}{shown}", rc,
                    lib.wunet_last_error().decode() if rc != 0 else "NOT REFUSED"))
    assert int(ctr) == 0 and not hyper.any() and not any(x.any() for x in t), "a refused call ran"
    return out


def digest(res):
    return hashlib.sha1(b"".join(np.ascontiguousarray(res[k]).tobytes() for k in sorted(res))).hexdigest()[:16]


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    lib = importlib.import_module(PKG + "._lib").declare(ctypes.CDLL(os.path.realpath(sys.argv[1])))
    lib.wunet_last_error.restype = ctypes.c_char_p
    device = sys.argv[2] if len(sys.argv) > 2 else "cuda"
    for label, *case in adam_cases():
        print(digest(run_adam(lib, device, *case)), label, flush=True)
    ref = adam_refusals(lib)
    print(hashlib.sha1(repr(ref).encode()).hexdigest()[:16], f"{len(ref)} refusals", flush=True)
    return 1 if any(msg == "NOT REFUSED" for _, _, msg in ref) else 0


if __name__ == "__main__":
    sys.exit(main())
