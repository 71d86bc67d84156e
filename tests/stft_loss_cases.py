"""The case table of the multi-resolution STFT loss, shared by tests/test_stft_loss_emu.py (CPU emulator) and
tests/test_gpu_stft_loss.py (MI355X): what runs, on which tensors, and the checks against tests/stft_loss_ref.py.
`engine` None = the product's default engine."""
import importlib

import torch

import stft_loss_ref as R
from conftest import PKG_NAME

# name -> (rows, T, ((n_fft, hop, win_length), ...)): the smallest shapes that exercise every way the kernels can go wrong
CASES = {
    "a": (3, 100, ((64, 16, 48),)),                                    # window shorter than n_fft; T a multiple of nothing; 7 frames
    "b": (2, 333, ((128, 50, 128),)),                                  # a hop that divides neither n_fft nor T
    "c": (2, 2048, ((512, 128, 512),)),                                # several K tiles; 257 bins
    "d": (4, 1024, ((64, 16, 48), (128, 50, 128), (256, 64, 200))),    # accumulation across resolutions
    "e": (1, 4096, ((2048, 240, 1200),)),                              # longest K; zero-window rows skipped (GPU only)
    "f": (2, 640, ((320, 160, 320),)),                                 # the reference's validation STFT; n_fft not a power of two
}
EMU_CASES = ("a", "b", "d", "f")


def mods():
    return importlib.import_module(PKG_NAME + ".loss"), importlib.import_module(PKG_NAME + ".metrics")


def criterion(engine, resolutions, **kw):
    loss_mod, _ = mods()
    crit = loss_mod.stft_loss(fft_sizes=[r[0] for r in resolutions], hop_sizes=[r[1] for r in resolutions],
                              win_lengths=[r[2] for r in resolutions], **kw)
    crit._engine_override = engine
    return crit


def run(engine, device, resolutions, c, e, grad_loss=None, **kw):
    """loss(clean, enhanced) through the public module, backward with `grad_loss` (None: plain .backward()).
    Returns (loss, gradient w.r.t. enhanced)."""
    crit = criterion(engine, resolutions, **kw)
    x = e.detach().to(device).requires_grad_(True)
    loss = crit(c.to(device), x)
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, device=device))
    return loss.detach(), x.grad


def check_inputs(name):
    """The one condition the bars rest on: at most 1e-4 of the bins have a float64 power below 10 * clamp (near the clamp's kink every
    float32 computation, the yardsticks' too, may land on the other side)."""
    ref = R.case_reference(*CASES[name])
    print(f"case {name}: share of bins below 10 * clamp {ref['low_share']:.2e}")
    assert ref["low_share"] <= 1e-4
    return ref


def check_case(name, engine, device, c=None, e=None):
    """Loss and gradient of one case against the float64 oracle with the bars of stft_loss_ref.bars; c / e: the case's inputs at
    another address (the unaligned test).  Returns (loss, gradient)."""
    rows, T, res = CASES[name]
    ref = check_inputs(name)
    bar_l, bar_g, _ = R.bars(ref)
    loss, g = run(engine, device, res, ref["c"] if c is None else c, ref["e"] if e is None else e)
    dl, dg = R.d_loss(loss, ref["loss"]), R.d_max(g.reshape(ref["grad"].shape), ref["grad"])
    print(f"case {name}: loss {float(loss):.8f}  d {dl:.2e} (d_ref {ref['d_loss']:.2e}, bar {bar_l:.2e});  "
          f"gradient d {dg:.2e} (d_ref {ref['d_grad']:.2e}, bar {bar_g:.2e})")
    assert g.shape == ref["e"].shape and g.dtype == torch.float32 and torch.isfinite(g).all()
    assert dl <= bar_l, (name, dl, bar_l)
    assert dg <= bar_g, (name, dg, bar_g)
    return loss, g


def check_magnitudes(name, engine, device):
    """metrics.stft_magnitude of the case's `enhanced` at each of its resolutions against |torch.stft| in float64."""
    _, metrics = mods()
    rows, T, res = CASES[name]
    ref = check_inputs(name)
    _, _, bar_m = R.bars(ref)
    for i, (N, H, W) in enumerate(res):
        mag = metrics.stft_magnitude(ref["e"].to(device), n_fft=N, hop=H, win_length=W, engine=engine)
        assert mag.shape == (rows, 1 + T // H, N // 2 + 1) and mag.dtype == torch.float32 and mag.device.type == device.type
        dm = R.d_max(mag, ref["mags"][i])
        print(f"case {name} {(N, H, W)}: magnitudes d {dm:.2e} (d_ref {ref['d_mag'][i]:.2e}, bar {bar_m[i]:.2e})")
        assert dm <= bar_m[i], (name, (N, H, W), dm, bar_m[i])
