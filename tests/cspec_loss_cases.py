"""The case table of the compressed spectral loss, shared by tests/test_cspec_loss_emu.py (CPU emulator) and
tests/test_gpu_cspec_loss.py (MI355X): what runs, on which tensors, and the checks against tests/cspec_loss_ref.py.
`engine` None = the product's default engine.  The shapes are the STFT loss's (tests/stft_loss_cases.py): the two losses share the
GEMMs, so the smallest shapes at which those can go wrong are the same - a window shorter than n_fft, hops that divide nothing,
several K tiles, accumulation over resolutions, the longest K, n_fft = 320."""
import importlib

import torch

import cspec_loss_ref as R
from conftest import PKG_NAME
from stft_loss_cases import CASES

EMU_CASES = ("a", "b", "d", "f")
DEFAULT = (0.3, 0.3)                               # (compress, complex_weight)
EXTRA = ((1.0, 1.0), (0.5, 0.0))                   # the plain complex MSE; magnitude only - on cases a and d


def params(names):
    """(case, compress, complex_weight) of every run over `names`."""
    out = [(n,) + DEFAULT for n in names]
    for n in names:
        if n in ("a", "d"):
            out += [(n,) + k for k in EXTRA]
    return out


def loss_mod():
    return importlib.import_module(PKG_NAME + ".loss")


def criterion(engine, resolutions, **kw):
    crit = loss_mod().compressed_spectral_loss(fft_sizes=[r[0] for r in resolutions], hop_sizes=[r[1] for r in resolutions],
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


def check_inputs(name, compress, complex_weight):
    """The one condition the bars rest on: at most 1e-4 of the bins of either signal have a float64 power below 10 * clamp (near the
    clamp's kink every float32 computation, the yardsticks' too, may land on the other side)."""
    ref = R.case_reference(*CASES[name], compress, complex_weight)
    print(f"case {name}: share of bins below 10 * clamp {ref['low_share']:.2e}")
    assert ref["low_share"] <= 1e-4
    return ref


def check_case(name, compress, complex_weight, engine, device, c=None, e=None):
    """Loss and gradient of one case against the float64 oracle with the bars of cspec_loss_ref.bars; c / e: the case's inputs at
    another address (the unaligned test).  Returns (loss, gradient)."""
    rows, T, res = CASES[name]
    ref = check_inputs(name, compress, complex_weight)
    bar_l, bar_g = R.bars(ref)
    loss, g = run(engine, device, res, ref["c"] if c is None else c, ref["e"] if e is None else e, compress=compress,
                  complex_weight=complex_weight)
    dl, dg = R.d_loss(loss, ref["loss"]), R.d_max(g.reshape(ref["grad"].shape), ref["grad"])
    print(f"case {name} compress {compress} complex_weight {complex_weight}: loss {float(loss):.8f}  d {dl:.2e} "
          f"(d_ref {ref['d_loss']:.2e}, bar {bar_l:.2e});  gradient d {dg:.2e} (d_ref {ref['d_grad']:.2e}, bar {bar_g:.2e})")
    assert g.shape == ref["e"].shape and g.dtype == torch.float32 and torch.isfinite(g).all()
    assert dl <= bar_l, (name, dl, bar_l)
    assert dg <= bar_g, (name, dg, bar_g)
    return loss, g
