"""The case table of the mel loss, shared by tests/test_mel_loss_emu.py (CPU emulator) and tests/test_gpu_mel_loss.py (MI355X): what
runs, on which tensors, and the checks against tests/mel_loss_ref.py.  `engine` None = the product's default engine.  The shapes are
the STFT loss's (tests/stft_loss_cases.py), because the DFT GEMMs are shared; the n_mels are chosen for the two mel GEMMs: below one
MFMA tile, a multiple of neither 16 nor 8, several column tiles, differing per resolution, the largest at the longest K."""
import importlib

import torch

import mel_loss_ref as R
from conftest import PKG_NAME
from stft_loss_cases import CASES as STFT_CASES


def _case(name, n_mels, **kw):
    rows, T, res = STFT_CASES[name]
    return rows, T, res, tuple(n_mels), tuple(sorted(kw.items()))


# name -> (rows, T, resolutions, n_mels per resolution, the knobs that differ from the defaults)
CASES = {
    "a": _case("a", (8,)),                                  # fewer frames than a 64-frame tile; n_mels below one MFMA tile; window < n_fft
    "b": _case("b", (20,)),                                 # n_mels a multiple of neither 16 nor 8; a hop that divides nothing
    "c": _case("c", (80,)),                                 # several K tiles (257 bins) and several column tiles of the projection
    "c2": _case("c", (80,), power=2, lin_weight=1.0),       # ... with the power spectrogram and the linear term
    "d": _case("d", (8, 20, 40)),                           # accumulation over resolutions with differing n_mels
    "e": _case("e", (128,)),                                # longest K (1025 bins) at the largest n_mels; GPU only
    "f": _case("f", (40,), mel_scale="htk", norm=None, fmin=50.0, fmax=7000.0),
    "f8": _case("f", (40,), sample_rate=8000),              # another sample rate, the defaults
    "g": _case("b", (48,), floor=1e-7),                     # a bank with one empty filter
}
EMU_CASES = ("a", "b", "d", "f", "f8", "g")
EMPTY_FILTERS = {"g": 1}                                    # every other case: none


def mods():
    return importlib.import_module(PKG_NAME + ".loss"), importlib.import_module(PKG_NAME + ".metrics")


def criterion(engine, resolutions, n_mels, **kw):
    import warnings
    loss_mod, _ = mods()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                     # (case g's empty filter; the warning has a test of its own)
        crit = loss_mod.mel_loss(fft_sizes=[r[0] for r in resolutions], hop_sizes=[r[1] for r in resolutions],
                                 win_lengths=[r[2] for r in resolutions], n_mels=list(n_mels), **kw)
    crit._engine_override = engine
    return crit


def run(engine, device, resolutions, n_mels, c, e, grad_loss=None, **kw):
    """loss(clean, enhanced) through the public module, backward with `grad_loss` (None: plain .backward()).
    Returns (loss, gradient w.r.t. enhanced)."""
    import warnings
    crit = criterion(engine, resolutions, n_mels, **kw)
    x = e.detach().to(device).requires_grad_(True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        loss = crit(c.to(device), x)
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, device=device))
    return loss.detach(), x.grad


def check_inputs(name):
    """The conditions the bars rest on, asserted on the float64 reference: at most 1e-4 of the bins of either signal have a power
    below 10 * clamp; at most 1e-4 of the cells under non-empty filters have m below 10 * floor; none of those cells has
    |l_c - l_e| < 1e-5 (a float32 computation may take the other side of the L1 kink there); the bank has the empty filters the table
    says."""
    ref = R.case_reference(*CASES[name])
    print(f"case {name}: share of bins below 10 * clamp {ref['low_share']:.2e}, of cells below 10 * floor {ref['low_mel_share']:.2e}, "
          f"smallest |l_c - l_e| {ref['min_gap']:.2e}, empty filters {ref['empty']}")
    assert ref["low_share"] <= 1e-4
    assert ref["low_mel_share"] <= 1e-4
    assert ref["min_gap"] >= 1e-5
    assert ref["empty"] == EMPTY_FILTERS.get(name, 0)
    return ref


def check_case(name, engine, device, c=None, e=None):
    """Loss and gradient of one case against the float64 oracle with the bars of mel_loss_ref.bars; c / e: the case's inputs at
    another address (the unaligned test).  Returns (loss, gradient)."""
    rows, T, res, n_mels, kw = CASES[name]
    ref = check_inputs(name)
    bar_l, bar_g = R.bars(ref)
    loss, g = run(engine, device, res, n_mels, ref["c"] if c is None else c, ref["e"] if e is None else e, **dict(kw))
    dl, dg = R.d_loss(loss, ref["loss"]), R.d_max(g.reshape(ref["grad"].shape), ref["grad"])
    print(f"case {name}: loss {float(loss):.8f}  d {dl:.2e} (d_ref {ref['d_loss']:.2e}, bar {bar_l:.2e});  "
          f"gradient d {dg:.2e} (d_ref {ref['d_grad']:.2e}, bar {bar_g:.2e})")
    assert g.shape == ref["e"].shape and g.dtype == torch.float32 and torch.isfinite(g).all()
    assert dl <= bar_l, (name, dl, bar_l)
    assert dg <= bar_g, (name, dg, bar_g)
    return loss, g


def check_spectrogram(name, engine, device):
    """metrics.mel_spectrogram of the case's `enhanced` at each of its resolutions, linear and log, against float64: 4 d_ref."""
    _, metrics = mods()
    rows, T, res, n_mels, kw = CASES[name]
    full = R.knobs(**dict(kw))
    args = {k: full[k] for k in ("sample_rate", "fmin", "fmax", "mel_scale", "norm", "power")}
    for (N, H, W), nm in zip(res, n_mels):
        for log in (False, True):
            ref = R.spectrogram_reference(rows, T, (N, H, W), nm, log, kw)
            mel = metrics.mel_spectrogram(ref["e"].to(device), n_fft=N, hop=H, win_length=W, n_mels=nm, log=log, floor=full["floor"],
                                          engine=engine, **args)
            assert mel.shape == (rows, 1 + T // H, nm) and mel.dtype == torch.float32 and mel.device.type == device.type
            dm = R.d_max(mel, ref["mel"])
            print(f"case {name} {(N, H, W)} n_mels {nm} log {log}: d {dm:.2e} (d_ref {ref['d_mel']:.2e}, bar {4.0 * ref['d_mel']:.2e})")
            assert dm <= 4.0 * ref["d_mel"], (name, (N, H, W), log, dm, ref["d_mel"])
