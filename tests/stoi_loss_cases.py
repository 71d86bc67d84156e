"""The case table of the STOI loss, shared by tests/test_stoi_loss_emu.py (CPU emulator) and tests/test_gpu_stoi_loss.py (MI355X): the
six cases of tests/stoi_cases.py, what runs on them and the checks against tests/stoi_loss_ref.py.  `engine` None = the product's
default engine.  Conditions on the inputs are asserted before any comparison; the bars are
  loss      |loss - (-mean oracle64)| <= stoi_ref.bar (4 d_ref + 2^-23 of the scores) and |loss + mean metrics.stoi| <= 2^-22;
  gradient  per row with >= 30 frames: max_t |g - g64| <= 4 d_ref max_t |g64|, d_ref the case's maximum over those rows and over both
            float32 yardsticks of max_t |g32 - g64| / max_t |g64|, measured on the CPU at test time and printed beside every d;
  zeros     short rows: g == 0 exactly and the row's score 1e-5; at 10 kHz: g == 0 wherever g64 == 0.
d_ref measured (fft yardstick / matmul yardstick; they move a little with the host's FFT and BLAS): a 1.2e-6 / 7.7e-7, b 1.7e-6 / 1.8e-6,
d 3.6e-6 / 2.9e-6, e 2.9e-6 / 2.8e-6, f 1.2e-6 / 7.7e-7 on one host, a 1.5e-6 / 8.8e-7, b 2.3e-6 / 1.8e-6, d 3.7e-6 / 3.1e-6, e 2.8e-6 / 3.1e-6 on
another; the kernels' d, worst row: a 7.5e-7, b 7.2e-7, d 6.3e-7, e 1.3e-6, f 7.5e-7 (MI355X and emulator alike); kink margins a 1.2e-3, b 4.9e-3, d 5.6e-3, e 2.1e-4, f 1.4e-3; clipped shares a 3.4 %, b 2.5 %, d 0.5 %, e 0.3 %."""
import importlib

import numpy as np
import torch

import stoi_cases as C
import stoi_loss_ref as L
import stoi_ref as R
from conftest import PKG_NAME

CASES = C.CASES
KINK_MARGIN = 1e-4
CLIPPED_CASES = ("a", "b", "e")             # cases that must exercise the clip branch


def loss_mod():
    return importlib.import_module(PKG_NAME + ".loss")


def reference(name):
    return L.case_reference(*CASES[name])


def check_inputs(name):
    """Conditions, not measurements: frame energies away from the threshold (stoi_cases.check_inputs), every item away from the kink
    of the clip, the clip branch really taken where the case is there for it."""
    C.check_inputs(name)
    ref = reference(name)
    print(f"case {name}: kink margin {ref['kink']:.2e}, clipped share {ref['clipped']:.4f}, rows with segments {ref['scoring']}")
    assert ref["kink"] >= KINK_MARGIN
    if name in CLIPPED_CASES:
        assert ref["clipped"] > 0.0
    return ref


def make(engine, fs):
    crit = loss_mod().stoi_loss(sample_rate=fs)
    crit._engine_override = engine
    return crit


def run(engine, device, name, c=None, e=None, grad_loss=None):
    """(loss, grad) of one case: tensors on `device`."""
    fs = CASES[name][2]
    ref = reference(name)
    c = ref["c"].to(device) if c is None else c
    e = (ref["e"].to(device) if e is None else e).detach().requires_grad_(True)
    loss = make(engine, fs)(c, e)
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, device=device))
    return loss.detach(), e.grad


def check_case(name, engine, device, c=None, e=None):
    rows, T, fs, _ = CASES[name]
    ref = check_inputs(name)
    loss, g = run(engine, device, name, c, e)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == device.type
    assert g.shape == (rows, T) and g.dtype == torch.float32 and g.device.type == device.type
    gn = g.double().cpu().numpy()
    assert np.isfinite(gn).all()
    d_loss = abs(float(loss) - ref["loss"])
    metric = C.metrics().stoi(ref["c"].to(device) if c is None else c, ref["e"].to(device) if e is None else e, sample_rate=fs, engine=engine)
    d_metric = abs(float(loss) + float(metric.double().mean()))
    print(f"case {name}: loss {float(loss):.8f}  d {d_loss:.2e} (bar {R.bar(ref):.2e})  |loss + mean metric| {d_metric:.2e} (bar {2.0 ** -22:.2e})")
    for r in range(rows):
        if r in ref["scoring"]:
            top = np.abs(ref["g64"][r]).max()
            d = np.abs(gn[r] - ref["g64"][r]).max() / top
            print(f"case {name} row {r}: max|g64| {top:.3e}  d {d:.2e} (d_ref {ref['dg_ref']:.2e}: fft {ref['dg_fft']:.2e}, matmul {ref['dg_matmul']:.2e}; "
                  f"bar {4.0 * ref['dg_ref']:.2e})")
    assert d_loss <= R.bar(ref), (name, d_loss)
    assert d_metric <= 2.0 ** -22, (name, d_metric)
    for r in range(rows):
        if r in ref["scoring"]:
            top = np.abs(ref["g64"][r]).max()
            assert np.abs(gn[r] - ref["g64"][r]).max() <= 4.0 * ref["dg_ref"] * top, (name, r)
            if fs == R.FS:
                assert (gn[r][ref["g64"][r] == 0.0] == 0.0).all() and (ref["g64"][r] == 0.0).any(), (name, r)
        else:
            assert (gn[r] == 0.0).all() and ref["scores64"][r] == R.SHORT, (name, r)
    return loss, g
