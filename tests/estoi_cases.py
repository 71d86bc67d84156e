"""What the ESTOI tests run and check, shared by tests/test_estoi_emu.py, tests/test_estoi_loss_emu.py (CPU emulator) and
tests/test_gpu_estoi.py (MI355X): the six cases of tests/stoi_cases.py, unchanged, through metrics.stoi(extended=True) and
loss.stoi_loss(extended=True), against tests/estoi_ref.py.  `engine` None = the product's default engine.
Conditions on the inputs, asserted before any comparison: stoi_cases.check_inputs (frame energies at least 0.05 dB from the threshold) and
every centred row norm and column norm of the float64 path strictly positive (ESTOI has no kink; a zero norm is where its derivative is
undefined).  Bars, d_ref measured on the CPU at test time and printed beside every d:
  score     |score - oracle64| <= 4 d_ref + 2^-23 per row; frame counts exactly; short rows exactly float32(1e-5);
  loss      the score bar against -mean oracle64, and |loss + mean metrics.stoi(extended=True)| <= 2^-22;
  gradient  per scoring row max_t |g - g64| <= 4 d_ref max_t |g64|; short rows exactly 0; at 10 kHz g == 0 wherever g64 == 0.
Measured on one host (CPU emulator): float64 scores a 0.27077 / 0.00580, b 0.28195 / 0.00163 / 0.00585, d 0.33527 / 0.03111, e 0.17305 /
0.06422; score d_ref 1.3e-7 .. 4.5e-7 and the kernels' d 3.3e-8 .. 2.2e-7; gradient d_ref 7.3e-6 .. 9.3e-6 of a row's largest entry (0.036
.. 0.144) and the kernels' d 1.4e-6 .. 6.8e-6; least row norms 0.069 .. 0.16, least column norms 0.016 .. 0.082."""
import importlib

import numpy as np
import torch

import estoi_ref as E
import stoi_cases as C
import stoi_ref as R
from conftest import PKG_NAME

CASES = C.CASES


def loss_mod():
    return importlib.import_module(PKG_NAME + ".loss")


def check_inputs(name):
    C.check_inputs(name)
    ref = E.case_reference(*CASES[name])
    print(f"case {name}: float64 ESTOI {ref['score']}, frames {ref['frames']}; least centred row norm {ref['row_norm']:.3e}, column norm "
          f"{ref['col_norm']:.3e}")
    assert ref["row_norm"] > 0.0 and ref["col_norm"] > 0.0
    if name in ("c", "f"):
        assert ref["score"][-1] == R.SHORT and ref["frames"][-1] < R.SEG
    return ref


def run(engine, device, name, c=None, e=None):
    fs = CASES[name][2]
    ref = E.case_reference(*CASES[name])
    c = ref["c"].to(device) if c is None else c
    e = ref["e"].to(device) if e is None else e
    return C.metrics().stoi(c, e, sample_rate=fs, return_frames=True, engine=engine, extended=True)


def check_case(name, engine, device, c=None, e=None):
    """Scores and frame counts of one case against the float64 oracle.  c / e: the case's inputs at another address.  Returns
    (scores, frames)."""
    rows = CASES[name][0]
    ref = check_inputs(name)
    bar = E.bar(ref)
    score, frames = run(engine, device, name, c, e)
    assert score.shape == (rows,) and score.dtype == torch.float32 and score.device.type == device.type
    assert frames.shape == (rows,) and frames.dtype == torch.int32 and frames.device.type == device.type
    d = np.abs(score.double().cpu().numpy() - ref["score"])
    print(f"case {name}: scores {score.cpu().numpy()}  d {d.max():.2e} (d_ref {ref['d_ref']:.2e}: restate32 {ref['d_restate']:.2e}, "
          f"fft32 {ref['d_fft']:.2e}; bar {bar:.2e})  frames {frames.cpu().numpy()}")
    assert list(frames.cpu().numpy()) == list(ref["frames"]), (name, frames, ref["frames"])
    assert (d <= bar).all(), (name, d, bar)
    short = ref["frames"] < R.SEG
    assert (score.cpu().numpy()[short] == np.float32(R.SHORT)).all()
    return score, frames


def make_loss(engine, fs):
    crit = loss_mod().stoi_loss(sample_rate=fs, extended=True)
    crit._engine_override = engine
    return crit


def run_loss(engine, device, name, c=None, e=None, grad_loss=None):
    """(loss, grad) of one case: tensors on `device`."""
    fs = CASES[name][2]
    ref = E.case_reference(*CASES[name])
    c = ref["c"].to(device) if c is None else c
    e = (ref["e"].to(device) if e is None else e).detach().requires_grad_(True)
    loss = make_loss(engine, fs)(c, e)
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, device=device))
    return loss.detach(), e.grad


def check_loss_case(name, engine, device, c=None, e=None):
    rows, T, fs, _ = CASES[name]
    check_inputs(name)
    ref = E.loss_reference(*CASES[name])
    loss, g = run_loss(engine, device, name, c, e)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.device.type == device.type
    assert g.shape == (rows, T) and g.dtype == torch.float32 and g.device.type == device.type
    gn = g.double().cpu().numpy()
    assert np.isfinite(gn).all()
    d_loss = abs(float(loss) - ref["loss"])
    metric = C.metrics().stoi(ref["c"].to(device) if c is None else c, ref["e"].to(device) if e is None else e, sample_rate=fs, engine=engine,
                              extended=True)
    d_metric = abs(float(loss) + float(metric.double().mean()))
    print(f"case {name}: loss {float(loss):.8f}  d {d_loss:.2e} (bar {E.bar(ref):.2e})  |loss + mean metric| {d_metric:.2e} (bar {2.0 ** -22:.2e})")
    for r in ref["scoring"]:
        top = np.abs(ref["g64"][r]).max()
        d = np.abs(gn[r] - ref["g64"][r]).max() / top
        print(f"case {name} row {r}: max|g64| {top:.3e}  d {d:.2e} (d_ref {ref['dg_ref']:.2e}: fft {ref['dg_fft']:.2e}, matmul {ref['dg_matmul']:.2e}; "
              f"bar {4.0 * ref['dg_ref']:.2e})")
    assert d_loss <= E.bar(ref), (name, d_loss)
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


def offset_views(name, device):
    """The case's inputs as views one float into their buffers: 4-byte alignment only."""
    rows, T = CASES[name][:2]
    ref = E.case_reference(*CASES[name])
    views = []
    for x in (ref["c"], ref["e"]):
        buf = torch.zeros(rows * T + 8, device=device)
        buf[1:1 + rows * T] = x.reshape(-1).to(device)
        views.append(buf[1:1 + rows * T].view(rows, T))
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    return views
