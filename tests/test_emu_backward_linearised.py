"""CPU emulator: the whole backward pass - gradient assembly, BatchNorm backward, both gradient GEMMs, the head, the input gradient and
how they are chained - against the float64 arbiter linearised at the device's own forward point (tests/linearised_ref.py), at
margin x d_ref: 2 x (fp32 MFMA path) / 4 x (fp16-split path) the distance of the reference's own float32 ATen arithmetic at the same
point.  The plain-arbiter gradient tests (test_emu_network.py) have to allow 3e-4 .. 2e-2 of a tensor, because the forward's rounding
flips LeakyReLU slopes; here only the backward's rounding is left, ~1e-6, and one wrong element shows (the self-check below).

Measured on the emulator (profiles/backward_linearised.txt): d_ref 4.8e-7 .. 4.0e-6, the device's worst tensor at 0.25 .. 1.85 x d_ref
(fp32 path at most 1.85 x, bar 2 x; split path at most 1.76 x, bar 4 x), at most 2 ambiguous slopes in a case."""
import importlib

import pytest
import torch

import emu_lib
import linearised_ref as lr
from conftest import PKG_NAME

SWITCHES = ("WUNET_H3_NOSPLIT", "WUNET_NO_E0", "WUNET_REDUCE_SERIAL", "WUNET_NO_ENC_GZ", "WUNET_PA_SWAP", "WUNET_UPT")


def _run(monkeypatch, case):
    for k in SWITCHES:                           # (planner switches, read when a context is planned: only the case's own are set)
        monkeypatch.delenv(k, raising=False)
    for k, v in case[5].items():
        monkeypatch.setenv(k, v)
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    eng = eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=case[0])
    return lr.device_run(eng, torch.device("cpu"), case)


@pytest.mark.parametrize("case", lr.CASES, ids=lr.case_id)
def test_backward_matches_the_arbiter_at_the_devices_forward_point(monkeypatch, case):
    m = lr.check(case, _run(monkeypatch, case), "emulator")
    assert m["k"] <= 2, (m["k"], "the emulator run leaves room for the hardware's last bit: choose another seed or shape")


def test_one_flipped_slope_is_seen(monkeypatch):
    """The harness's own check: the arbiter with the slope of ONE non-ambiguous element (of 3 x 10 x 128 in the widest layer) chosen the
    other way lies more than 100 x the case's bar from the device's gradients - so would a kernel wrong at one position."""
    case = lr.CASES[0]
    dev = _run(monkeypatch, case)
    m = lr.measure(case, dev)
    _, layers = lr.linearised(case, dev["z"], torch.float64, m["masks"])
    y, _, thr = layers[0]
    j = int(torch.argmax((y.abs() > 1e3 * thr).flatten().to(torch.int8)))          # the first element far from the kink
    assert (0, j) not in lr.ambiguous_elements(layers) and abs(float(y.flatten()[j])) > 1e3 * float(thr.flatten()[j])
    wrong, _ = lr.linearised(case, dev["z"], torch.float64, lr.flipped(layers, [(0, j)]))
    got = dict(dev["grads"], input=dev["input"])
    far = max(lr.rel(got[t], wrong[t]) for t in lr.compared(case))
    bar = lr.MARGIN[case[0]] * m["d_ref"]
    print(f"one flipped slope: {far:.2e} = {far / bar:.0f} x the bar ({bar:.2e})")
    assert m["worst"][1] <= bar < far / 100.0, (m["worst"], bar, far)
