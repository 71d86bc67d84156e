"""-m gpu: the fp16-split kernels at RAGGED tile shapes on the MI355X - the single-op table of tests/split_op_cases.py (the cases
tests/test_emu_split_ops.py runs on the CPU emulator) through wunet_op_conv1d_split / _dgrad_split / _wgrad_split, and the per-layer
forward of ragged nets with the split path forced on and on the fp32 kernels.  tests/test_gpu_parity.py holds the same entry points to
the same bar at the BASELINE geometries, where every tile is full; here are the channel counts off the 8 / 16 / 32 grid, the odd
batches that leave the last tile partly empty, 2 .. 16 items under one tile and split K that starts inside a K tail - what the emulator
can only restate: the zero pads an LDS-DMA piece fetches beyond the last channel group or item, the lanes of a 16x16x32 MFMA whose K
quarter holds no channel, the store guards of a tile row outside the batch.

Reference: F.conv1d semantics in float64 (oracle/wunet_oracle.c).  The three ops are linear (no LeakyReLU kink), so the bar is the
1e-5 of test_split_ops_at_baseline_geometries, tensor-relative and relative to the tensor's largest entry, on every element (outputs
are pre-filled with NaN: an unwritten edge element fails the finite check).

Figures on the MI355X: NOT RECORDED YET - this module has not had a hardware run; every test prints its measured pair per case and op
and the kernel names it saw, to be written here from the first one.  What the same table gives on the CPU emulator (float64 oracle;
tensor-relative norm / largest difference over the largest |ref|), and the kernels the planner launches there (the plan does not
depend on the device):
  conv   1.7e-7 .. 2.9e-7 / <= 5.7e-7     dgrad  2.6e-7 .. 3.6e-7 / <= 8.8e-7     wgrad  2.8e-7 .. 3.4e-7 / <= 5.8e-7
  B1-24x40-L256-k15   conv_h3d_kernel<15, 3, 1> + <15, 2, 1>, wgrad_h3d_kernel<15, 2>     B2-20x24-L512-k5    conv_h3d_kernel<5, 2, 1> x 2, wgrad_h3d_kernel<5, 2>
  B3-48x24-L128-k5    conv_h3d_kernel<5, 2, 2> + <5, 3, 2>, wgrad_h3d_kernel<5, 2>        B5-16x56-L64-k15    conv_h3d_kernel<15, 2, 4> x 2, wgrad_h3_kernel<15, 2>
  B9-72x40-L32-k5     conv_h3d_kernel<5, 3, 8> x 2, wgrad_h3_kernel<5, 3>                 B17-40x72-L16-k15   conv_h3d_kernel<15, 3, 16> x 2, wgrad_h3_kernel<15, 2>
  B2-72x80-L512-k15   conv_h3d_kernel<15, 3, 1> x 2, wgrad_h3d_kernel<15, 3>              B3-104x24-L256-k5   conv_h3d_kernel<5, 2, 1> x 2, wgrad_h3d_kernel<5, 2>
  B16-16x16-L16-k5    conv_h3d_kernel<5, 2, 16> x 2, wgrad_h3_kernel<5, 2>                B33-24x24-L16-k5    conv_h3d_kernel<5, 2, 16> x 2, wgrad_h3_kernel<5, 2>
  B7-60x20-L64-k5     conv_h3d_kernel<5, 2, 4> x 2, wgrad_h3_kernel<5, 2>                 B5-100x60-L128-k15  conv_h3d_kernel<15, 2, 2> x 2, wgrad_h3d_kernel<15, 2>
  B1-20x24-L256-k15   conv_h3d_kernel<15, 2, 1> x 2, wgrad_h3d_kernel<15, 2>              B3-20x40-L1024-k5   conv_h3d_kernel<5, 3, 1> + <5, 2, 1>, wgrad_h3d_kernel<5, 3>
  B2-28x36-L2048-k15  conv_h3d_kernel<15, 3, 1> + <15, 2, 1>, wgrad_h3d_kernel<15, 3>
  K tail on / off differ in: conv and dgrad (72x80), conv only (104x24, 100x60), dgrad only (28x36: four whole groups forward)
  per-layer forward, worst layer / output, training mode: split 9.1e-7 / 1.7e-6, fp32 6.5e-7 / 1.1e-6 (eval mode: half of that)
"""
import importlib

import numpy as np
import pytest
import torch

import split_op_cases as C
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu
BAR = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def engine():
    return importlib.import_module(PKG_NAME + ".engine").default_engine()


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _check(what, got, ref):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), (what, int((~np.isfinite(got)).sum()))
    rel, err = C.errors(got, ref)
    print(f"{what}: rel {rel:.2e} max {err:.2e}")
    assert rel < BAR and err < BAR, (what, rel, err)
    return got


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_split_ops_at_ragged_geometries(engine, dev, case):
    """conv, data gradient and weight gradient of one case, every element, and the kernels that ran: a conv_h3*_kernel<K, launch
    (conv_h3d_kernel from 256 samples on), and ONE weight-gradient kernel - wgrad_h3d_kernel from 128 samples on, wgrad_h3_kernel
    below.  (The planner keeps that rule at every shape of the table: launch_wgrad_h3 takes the DMA-staged kernel when a 128-position
    chunk lies inside one item and plan_h3_wgrad's rows per wave fit its registers, which they do up to the table's 80 output
    channels.)  The data / weight gradient need Cin >= 16, which every case of the table has."""
    B, Cin, Cout, L, K, _, _ = case
    x, w, b, gz = (torch.tensor(a).to(dev) for a in C.operands(case))
    zr, dxr, dwr = C.reference(case)
    z, dx, dw = _nan((B, Cout, L), dev), _nan((B, Cin, L), dev), _nan((Cout, Cin, K), dev)
    lib = engine.lib

    def run():
        assert lib.wunet_op_conv1d_split(x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        assert lib.wunet_op_conv1d_dgrad_split(gz.data_ptr(), w.data_ptr(), dx.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        assert lib.wunet_op_conv1d_wgrad_split(gz.data_ptr(), x.data_ptr(), dw.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
    names = C.profiled(lib, run)
    torch.cuda.synchronize()
    print(f"{C.case_id(case)} kernels: {sorted(names)}")
    conv = [nm for nm in names if nm.startswith("conv_h3") and "_kernel<%d," % K in nm]
    assert conv and sum(names[nm] for nm in conv) == 2, names          # (forward conv + data gradient)
    if L >= 256:      # the un-segmented levels run the DMA-staged, pipelined kernel
        assert all(nm.startswith("conv_h3d_kernel<%d," % K) for nm in conv), names
    wg = [nm for nm in names if nm.startswith("wgrad_h3")]
    assert len(wg) == 1 and names[wg[0]] == 1 and wg[0].startswith(("wgrad_h3d_kernel<%d," if L >= 128 else "wgrad_h3_kernel<%d,") % K), names
    _check(C.case_id(case) + " conv", z, zr)
    _check(C.case_id(case) + " dgrad", dx, dxr)
    _check(C.case_id(case) + " wgrad", dw, dwr)


@pytest.mark.parametrize("case", C.KTAIL_CASES, ids=C.case_id)
def test_k_tail_at_ragged_geometries(engine, dev, monkeypatch, case):
    """The cases with left-over channel groups: conv_h3d_kernel's K tail (WUNET_H3_KTAIL=1, the default) and the zero-padded last
    chunk (= 0; read when the op plans its tiling) both meet the bar on every element, and are not the same numbers."""
    B, Cin, Cout, L, K, _, _ = case
    x, w, b, gz = (torch.tensor(a).to(dev) for a in C.operands(case))
    zr, dxr, _ = C.reference(case)
    lib = engine.lib
    got = {}
    for kt in ("0", "1"):
        monkeypatch.setenv("WUNET_H3_KTAIL", kt)
        z, dx = _nan((B, Cout, L), dev), _nan((B, Cin, L), dev)
        assert lib.wunet_op_conv1d_split(x.data_ptr(), w.data_ptr(), b.data_ptr(), z.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        assert lib.wunet_op_conv1d_dgrad_split(gz.data_ptr(), w.data_ptr(), dx.data_ptr(), B, Cin, Cout, L, K, None) == 0, lib.wunet_last_error()
        torch.cuda.synchronize()
        got[kt] = (_check(f"{C.case_id(case)} ktail={kt} conv", z, zr), _check(f"{C.case_id(case)} ktail={kt} dgrad", dx, dxr))
    assert not (np.array_equal(got["0"][0], got["1"][0]) and np.array_equal(got["0"][1], got["1"][1]))


@pytest.mark.parametrize("h3", [2, 0], ids=["split", "fp32"])
@pytest.mark.parametrize("net", C.NETS, ids=C.net_id)
def test_layer_forward_on_ragged_nets(dev, net, h3):
    """C.check_layer_forward on the hardware, training and eval: every layer's raw conv output at 2e-5 * max(1, max |z_ref|), the
    output at 1e-5, the operand's row padding exactly zero.  With the split path forced on, every conv but the first (one input
    channel: conv_first_kernel) must have run on a conv_h3*_kernel; with h3 = 0 none of them."""
    eng = importlib.import_module(PKG_NAME + ".engine").Engine(h3=h3)
    for training in (True, False):
        res = {}

        def run():
            res["err"] = C.check_layer_forward(eng, dev, net, training)
        ran = C.profiled(eng.lib, run)
        convs = {k: v for k, v in ran.items() if k.startswith("conv_")}
        print(f"layer forward {C.net_id(net)} h3={h3} {'train' if training else 'eval'}: worst layer {res['err'][0]:.2e}, output {res['err'][1]:.2e}, {convs}")
        n_split = sum(v for k, v in ran.items() if k.startswith("conv_h3"))
        assert n_split == (2 * net[0] if h3 else 0), ran
        if not h3:
            assert sum(v for k, v in ran.items() if k.startswith("conv_mfma_kernel<")) == 2 * net[0], ran
