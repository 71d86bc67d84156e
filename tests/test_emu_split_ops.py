"""Single-op parity of the fp16-split kernels (conv_h3d_kernel, wgrad_h3d_kernel, wgrad_h3_kernel) through the C ABI's
wunet_op_*_split entry points, on the CPU fiber emulator at small geometries that reach every tile shape: un-segmented tiles
(L >= 256), 2 .. 16 items per tile (L = 128 .. 16), split-K, channel counts that are not multiples of 8 / 16 / 32, and operands
whose magnitudes sit far from 1 (the device-derived power-of-two scales).  The cases are the table of tests/split_op_cases.py, which
tests/test_gpu_split_ops_ragged.py runs on the hardware as well; tests/test_gpu_parity.py runs the same entry points at all BASELINE
layer geometries there.  Oracle: F.conv1d semantics restated in C (oracle/wunet_oracle.c, f64 build).

test_layer_forward_on_ragged_nets: the per-layer forward check of tests/split_op_cases.py (raw conv output of every layer and the
network output against the float64 oracle, the fp16-split path forced on and the fp32 kernels, training and eval) on the emulator."""
import numpy as np
import pytest

import emu_lib
import split_op_cases as C


def rel_norm(a, r):
    return float(np.linalg.norm((a - r).ravel()) / max(np.linalg.norm(r.ravel()), 1e-30))


@pytest.mark.parametrize("B,Cin,Cout,L,K,xs,ws", C.CASES)
def test_split_ops_vs_oracle(B, Cin, Cout, L, K, xs, ws):
    case = (B, Cin, Cout, L, K, xs, ws)
    x, w, b, gz = C.operands(case)
    zr, dxr, dwr = C.reference(case)
    z = emu_lib.op_conv1d_split(x, w, b)
    assert rel_norm(z, zr) < 2e-6 and np.abs(z - zr).max() < 2e-6 * np.abs(zr).max()
    if Cin >= 16:
        dx = emu_lib.op_dgrad_split(gz, w, Cin)
        dw = emu_lib.op_wgrad_split(gz, x, K)
        assert rel_norm(dx, dxr) < 2e-6 and np.abs(dx - dxr).max() < 2e-6 * np.abs(dxr).max()
        assert rel_norm(dw, dwr) < 2e-6 and np.abs(dw - dwr).max() < 4e-6 * np.abs(dwr).max()


def test_split_ops_reject_shapes_the_kernels_do_not_cover():
    x = np.zeros((1, 16, 8), np.float32)
    w = np.zeros((16, 16, 5), np.float32)
    with pytest.raises(RuntimeError, match="L >= 16"):
        emu_lib.op_conv1d_split(x, w, None)
    x = np.zeros((2, 8, 256), np.float32)
    w = np.zeros((16, 8, 5), np.float32)
    with pytest.raises(RuntimeError, match="Cin >= 16"):
        emu_lib.op_dgrad_split(np.zeros((2, 16, 256), np.float32), w, 8)


@pytest.mark.parametrize("h3", [2, 0], ids=["split", "fp32"])
@pytest.mark.parametrize("net", C.NETS, ids=C.net_id)
def test_layer_forward_on_ragged_nets(net, h3):
    """Ragged channel groups on every layer with an odd batch, batch 1, and padded rows: every layer's raw conv output at
    2e-5 * max(1, max |z_ref|), the output at 1e-5, the operand's row padding exactly zero (C.check_layer_forward), training and eval.
    Measured here, worst layer (of its bar's scale) / output, training mode (eval mode is 2x closer), split and fp32:
    (3, 20, 3, 2048) 9.1e-7 / 1.6e-6 and 6.5e-7 / 1.1e-6; (2, 28, 1, 1024) 7.3e-7 / 1.1e-6 and 4.5e-7 / 8.0e-7;
    (3, 16, 2, 768) 9.1e-7 / 1.7e-6 and 5.0e-7 / 1.1e-6."""
    import importlib
    from conftest import PKG_NAME
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    eng = eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=h3)
    for training in (True, False):
        names = {}

        def run():
            names["err"] = C.check_layer_forward(eng, "cpu", net, training)
        ran = C.profiled(eng.lib, run)
        print(f"emu layer forward {C.net_id(net)} h3={h3} {'train' if training else 'eval'}: worst layer {names['err'][0]:.2e}, output {names['err'][1]:.2e}")
        n_split = sum(v for k, v in ran.items() if k.startswith("conv_h3"))
        assert n_split == (2 * net[0] if h3 else 0), ran          # (every layer but the first one-channel conv)
