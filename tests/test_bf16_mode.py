"""BASELINE.json configs[4] ("deep variant, bf16"): the bf16 mode of the GEMM path (wunet_set_h3(ctx, 3 | 4): conv inputs, g_z and
weights stored as ONE bf16 word per value, one pass of v_mfma_f32_16x16x32_bf16, fp32 accumulation; raw conv outputs,
BatchNorm, gradient assembly and the optimiser stay fp32).

Parity bar.  The reference has no bf16 code of its own: "the reference in bf16" is its model under torch.autocast(bfloat16) on the
CPU (conv1d runs in bf16 and every activation is then STORED in bf16).  Measured against the f64 oracle that run is 1.8e-2 off on
the output and 14-17 % (relative norm) on the worst gradient tensor; this mode keeps activations in fp32 between layers and is
closer to the exact result on both.  The tests state exactly that: error vs the f64 oracle <= the autocast reference's error vs
the same oracle, and the difference to the autocast run itself stays inside the sum of the two.

That bar judges the mode, not its kernels: it has to allow the bf16 noise itself.  The bf16 instantiations of the GEMM kernels are held
to fp32-accumulation accuracy one op and one layer at a time, against the float64 conv of the bf16-rounded operands, in
tests/test_emu_bf16_ops.py (emulator) and tests/test_gpu_bf16_ops.py (MI355X); tests/bf16_ref.py says why that comparison is exact."""
import importlib

import numpy as np
import pytest
import torch

import emu_lib
from conftest import PKG_NAME
from oracle import c_oracle, plan, torch_port
from test_scale_robustness import errors, run_step


def _engine(h3):
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=h3)


def autocast_reference(sd, noisy, clean, n, ci, loss="mse"):
    """The reference's arithmetic for a bf16 run: its forward (ATen ops, oracle/torch_port.py) under CPU autocast."""
    tsd = torch_port.state_to_torch(sd, requires_grad=True)
    with torch.autocast("cpu", dtype=torch.bfloat16):
        out = torch_port.forward(tsd, torch.from_numpy(noisy), n, ci, True)
        lv = torch_port.loss_value(loss, torch.from_numpy(clean), out)
    lv.backward()
    return out.detach().float().numpy(), {k: v.grad.numpy() for k, v in tsd.items() if v.requires_grad}


@pytest.mark.parametrize("net", [(3, 16, 3, 1024), (4, 16, 5, 1024), (2, 24, 2, 1024),
                                 (3, 16, 2, 768)],           # 768 = 3 * 2^8 samples: rows padded to 1024 / 512 / 256 / 128
                         ids=lambda c: "n%dci%dB%dT%d" % c)
def test_bf16_mode_is_at_least_as_accurate_as_the_reference_under_autocast(net):
    n, ci, B, T = net
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)
    ref = c_oracle.step({k: v.copy() for k, v in sd.items()}, noisy, clean, n, ci, True, "mse", precision="f64")
    ao, ag = autocast_reference(sd, noisy, clean, n, ci)
    oe_ref, ge_ref = errors(ao, ag, ref)
    out, grads = run_step(_engine(4), sd, n, ci, noisy, clean)
    oe, ge = errors(out, grads, ref)
    assert np.isfinite(out).all()
    # (the autocast run's own error depends on which bf16 conv oneDNN picks for the host CPU - AMX, avx512_bf16 or the converted
    #  fp32 kernels: 0.160 - 0.17 on the worst gradient tensor across the hosts this suite has run on, against a deterministic
    #  0.162 here for the padded length.  Both are the same bf16 rounding noise; the bar allows that spread)
    assert oe <= oe_ref and ge <= 1.1 * ge_ref, (oe, ge, oe_ref, ge_ref)
    assert oe > 1e-4                       # (it really is the bf16 arithmetic: the fp16-split path sits at 2e-6)
    od, gd = errors(out, grads, {"out": ao, "grads": ag})
    assert od <= oe + oe_ref and gd <= 1.5 * (ge + ge_ref), (od, gd)


def test_bf16_mode_eval_forward():
    n, ci, B, T = 3, 16, 3, 1024
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)
    ref = c_oracle.step({k: v.copy() for k, v in sd.items()}, noisy, clean, n, ci, False, "mse", precision="f64")
    out, _ = run_step(_engine(4), sd, n, ci, noisy, clean, train=False)
    tsd = torch_port.state_to_torch(sd)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        ao = torch_port.forward(tsd, torch.from_numpy(noisy), n, ci, False).float().numpy()
    e, e_ref = np.abs(out - ref["out"]).max(), np.abs(ao - ref["out"]).max()
    assert e <= e_ref and e < 5e-3, (e, e_ref)
