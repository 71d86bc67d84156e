"""The backward's two elementwise A/B switches (WUNET_NO_ENC_GZ, WUNET_PA_SWAP; planner switches, read when a context is planned) change
which kernel forms an encoder layer's g and how pass A's grid is laid out - never a bit of any result.  Shared by the emulator test
(tests/test_emu_network.py) and the hardware test (tests/test_gpu_parity.py): the shapes, the switch settings, one training step."""
import ctypes
import importlib

import numpy as np
import torch

from conftest import PKG_NAME
from oracle import plan

# (n, ci, B, T), the environment both runs share
SHAPES = {
    # the encoder levels above the middle neither fused nor split: GZ_ENC recompute runs (or g is stored and read back), one piece per channel
    "n3_unsplit": ((3, 24, 3, 2048), {"WUNET_H3_NOSPLIT": "1"}),
    # the top level in three pieces per channel (the swapped grid runs), split-K data gradients (pass A adds the partials itself)
    "n4_split": ((4, 16, 3, 4096), {}),
}
SWITCHES = {"no_enc_gz": ("WUNET_NO_ENC_GZ", "1"), "pa_swap_off": ("WUNET_PA_SWAP", "0")}


def train_step(make_engine, dev, shape):
    """One mse training step at h3 = 2 on a fresh engine (its contexts are planned under the environment of the moment): every result as
    numpy arrays, and what the profiler saw: {kernel name: algorithmic bytes} (the emulator build reports 0 bytes)."""
    n, ci, B, T = shape
    pkg = importlib.import_module(PKG_NAME)
    eng = make_engine()
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)
    m = pkg.Model(n_layers=n, channels_interval=ci, input_grad=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m.to(dev).train()
    crit = pkg.mse_loss()
    m._engine_override = crit._engine_override = eng
    eng.lib.wunet_profile_enable(1)
    try:
        x = torch.from_numpy(noisy).to(dev).requires_grad_(True)
        out = m(x)
        loss = crit(torch.from_numpy(clean).to(dev), out)
        loss.backward()
        if dev.type == "cuda":
            torch.cuda.synchronize()
    finally:
        buf = ctypes.create_string_buffer(1 << 16)
        eng.lib.wunet_profile_collect(buf, len(buf))
        eng.lib.wunet_profile_enable(0)
    res = {"out": out.detach().cpu().numpy(), "loss": loss.detach().cpu().numpy(), "grad_input": x.grad.cpu().numpy()}
    for k, p in m.named_parameters():
        res["grad " + k] = p.grad.cpu().numpy()
    return res, {ln.split("\t")[0]: float(ln.split("\t")[4]) for ln in buf.value.decode().strip().splitlines()}


def assert_same_step(base, other, what):
    (a, names_a), (b, names_b) = base, other
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)
    assert names_a.keys() == names_b.keys(), (what, names_a.keys() ^ names_b.keys())
