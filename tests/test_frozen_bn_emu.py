"""CPU emulator tests of frozen BatchNorm (include/wunet_hip.h: wunet_set_bn_frozen): a layer whose nn.BatchNorm1d module is in
eval mode normalises with its running statistics, leaves them untouched and back-propagates, inside a training forward (mixed
masks) and through model.eval() (every layer frozen: the eval forward, then a backward).  The arbiter is oracle/torch_port in
float64 with autograd, each layer in its own mode (tests/frozen_bn_ref.py).  fp32 kernels (emu_engine) and the fp16-split
kernels forced onto every level they can run (emu_engine_h3)."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import emu_lib
import frozen_bn_ref as ref
from conftest import PKG_NAME
from oracle import plan, torch_port


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.fixture(scope="module")
def emu_engine_h3():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=2)


def _model(n, ci, eng, sd):
    pkg_model = importlib.import_module(PKG_NAME + ".model")
    m = pkg_model.Model(n_layers=n, channels_interval=ci)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m._engine_override = eng
    return m


def _step(m, eng, noisy, clean, loss):
    pkg_loss = importlib.import_module(PKG_NAME + ".loss")
    crit = {"mse": pkg_loss.mse_loss, "l1": pkg_loss.l1_loss, "smooth_l1": pkg_loss.smooth_l1_loss}[loss]()
    crit._engine_override = eng
    out = m(torch.from_numpy(noisy))
    lv = crit(torch.from_numpy(clean), out)
    lv.backward()
    return out.detach().numpy(), lv.item()


def _check(m, sd, n, ci, out, r_out, r_grads, r_state, mask, gtol=3e-4):
    assert np.all(np.isfinite(out))
    assert np.abs(out - r_out).max() < 2e-5
    for k, p in m.named_parameters():
        g, r = p.grad.numpy(), r_grads[k]
        scale = max(np.abs(r).max(), 1e-6)
        assert np.abs(g - r).max() < gtol * scale + 1e-6, (k, np.abs(g - r).max(), scale)
    post = m.state_dict()
    for (prefix, _, _, _), f in zip(plan.conv_layers(n, ci), mask):
        for b in ("running_mean", "running_var", "num_batches_tracked"):
            k = f"{prefix}.1.{b}"
            if f:
                assert np.array_equal(post[k].numpy(), sd[k]), k          # frozen: bit-unchanged
            else:
                # (1e-5 as test_train_step_matches_oracle's, relative once the statistics exceed 1: a stale frozen layer feeds
                #  activations of ~1000x its normalised scale into the next ones)
                r = r_state[k].astype(np.float64)
                assert np.abs(post[k].numpy().astype(np.float64) - r).max() < 1e-5 * max(1.0, np.abs(r).max()), k


# the geometries of test_train_step_matches_oracle: padded lengths (96, 80), levels of 1 - 2 samples, a 1024-sample level
GEOMS = [(2, 4, 2, 32, "mse"), (3, 8, 3, 64, "l1"), (2, 24, 1, 1024, "smooth_l1"), (4, 4, 2, 16, "mse"),
         (3, 8, 2, 16, "smooth_l1"), (3, 8, 2, 96, "mse"), (4, 6, 2, 80, "smooth_l1")]
# the split kernels: every level on them, split-K at a 128-sample level (odd batch), padded rows of 768 / 384 / 192 / 96
GEOMS_H3 = [(2, 24, 1, 1024, "smooth_l1"), (3, 16, 3, 1024, "mse"), (3, 16, 3, 768, "mse")]


def test_arbiter_wrapper_matches_the_port():
    """The per-layer wrapper is the unpatched port when every layer is trained and when every layer is frozen."""
    n, ci = 3, 8
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(2, 64, 0)
    for training in (True, False):
        mask = [not training] * (2 * n + 1)
        out_w, lv_w, g_w, st_w = ref.run(sd, noisy, clean, n, ci, "mse", mask)
        s = torch_port.state_to_torch(sd, dtype=torch.float64, requires_grad=True)
        o = torch_port.forward(s, torch.from_numpy(noisy).double(), n, ci, training=training)
        lv = torch_port.loss_value("mse", torch.from_numpy(clean).double(), o)
        lv.backward()
        assert np.array_equal(o.detach().numpy(), out_w) and lv.item() == lv_w
        for k, v in s.items():
            if v.requires_grad:
                assert np.array_equal(v.grad.numpy(), g_w[k]), k
            assert np.array_equal(v.detach().numpy(), st_w[k]), k


def _run_mask(eng, n, ci, B, T, loss, name, gtol=3e-4, sd=None):
    sd = plan.golden_state(n, ci, 0) if sd is None else sd
    noisy, clean = plan.golden_batch(B, T, 0)
    m = _model(n, ci, eng, sd)
    if name == "eval":
        mask = [True] * (2 * n + 1)
        m.eval()
    else:
        mask = ref.masks(n)[name]
        m.train()
        ref.set_bn_modes(m, mask)
    r_out, r_lv, r_grads, r_state = ref.run(sd, noisy, clean, n, ci, loss, mask)
    out, lv = _step(m, eng, noisy, clean, loss)
    assert abs(lv - r_lv) < 1e-5
    _check(m, sd, n, ci, out, r_out, r_grads, r_state, mask, gtol)


@pytest.mark.parametrize("name", ["eval", "enc", "alt"])
@pytest.mark.parametrize("n,ci,B,T,loss", GEOMS)
def test_frozen_bn_matches_arbiter(emu_engine, n, ci, B, T, loss, name):
    _run_mask(emu_engine, n, ci, B, T, loss, name)


@pytest.mark.parametrize("name", ["eval", "enc", "alt"])
@pytest.mark.parametrize("n,ci,B,T,loss", GEOMS_H3)
def test_frozen_bn_split_matches_arbiter(emu_engine_h3, n, ci, B, T, loss, name):
    _run_mask(emu_engine_h3, n, ci, B, T, loss, name)


@pytest.mark.parametrize("eng_name", ["emu_engine", "emu_engine_h3"])
def test_frozen_bn_stale_running_statistics(request, eng_name):
    """running_var x 1e-6 on a frozen encoder layer: its activations are ~1000x what batch normalisation would give, beyond the
    data-independent bound |gamma| sqrt(N) + |beta| the training forward derives split-operand scales from.  The frozen layer's
    consumers must take their scale from the measured maximum: finite, and within the bar on the split path."""
    eng = request.getfixturevalue(eng_name)
    n, ci, B, T = 2, 24, 1, 1024
    sd = plan.golden_state(n, ci, 0)
    sd["encoder.1.main.1.running_var"] = (sd["encoder.1.main.1.running_var"] * np.float32(1e-6)).astype(np.float32)
    _run_mask(eng, n, ci, B, T, "smooth_l1", "enc", sd=sd)


def test_no_frozen_mask_is_bit_identical(emu_engine_h3):
    """A mask without a frozen layer - set through the C ABI, or left behind by a masked step on the shared context - runs
    exactly what an unmasked context runs."""
    eng = emu_engine_h3
    n, ci, B, T = 3, 16, 3, 1024
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)

    def plain_step():
        m = _model(n, ci, eng, sd)
        m.train()
        out, _ = _step(m, eng, noisy, clean, "mse")
        return out, [p.grad.numpy().copy() for p in m.parameters()], {k: v.numpy().copy() for k, v in m.state_dict().items()}

    base = plain_step()
    # a masked step on the same context, then an unmasked one: the engine clears the mask
    m = _model(n, ci, eng, sd)
    m.train()
    ref.set_bn_modes(m, ref.masks(n)["alt"])
    _step(m, eng, noisy, clean, "mse")
    for got in (plain_step(),):
        assert np.array_equal(got[0], base[0])
        assert all(np.array_equal(a, b) for a, b in zip(got[1], base[1]))
        assert all(np.array_equal(got[2][k], base[2][k]) for k in base[2])
    # an all-zero mask through the C ABI (the engine believes the context unmasked and leaves it)
    nl = 2 * n + 1
    hold = eng._using(n, ci, B, T, torch.device("cpu"))
    with hold as h:
        assert hold.ent[2] is None
        zeros = (ctypes.c_ubyte * nl)()
        assert eng.lib.wunet_set_bn_frozen(h, zeros, nl) == 0
        assert eng.lib.wunet_set_bn_frozen(h, zeros, nl - 1) != 0          # one byte per conv layer
        assert eng.lib.wunet_set_bn_frozen(h, zeros, nl) == 0
    got = plain_step()
    assert np.array_equal(got[0], base[0])
    assert all(np.array_equal(a, b) for a, b in zip(got[1], base[1]))
    assert all(np.array_equal(got[2][k], base[2][k]) for k in base[2])


def test_eval_forward_under_grad_is_the_eval_forward(emu_engine):
    """model.eval(): the forward under grad is the eval forward (bit-identical to no_grad) and holds no backward workspace."""
    n, ci, B, T = 3, 8, 2, 96
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    m = _model(n, ci, emu_engine, sd)
    m.eval()
    with torch.no_grad():
        a = m(torch.from_numpy(noisy))
    b = m(torch.from_numpy(noisy))
    assert b.requires_grad
    assert np.array_equal(a.numpy(), b.detach().numpy())
    assert getattr(b.grad_fn, "ws", None) is None
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k
