"""CPU emulator tests of the gradient with respect to the waveform input (Model(..., input_grad=True); include/wunet_hip.h:
wunet_backward_input).  The arbiter is oracle/torch_port.forward in float64 with torch.autograd.grad w.r.t. the input, each layer's
BatchNorm in its own mode (tests/frozen_bn_ref.py).  Every form in which the first layer's backward leaves its g_z is reached - the
fused single-block pass, the E0 pass that stores nothing, the stored g of WUNET_NO_E0=1 - and asserted through the profiler."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import emu_lib
import frozen_bn_ref as ref
from conftest import PKG_NAME
from oracle import plan, torch_port


def _engine(h3=None):
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True, h3=h3)


def _model(n, ci, eng, sd, **kw):
    m = importlib.import_module(PKG_NAME + ".model").Model(n_layers=n, channels_interval=ci, **kw)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    m._engine_override = eng
    return m


def upstream(shape, seed=3):
    """A random grad_output (not only a loss's)."""
    return np.random.Generator(np.random.PCG64(seed)).standard_normal(size=shape).astype(np.float32)


def arbiter(sd, noisy, gout, n, ci, mask, training=True, dtype=torch.float64, bf16=False):
    """(out, dL/dx, {param: dL/dparam}) of oracle/torch_port.forward for the upstream gradient gout; mask: frozen layers."""
    s = torch_port.state_to_torch(sd, dtype=dtype, requires_grad=True)
    x = torch.as_tensor(np.asarray(noisy), dtype=dtype).requires_grad_(True)
    names = [k for k, v in s.items() if v.requires_grad]
    with ref.frozen_layers([p for p, f in zip(ref.prefixes(n, ci), mask) if f]), \
            torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        out = torch_port.forward(s, x, n, ci, training=training)
    g = torch.autograd.grad(out, [x] + [s[k] for k in names], grad_outputs=torch.as_tensor(gout).to(out.dtype))
    f = (lambda t: t.detach().float().numpy()) if bf16 else (lambda t: t.detach().numpy())
    return f(out), f(g[0]), {k: f(v) for k, v in zip(names, g[1:])}


def profiled(eng, fn):
    """fn() with the per-launch profiler on: (fn's result, {kernel name: launches})."""
    eng.lib.wunet_profile_enable(1)
    try:
        res = fn()
        buf = ctypes.create_string_buffer(1 << 16)
        eng.lib.wunet_profile_collect(buf, len(buf))
    finally:
        eng.lib.wunet_profile_enable(0)
    return res, {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().strip().splitlines()}


def model_step(eng, sd, noisy, gout, n, ci, mask=None, eval_frozen=False):
    """Model(input_grad=True) forward + backward(gout) with an input that requires grad: (model, out, dL/dx)."""
    m = _model(n, ci, eng, sd, input_grad=True)
    if eval_frozen:
        m.eval()
        for p in m.parameters():
            p.requires_grad_(False)
    else:
        m.train()
        if mask is not None:
            ref.set_bn_modes(m, mask)
    x = torch.from_numpy(noisy.copy()).requires_grad_(True)
    out = m(x)
    out.backward(torch.from_numpy(gout))
    return m, out.detach().numpy(), x.grad.numpy()


def close(got, want, rel=3e-4):
    """The bar of the neighbouring gradient tests (test_train_step_matches_oracle, test_frozen_bn_emu._check)."""
    scale = max(np.abs(want).max(), 1e-6)
    return np.abs(got - want).max() < rel * scale + 1e-6, (np.abs(got - want).max(), scale)


# (n, ci, B, T, engine h3, environment, the kernel mode expected): the fused single-block pass of a small level (g_z stored by pass A);
# the E0 geometries of test_first_layer_weight_gradient_from_the_gradient_assembly_sums (padded rows of 768 / 1536 included) - nothing
# stored, g rebuilt from the consumers' data gradients - and the same with WUNET_NO_E0=1: g stored, k1..k3 applied by the kernel
E0_GEOMS = [(2, 24, 2, 1024), (3, 24, 3, 2048), (2, 16, 5, 512), (2, 24, 2, 768), (3, 24, 1, 1536)]
PATHS = ([("fuse", 2, 4, 2, 64, None, {}, "GZ")]
         + [("e0", *g, 2, {"WUNET_H3_NOSPLIT": "1"}, "ENC") for g in E0_GEOMS]
         + [("no_e0", *g, 2, {"WUNET_H3_NOSPLIT": "1", "WUNET_NO_E0": "1"}, "G") for g in E0_GEOMS])


@pytest.mark.parametrize("name,n,ci,B,T,h3,env,mode", PATHS, ids=lambda v: v if isinstance(v, str) else None)
def test_input_gradient_on_every_first_layer_path(monkeypatch, name, n, ci, B, T, h3, env, mode):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if "WUNET_NO_E0" not in env:
        monkeypatch.delenv("WUNET_NO_E0", raising=False)
    eng = _engine(h3)
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    nl = 2 * n + 1
    (m, out, gx), names = profiled(eng, lambda: model_step(eng, sd, noisy, gout, n, ci))
    r_out, r_gx, r_grads = arbiter(sd, noisy, gout, n, ci, [False] * nl)
    assert names.get(f"input_grad_kernel<{mode}>", 0) == 1, names
    assert sum(v for k, v in names.items() if k.startswith("input_grad_kernel")) == 1, names
    if mode == "ENC":
        assert names.get("pass_a_kernel<ENC, e0>", 0) == 1, names
    else:
        assert "pass_a_kernel<ENC, e0>" not in names, names
    assert np.abs(out - r_out).max() < 2e-5
    ok, info = close(gx, r_gx)
    assert ok, info
    k = "encoder.0.main.0.weight"                    # (the gradient the first layer's pass produces beside it)
    ok, info = close(dict(m.named_parameters())[k].grad.numpy(), r_grads[k])
    assert ok, (k, info)


@pytest.mark.parametrize("n,ci,B,T,h3,nosplit", [(2, 4, 2, 64, None, False), (2, 24, 2, 768, 2, True), (3, 8, 2, 96, None, False)])
def test_requesting_the_input_gradient_moves_nothing_else(monkeypatch, n, ci, B, T, h3, nosplit):
    """Output, loss, every parameter gradient, running statistics and num_batches_tracked: bit-identical with and without it."""
    if nosplit:
        monkeypatch.setenv("WUNET_H3_NOSPLIT", "1")
    eng = _engine(h3)
    pkg_loss = importlib.import_module(PKG_NAME + ".loss")
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)

    def step(want_x):
        m = _model(n, ci, eng, sd, input_grad=True).train()
        crit = pkg_loss.mse_loss()
        crit._engine_override = eng
        x = torch.from_numpy(noisy.copy()).requires_grad_(want_x)
        out = m(x)
        lv = crit(torch.from_numpy(clean), out)
        lv.backward()
        assert (x.grad is not None) == want_x
        return (out.detach().numpy(), lv.item(), [p.grad.numpy().copy() for p in m.parameters()],
                {k: v.numpy().copy() for k, v in m.state_dict().items()})

    a, b = step(False), step(True)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    assert all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))
    assert all(np.array_equal(a[3][k], b[3][k]) for k in a[3])


# (2, 16, 5, 512): the E0 path under both masks.  (Some other E0 geometries put a frozen layer's pre-activation within rounding of the
#  LeakyReLU kink: its slope then follows the order of the sums and the weight gradient of encoder.0 moves by as much as the input's.)
@pytest.mark.parametrize("n,ci,B,T,h3,nosplit", [(3, 8, 2, 96, None, False), (2, 16, 5, 512, 2, True), (3, 16, 3, 768, 2, False)])
def test_input_gradient_with_a_mixed_frozen_mask(monkeypatch, n, ci, B, T, h3, nosplit):
    if nosplit:
        monkeypatch.setenv("WUNET_H3_NOSPLIT", "1")
    eng = _engine(h3)
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    for name in ("alt", "enc"):
        mask = ref.masks(n)[name]
        m, out, gx = model_step(eng, sd, noisy, gout, n, ci, mask=mask)
        r_out, r_gx, r_grads = arbiter(sd, noisy, gout, n, ci, mask)
        assert np.abs(out - r_out).max() < 2e-5
        ok, info = close(gx, r_gx)
        assert ok, (name, info)
        for k, p in m.named_parameters():
            ok, info = close(p.grad.numpy(), r_grads[k])
            assert ok, (name, k, info)


@pytest.mark.parametrize("n,ci,B,T,h3,nosplit", [(3, 8, 2, 96, None, False), (2, 24, 2, 768, 2, True)])
def test_input_gradient_of_an_eval_model_with_frozen_weights(monkeypatch, n, ci, B, T, h3, nosplit):
    """Robustness / saliency on a trained model: model.eval(), every parameter requires_grad_(False), the input requires grad - the
    eval forward, then the re-forward of _WaveUNetFn.backward on the running statistics.  The buffers stay untouched."""
    if nosplit:
        monkeypatch.setenv("WUNET_H3_NOSPLIT", "1")
    eng = _engine(h3)
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    m, out, gx = model_step(eng, sd, noisy, gout, n, ci, eval_frozen=True)
    r_out, r_gx, _ = arbiter(sd, noisy, gout, n, ci, [True] * (2 * n + 1), training=False)
    assert np.abs(out - r_out).max() < 2e-5
    ok, info = close(gx, r_gx)
    assert ok, info
    assert all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert np.array_equal(v.numpy(), sd[k]), k


def test_cascade_trains_the_first_stage():
    """m2(m1(x)), both training: m1's parameter gradients need m2's input gradient; against the float64 composition."""
    n, ci, B, T = 2, 8, 2, 256
    eng = _engine()
    sd1, sd2 = plan.golden_state(n, ci, 0), plan.golden_state(n, ci, 1)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    m1 = _model(n, ci, eng, sd1).train()
    m2 = _model(n, ci, eng, sd2).train()
    m2.input_grad = True                              # (the attribute is settable after construction)
    y = m2(m1(torch.from_numpy(noisy.copy())))
    y.backward(torch.from_numpy(gout))
    s1 = torch_port.state_to_torch(sd1, dtype=torch.float64, requires_grad=True)
    s2 = torch_port.state_to_torch(sd2, dtype=torch.float64, requires_grad=True)
    yr = torch_port.forward(s2, torch_port.forward(s1, torch.from_numpy(noisy).double(), n, ci, True), n, ci, True)
    yr.backward(torch.from_numpy(gout).double())
    assert np.abs(y.detach().numpy() - yr.detach().numpy()).max() < 2e-5
    for (k, p), (k2, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        for got, want, tag in ((p, s1[k], "m1"), (p2, s2[k2], "m2")):
            if k.endswith(".0.bias") and not k.startswith("out"):
                assert np.all(got.grad.numpy() == 0.0), (tag, k)          # exact zero in front of batch-statistics BatchNorm
                continue
            ok, info = close(got.grad.numpy(), want.grad.numpy())
            assert ok, (tag, k, info)


def test_default_model_still_refuses_and_names_the_switch():
    eng = _engine()
    n, ci = 2, 4
    m = _model(n, ci, eng, plan.golden_state(n, ci, 0)).train()
    assert m.input_grad is False
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(NotImplementedError, match=r"waveform input.*input_grad=True"):
        m(torch.zeros(2, 1, 64).requires_grad_(True))
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())       # refused before the forward touched the buffers
    # switched on, an input that does not require grad returns no input gradient (and needs none)
    m.input_grad = True
    x = torch.zeros(2, 1, 64)
    m(x).sum().backward()
    assert x.grad is None


def test_the_new_symbol_is_exported_and_bound():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    assert "wunet_backward_input" in lib_mod.EXPORTS
    assert hasattr(emu_lib.lib(), "wunet_backward_input")
    eng = _engine()
    assert eng.lib.wunet_backward_input.argtypes is not None
    assert eng.lib.wunet_backward_input(None, None, None, None, None, None) == -1                    # null arguments: an error code
