"""-m gpu: the gradient with respect to the waveform input (Model(..., input_grad=True); include/wunet_hip.h: wunet_backward_input)
on the MI355X.  Arbiter: oracle/torch_port in float64 with torch.autograd.grad w.r.t. the input; the bar is test_gemm_paths_match_reference's
form - at most twice the reference's own float32 CPU distance to the arbiter (tensor-relative) + 1e-3."""
import importlib

import numpy as np
import pytest
import torch

import frozen_bn_ref as ref
from conftest import PKG_NAME
from oracle import plan
from test_input_grad_emu import arbiter, profiled, upstream

pytestmark = pytest.mark.gpu


def _dist(a, b):
    return float(np.linalg.norm((np.asarray(a, np.float64) - b).ravel()) / max(np.linalg.norm(np.asarray(b).ravel()), 1e-30))


def _model(n, ci, sd, dev, eng=None):
    m = importlib.import_module(PKG_NAME + ".model").Model(n_layers=n, channels_interval=ci, input_grad=True)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    if eng is not None:
        m._engine_override = eng
    return m.to(dev)


def _gpu_step(m, noisy, gout, dev, mask=None, eval_frozen=False):
    if eval_frozen:
        m.eval()
        for p in m.parameters():
            p.requires_grad_(False)
    else:
        m.train()
        if mask is not None:
            ref.set_bn_modes(m, mask)
    x = torch.from_numpy(noisy).to(dev).requires_grad_(True)
    out = m(x)
    out.backward(torch.from_numpy(gout).to(dev))
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), x.grad.cpu().numpy()


def _check_against_arbiter(gx, sd, noisy, gout, n, ci, mask, training=True):
    _, r64, _ = arbiter(sd, noisy, gout, n, ci, mask, training=training)
    _, r32, _ = arbiter(sd, noisy, gout, n, ci, mask, training=training, dtype=torch.float32)
    d, d_ref = _dist(gx, r64), _dist(r32, r64)
    assert np.isfinite(gx).all()
    assert d <= 2.0 * d_ref + 1e-3, (d, d_ref)
    return d, d_ref


def test_full_size_input_gradient_matches_float64():
    """n=12, ci=24, B=64, T=16384 on the split GEMM path (the default engine): the E0 first layer, g rebuilt by the kernel."""
    dev = torch.device("cuda:0")
    n, ci, B, T = 12, 24, 64, 16384
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    m = _model(n, ci, sd, dev)
    _, gx = _gpu_step(m, noisy, gout, dev)
    eng = m._engine()
    (_, gx_p), names = profiled(eng, lambda: _gpu_step(_model(n, ci, sd, dev), noisy, gout, dev))
    assert names.get("input_grad_kernel<ENC>", 0) == 1 and names.get("pass_a_kernel<ENC, e0>", 0) == 1, names
    assert np.array_equal(gx, gx_p)                 # (the profiler serialises the streams: the same bits)
    _check_against_arbiter(gx, sd, noisy, gout, n, ci, [False] * (2 * n + 1))


def test_padded_length_with_a_frozen_mask():
    dev = torch.device("cuda:0")
    n, ci, B, T = 12, 24, 8, 12288                  # 3 * 2^12: rows of 16384 inside the workspace
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 1)
    gout = upstream(noisy.shape)
    mask = ref.masks(n)["alt"]
    _, gx = _gpu_step(_model(n, ci, sd, dev), noisy, gout, dev, mask=mask)
    assert gx.shape == (B, 1, T)
    _check_against_arbiter(gx, sd, noisy, gout, n, ci, mask)


def test_eval_model_with_frozen_weights():
    dev = torch.device("cuda:0")
    n, ci, B, T = 12, 24, 8, 16384
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 2)
    gout = upstream(noisy.shape)
    m = _model(n, ci, sd, dev)
    _, gx = _gpu_step(m, noisy, gout, dev, eval_frozen=True)
    assert all(p.grad is None for p in m.parameters())
    for k, v in m.state_dict().items():
        assert np.array_equal(v.cpu().numpy(), sd[k]), k
    _check_against_arbiter(gx, sd, noisy, gout, n, ci, [True] * (2 * n + 1), training=False)


def test_bf16_mode_input_gradient():
    """bf16 GEMM mode (wunet_set_h3(ctx, 3)) at tests/test_bf16_mode.py's bar: no further from the float64 arbiter than the reference
    under CPU bf16 autocast (x 1.1 for the spread of the CPU's bf16 kernels)."""
    dev = torch.device("cuda:0")
    eng = importlib.import_module(PKG_NAME + ".engine").Engine(h3=3)
    n, ci, B, T = 12, 24, 4, 16384
    sd = plan.golden_state(n, ci, 0)
    noisy, _ = plan.golden_batch(B, T, 0)
    gout = upstream(noisy.shape)
    _, gx = _gpu_step(_model(n, ci, sd, dev, eng), noisy, gout, dev)
    mask = [False] * (2 * n + 1)
    _, r64, _ = arbiter(sd, noisy, gout, n, ci, mask)
    _, rbf, _ = arbiter(sd, noisy, gout, n, ci, mask, dtype=torch.float32, bf16=True)
    e, e_ref = _dist(gx, r64), _dist(rbf, r64)
    assert np.isfinite(gx).all() and e <= 1.1 * e_ref, (e, e_ref)


def test_same_bits_nothing_else_moves_and_graph_replay():
    """B=64, T=16384: requesting the input gradient leaves output, loss, every parameter gradient and the buffers bit-identical; two
    runs give the same input-gradient bits; a captured forward + backward + input gradient replays to the eager bits."""
    dev = torch.device("cuda:0")
    pkg = importlib.import_module(PKG_NAME)
    n, ci, B, T = 12, 24, 64, 16384
    sd = plan.golden_state(n, ci, 0)
    noisy, clean = plan.golden_batch(B, T, 0)
    y = torch.from_numpy(clean).to(dev)

    def step(want_x):
        m = _model(n, ci, sd, dev).train()
        x = torch.from_numpy(noisy).to(dev).requires_grad_(want_x)
        out = m(x)
        lv = pkg.smooth_l1_loss()(y, out)
        lv.backward()
        torch.cuda.synchronize()
        return (out.detach().cpu(), lv.item(), [p.grad.cpu() for p in m.parameters()], {k: v.cpu() for k, v in m.state_dict().items()},
                x.grad.cpu() if want_x else None)

    a, b, c = step(False), step(True), step(True)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2]))
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3])
    assert torch.equal(b[4], c[4])

    m = _model(n, ci, sd, dev).train()
    x = torch.from_numpy(noisy).to(dev).requires_grad_(True)
    g = torch.from_numpy(upstream(noisy.shape)).to(dev)

    def fb():
        x.grad = None
        m.zero_grad(set_to_none=True)
        m(x).backward(g)

    for _ in range(3):
        fb()
    torch.cuda.synchronize()
    eager_x, eager_p = x.grad.clone(), [p.grad.clone() for p in m.parameters()]
    graph = torch.cuda.CUDAGraph()
    x.grad = None
    m.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        m(x).backward(g)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(x.grad, eager_x)
    assert all(torch.equal(p.grad, q) for p, q in zip(m.parameters(), eager_p))
