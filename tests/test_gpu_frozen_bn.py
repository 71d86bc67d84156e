"""-m gpu: frozen BatchNorm on the MI355X at the BASELINE size (12 levels, batch 64 x 16384): backward through model.eval() and
through a training model with some BatchNorm modules in eval mode, against oracle/torch_port in float64 with each layer in its
own mode (tests/frozen_bn_ref.py); the eval forward under grad; a Trainer whose model keeps BatchNorm frozen."""
import importlib

import numpy as np
import pytest
import torch

import frozen_bn_ref as ref
from conftest import PKG_NAME
from oracle import plan

pytestmark = pytest.mark.gpu

N, CI, B, T = 12, 24, 64, 16384
TOL, REL_BAR = 1e-4, 1.0e-2        # test_full_size_properties' bars (absolute, tensor-relative)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


_ARB = {}


def _arbiter(name):
    """float64 arbiter of one mask at the full size, computed once per module."""
    if name not in _ARB:
        noisy, clean = plan.golden_batch(B, T, 5)
        mask = [True] * (2 * N + 1) if name == "eval" else ref.masks(N)[name]
        _ARB[name] = (noisy, clean, mask) + ref.run(plan.golden_state(N, CI, 0), noisy, clean, N, CI, "smooth_l1", mask)
    return _ARB[name]


def _gpu_step(pkg, dev, name, noisy, clean, mask, h3=None, loss="smooth_l1", sd=None):
    eng = importlib.import_module(PKG_NAME + ".engine").Engine(h3=h3)
    m = pkg.Model(n_layers=N, channels_interval=CI)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in (sd or plan.golden_state(N, CI, 0)).items()})
    m.to(dev)
    m._engine_override = eng
    if name == "eval":
        m.eval()
    else:
        m.train()
        ref.set_bn_modes(m, mask)
    crit = {"smooth_l1": pkg.smooth_l1_loss, "mse": pkg.mse_loss}[loss]()
    crit._engine_override = eng
    out = m(torch.from_numpy(noisy).to(dev))
    lv = crit(torch.from_numpy(clean).to(dev), out)
    lv.backward()
    torch.cuda.synchronize()
    return m, out.detach().cpu().numpy(), lv.item()


def _check_full(m, out, lv, arb):
    noisy, clean, mask, r_out, r_lv, r_grads, r_state = arb
    assert np.isfinite(out).all()
    oe = float(np.abs(out - r_out).max())
    assert oe < TOL, oe
    assert abs(lv - r_lv) < 1e-5
    worst = 0.0
    for k, p in m.named_parameters():
        g, r = p.grad.cpu().numpy().astype(np.float64), r_grads[k]
        err = float(np.abs(g - r).max())
        rel = float(np.linalg.norm((g - r).ravel()) / (np.linalg.norm(r.ravel()) + 1e-12))
        worst = max(worst, rel)
        if k.endswith(".0.bias") and not k.startswith("out") and np.abs(r).max() < 1e-9:
            assert np.all(g == 0.0), k                 # a batch-statistics layer's conv bias: exact zero
            continue
        # (the absolute bar as test_odd_shapes_vs_oracle's: 1e-4 or 2e-3 of the tensor's largest entry - frozen layers pass on
        #  activations the batch does not normalise, and a mixed mask's gradients are larger than the batch-statistics net's)
        assert err < max(TOL, 2e-3 * np.abs(r).max()) and rel < REL_BAR, (k, err, rel, np.abs(r).max())
    post = m.state_dict()
    sd = plan.golden_state(N, CI, 0)
    for (prefix, _, _, _), f in zip(plan.conv_layers(N, CI), mask):
        for b in ("running_mean", "running_var", "num_batches_tracked"):
            k = f"{prefix}.1.{b}"
            got = post[k].cpu().numpy()
            if f:
                assert np.array_equal(got, sd[k]), k
            else:
                assert np.abs(got.astype(np.float64) - r_state[k]).max() < 1e-4 * max(1.0, np.abs(r_state[k]).max()), k
    print(f"frozen BatchNorm: output {oe:.2e}, worst tensor-relative gradient distance {worst:.2e}")


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("h3", [None, 0], ids=["default", "fp32"])
def test_eval_backward_vs_arbiter(pkg, dev, h3):
    """model.eval() + smooth-L1 backward: every gradient (the conv biases' included - they no longer cancel) against float64."""
    arb = _arbiter("eval")
    m, out, lv = _gpu_step(pkg, dev, "eval", arb[0], arb[1], arb[2], h3=h3)
    _check_full(m, out, lv, arb)


@pytest.mark.timeout(1200)
@pytest.mark.parametrize("h3", [None, 0], ids=["default", "fp32"])
def test_mixed_mask_vs_arbiter(pkg, dev, h3):
    """Training model, encoder BatchNorm frozen, middle and decoder on batch statistics: output, gradients, and running
    statistics (untouched on the frozen layers, updated on the others)."""
    arb = _arbiter("enc")
    m, out, lv = _gpu_step(pkg, dev, "enc", arb[0], arb[1], arb[2], h3=h3)
    _check_full(m, out, lv, arb)


def _errs(out, grads, ref_out, ref_grads):
    oe = float(np.abs(out - ref_out).max())
    num = den = 0.0
    for k, g in grads.items():
        num += float(np.sum((g.astype(np.float64) - ref_grads[k]) ** 2))
        den += float(np.sum(ref_grads[k].astype(np.float64) ** 2))
    return oe, (num / max(den, 1e-300)) ** 0.5


@pytest.mark.timeout(1200)
def test_eval_backward_bf16_mode(pkg, dev):
    """The bf16 mode (wunet_set_h3(ctx, 3)) through model.eval(): against the reference's fp32 run with every BatchNorm frozen,
    no further off than the reference's own forward under torch.autocast(bfloat16) - test_bf16_mode_vs_reference_under_autocast's
    bar.  (Batch 8: the autocast CPU run at batch 64 would dominate the suite.)"""
    b = 8
    noisy, clean = plan.golden_batch(b, T, 7)
    sd = plan.golden_state(N, CI, 0)
    mask = [True] * (2 * N + 1)
    r_out, _, r_grads, _ = ref.run(sd, noisy, clean, N, CI, "mse", mask, dtype=torch.float32)
    a_out, _, a_grads, _ = ref.run(sd, noisy, clean, N, CI, "mse", mask, dtype=torch.float32, bf16_autocast=True)
    m, out, _ = _gpu_step(pkg, dev, "eval", noisy, clean, mask, h3=3, loss="mse", sd=sd)
    grads = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    oe, ga = _errs(out, grads, r_out, r_grads)
    oe_ref, ga_ref = _errs(a_out, a_grads, r_out, r_grads)
    print(f"bf16 eval backward: out err {oe:.2e} (autocast reference {oe_ref:.2e}), gradient error {ga:.2e} ({ga_ref:.2e})")
    assert np.isfinite(out).all()
    assert oe <= oe_ref and ga <= ga_ref, (oe, ga, oe_ref, ga_ref)


def test_eval_forward_under_grad_is_the_eval_forward(pkg, dev):
    """enhancement.py's grad-enabled eval forward: the same path as under no_grad - bit-identical, no backward workspace held."""
    m = pkg.Model(n_layers=N, channels_interval=CI)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(N, CI, 0).items()})
    m.to(dev).eval()
    noisy = torch.from_numpy(plan.golden_batch(B, T, 5)[0]).to(dev)
    with torch.no_grad():
        a = m(noisy)
    b = m(noisy)
    torch.cuda.synchronize()
    assert b.requires_grad and torch.equal(a, b)
    assert getattr(b.grad_fn, "ws", None) is None


@pytest.mark.timeout(900)
def test_trainer_with_frozen_bn_graph_equals_eager_and_recaptures(pkg, dev, tmp_path):
    """A Model subclass whose train() keeps chosen BatchNorm modules frozen, driven by trainer.Trainer's captured step graph:
    bit for bit the written-out eager loop; flipping one layer's mode mid-run makes the trainer capture a new graph."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    n, ci, b, sl = N, CI, 8, T

    class FrozenModel(pkg.Model):
        frozen_layers = frozenset(range(n))

        def train(self, mode=True):
            super().train(mode)
            for i, (_, bn) in enumerate(self._leaves()):
                if i in self.frozen_layers:
                    bn.eval()
            return self

    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(10):
        clean = torch.rand(b, 1, sl, generator=g) * 2 - 1
        batches.append(((clean + 0.1 * torch.randn(b, 1, sl, generator=g)).to(dev), clean.to(dev)))
    flip_at = 6

    def make():
        m = FrozenModel(n_layers=n, channels_interval=ci)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(n, ci, 0).items()})
        m = m.to(dev).train()
        return m, pkg.smooth_l1_loss(), optim_mod.FusedAdam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))

    cfg = {"root_dir": str(tmp_path), "experiment_name": "f", "trainer": {"epochs": 1, "save_checkpoint_interval": 0, "graph": True}}
    m1, crit1, opt1 = make()
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, [], None)
    assert tr.use_graph
    graph_before = None
    for k, (mix, cl) in enumerate(batches):
        if k == flip_at:
            graph_before = tr._graph
            assert graph_before is not None
            m1.frozen_layers = frozenset(range(n - 1))       # encoder.(n-1) back on batch statistics
            m1.train()
        tr._step(mix, cl)
    assert tr._graph is not None and tr._graph is not graph_before        # captured again under the new modes
    m2, crit2, opt2 = make()
    for k, (mix, cl) in enumerate(batches):
        if k == flip_at:
            m2.frozen_layers = frozenset(range(n - 1))
            m2.train()
        opt2.zero_grad()
        crit2(cl, m2(mix)).backward()
        opt2.step()
    torch.cuda.synchronize()
    for (k, a), (_, c) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, c), k
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        s1, s2 = opt1.state[p1], opt2.state[p2]
        assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])
