"""-m gpu: the row losses (scale-invariant SDR / SNR per utterance: loss_rows_partial_kernel / loss_rows_final_kernel /
loss_rows_bwd_kernel behind wunet_loss_rows_forward / _backward), metrics.si_sdr and the Trainer's opt-in validation on the MI355X.
The op cases are those of tests/test_loss_rows_emu.py on device tensors (tests/loss_rows_cases.py) against the same float64 yardstick
(tests/si_sdr_ref.py) with the same bars: values 2^-22 * max(|ref|, 1), gradient 1e-5 of each row's largest element.  The network
test compares parameter gradients with oracle/torch_port in float64 under the float64 loss, at the tolerance of the small-net fixture
tests of tests/test_gpu_parity.py (test_golden_small_cases).  The Trainer tests' yardstick is the written-out eager loop.

Measured on the MI355X (worst over both kinds and zero_mean on / off; bar in brackets):
  shapes (1,1) ... (100,8200), (64,16384): values 5.7e-8 [2.4e-7], gradient 5.9e-8 [1e-5]
  input-SNR ladder -10 ... 60 dB, T 4096:  values 4.9e-8 [2.4e-7], gradient 5.1e-8 [1e-5]
  4-byte-aligned bases:                    values 2.9e-8, gradient 4.7e-8
  degenerate rows (T 64):                  0 dB exactly / -98.31 dB / +96.77 dB; the e = s row's gradient 5.4e-7 [1e-5]
  small net through si_sdr_loss:           output 1.4e-6 [1e-4]; loss 5.873946, 4.9e-7 dB from the float64 one [1.0e-2, derived in the
                                           test from the output's bar]; worst parameter gradient decoder.3.main.0.weight 1.6e-6 =
                                           0.02 of its bar
(a row of one sample, whose gradient is exactly 0, came out at -1.2e-8 while the backward added a separately rounded centring
term D to A e; it applies A (e - mean) since)
"""
import importlib

import numpy as np
import pytest
import torch

import loss_rows_cases as C
import si_sdr_ref as R
from conftest import PKG_NAME
from oracle import plan, torch_port

pytestmark = pytest.mark.gpu

TOL = 1e-4                     # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES + ((64, 16384),), ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_and_gradient_on_device_tensors(dev, shape, kind):
    """Every shape of the emulator test and the workload's own (64 x 16384: one 8 MB pass), zero_mean on and off."""
    s, e = R.pair(*shape)
    for zero_mean in (True, False):
        C.check_case(f"{kind} {shape} zero_mean={zero_mean}", None, dev, kind, zero_mean, s, e)


@pytest.mark.parametrize("kind", C.KINDS)
def test_ladder_alignment_degenerate_rows_and_scaling(dev, kind):
    """The rest of the emulator's op cases on the device: the input-SNR ladder (gradient bar up to 60 dB), bases with 4-byte
    alignment only (inputs; inputs and gradient through the C entry; inputs that disagree modulo 16), the degenerate rows,
    grad_loss = 0.25 exact, a second backward, two runs bit-identical, metrics == the loss's rows."""
    engine = importlib.import_module(PKG_NAME + ".engine").default_engine()
    s, e = R.ladder(4096)
    upto60 = [k for k, db in enumerate(R.LADDER_DB) if db <= 60.0]
    for zero_mean in (True, False):
        C.check_case(f"ladder {kind} zero_mean={zero_mean}", None, dev, kind, zero_mean, s, e, grad_rows=upto60)
    # alignment
    Rr, T = 3, 1031
    s, e, sv, ev = C.unaligned(Rr, T, dev)
    assert sv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and sv.is_contiguous()
    _, _, _, _, g = C.check_case(f"unaligned {kind}", None, dev, kind, True, sv, ev)
    _, coefs, _ = engine.loss_rows_forward(kind, sv, ev)
    gbuf = torch.full((Rr * T + 8,), float("nan"), device=dev)
    one = torch.ones((), device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    assert engine.lib.wunet_loss_rows_backward(3 if kind == "si_sdr" else 4, sv.data_ptr(), ev.data_ptr(), coefs.data_ptr(), one.data_ptr(), Rr, T, gbuf[1:].data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(gbuf[1:1 + Rr * T].view(Rr, 1, T), g)
    assert torch.isnan(gbuf[0]) and torch.isnan(gbuf[1 + Rr * T:]).all()
    loss2, g2 = C.run(None, dev, kind, True, sv, e)
    rl, _, rg = R.reference(kind, s, e, True)
    R.check_values(f"mixed alignment {kind}", loss2, None, rl, None)
    R.check_grad(f"mixed alignment {kind}", g2, rg)
    # degenerate rows
    C.check_degenerate(None, dev, kind)
    # scaling, a second backward, determinism, metrics
    s, e = R.pair(5, 4099)
    l1, g1 = C.run(None, dev, kind, True, s, e)
    _, gq = C.run(None, dev, kind, True, s, e, grad_loss=0.25)
    assert torch.equal(gq, 0.25 * g1)
    crit = getattr(C.mods()[0], kind + "_loss")()
    x = e.to(dev).requires_grad_(True)
    loss = crit(s.to(dev), x)
    loss.backward(retain_graph=True)
    loss.backward()
    assert torch.equal(x.grad, 2.0 * g1)
    s, e = R.pair(1, 200003)
    la, ga = C.run(None, dev, kind, True, s, e)
    lb, gb = C.run(None, dev, kind, True, s, e)
    assert torch.equal(la, lb) and torch.equal(ga, gb)
    rows = C.rows_db(None, dev, kind, True, s, e)
    _, coefs, rows2 = engine.loss_rows_forward(kind, s.to(dev), e.to(dev), per_row=True)
    assert rows.is_cuda and torch.equal(rows, rows2) and torch.equal(rows, coefs[:, 3].float())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(s, e)


def _make(pkg, dev, n, ci, crit):
    m = pkg.Model(n_layers=n, channels_interval=ci)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(n, ci, 0).items()})
    return m.to(dev), crit()


def test_small_net_gradients_through_si_sdr_loss(pkg, dev):
    """n_layers 4, channels_interval 8, B 4, T 1024 on the golden state, trained through si_sdr_loss: output, loss and every
    parameter gradient against oracle/torch_port in float64 with the float64 loss (tests/si_sdr_ref.per_row), at the tolerance of
    test_gpu_parity.test_golden_small_cases: 1e-4 absolute and 5e-4 of the tensor's largest element (+ 1e-7); conv biases in front
    of a batch-statistics BatchNorm get an exact 0."""
    n, ci, B, T = 4, 8, 4, 1024
    noisy, clean = plan.golden_batch(B, T, 0)
    m, crit = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    m.train()
    out = m(torch.from_numpy(noisy).to(dev))
    lv = crit(torch.from_numpy(clean).to(dev), out)
    lv.backward()
    torch.cuda.synchronize()
    t64 = torch_port.state_to_torch(plan.golden_state(n, ci, 0), dtype=torch.float64, requires_grad=True)
    o64 = torch_port.forward(t64, torch.from_numpy(noisy).double(), n, ci, True)
    l64 = -R.per_row("si_sdr", torch.from_numpy(clean).double(), o64).mean()
    l64.backward()
    eo = (out.detach().cpu().double() - o64.detach()).abs().max().item()
    el = abs(lv.item() - l64.item())
    print(f"small net si_sdr: out {eo:.2e}  loss {lv.item():.6f} vs {l64.item():.6f} ({el:.2e})")
    # the loss is in dB: to first order |d v| <= (10 / ln 10) * 2 |d e| (1 / rms(e - alpha s) + 1 / rms(alpha s)) for an output
    # error |d e| on every sample, all aligned with the residual; |d e| = the output's own bar (1e-4), plus the value bar of the loss
    with torch.no_grad():
        sc = torch.from_numpy(clean).double().reshape(B, T)
        sc = sc - sc.mean(dim=1, keepdim=True)
        ec = o64.reshape(B, T) - o64.reshape(B, T).mean(dim=1, keepdim=True)
        al = (ec * sc).sum(dim=1, keepdim=True) / (sc * sc).sum(dim=1, keepdim=True)
        rms_t = (al * sc).pow(2).mean(dim=1).sqrt().min().item()
        rms_n = (ec - al * sc).pow(2).mean(dim=1).sqrt().min().item()
    loss_bar = R.K10 * 2.0 * TOL * (1.0 / rms_n + 1.0 / rms_t) + R.VALUE_BAR * max(1.0, abs(l64.item()))
    print(f"small net si_sdr: loss bar {loss_bar:.2e} (rms of the target part {rms_t:.2e}, of the residual {rms_n:.2e})")
    assert eo < TOL and el <= loss_bar
    worst = (0.0, 0.0, "")
    for k, p in m.named_parameters():
        ref = t64[k].grad.numpy()
        got = p.grad.cpu().numpy()
        err = np.abs(got - ref).max()
        if k.endswith(".0.bias") and not k.startswith("out"):
            assert np.all(got == 0.0) and np.abs(ref).max() < 1e-6, k
            continue
        bar = min(TOL, 5e-4 * max(np.abs(ref).max(), 1e-6) + 1e-7)
        worst = max(worst, (err / bar, err, k))
        print(f"  {k}: err {err:.2e}  max|ref| {np.abs(ref).max():.2e}  ({err / bar:.2f} of the bar)")
    print(f"small net si_sdr: worst gradient {worst[2]} err {worst[1]:.2e} = {worst[0]:.2f} of its bar")
    for k, p in m.named_parameters():
        if k.endswith(".0.bias") and not k.startswith("out"):
            continue
        ref = t64[k].grad.numpy()
        err = np.abs(p.grad.cpu().numpy() - ref).max()
        assert err < TOL and err < 5e-4 * max(np.abs(ref).max(), 1e-6) + 1e-7, (k, err)


def _same_state(m1, opt1, m2, opt2, steps):
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        s1, s2 = opt1.state[p1], opt2.state[p2]
        assert int(s1["step"]) == int(s2["step"]) == steps
        assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])


def test_trainer_captures_the_si_sdr_step_once(pkg, dev, tmp_path):
    """Trainer with si_sdr_loss and FusedAdam, 12 steps: the step graph (forward + row loss + backward + Adam) is captured once and
    parameters, buffers and moments equal the written-out eager loop bit for bit."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    n, ci, sl = 4, 8, 1024
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=48, sample_length=sl, seed=3), batch_size=4, shuffle=False)
    cfg = {"root_dir": str(tmp_path), "experiment_name": "r", "trainer": {"epochs": 1, "save_checkpoint_interval": 0}}
    m1, crit1 = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    opt1 = optim_mod.FusedAdam(m1.parameters(), lr=1e-3, betas=(0.9, 0.999))
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, None)
    assert tr.use_graph and tr.captures == 0 and tr.validation_interval == 0
    tr.train()
    torch.cuda.synchronize()
    assert tr.use_graph and tr.captures == 1 and tr._graph is not None and tr.validation_scores == []
    m2, crit2 = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    opt2 = optim_mod.FusedAdam(m2.parameters(), lr=1e-3, betas=(0.9, 0.999))
    m2.train()
    tot = 0.0
    for mix, cl, _ in loader:
        opt2.zero_grad()
        loss = crit2(cl.to(dev), m2(mix.to(dev)))
        loss.backward()
        opt2.step()
        tot += loss.item()
    torch.cuda.synchronize()
    _same_state(m1, opt1, m2, opt2, 12)
    assert np.allclose(tr.epoch_losses, [tot / 12], rtol=1e-5, atol=1e-5)


def test_validation_scores_the_si_sdr_improvement_and_keeps_the_graph(pkg, dev, tmp_path):
    """"validation": {"metric": "si_sdr", "interval": 1} over 2 epochs of 6 steps, recordings of 3 * 1024 + 17 samples at batch 1:
    validation_scores equals metrics.si_sdr_improvement computed by hand on inference.enhance's output of the written-out loop's
    model after each epoch; the graph captured in epoch 1 - before the first validation - is replayed through epoch 2 (captures == 1)
    and the final state still equals the eager loop's bit for bit; best_model.tar exists, reloads, and a resumed Trainer has its
    best_score."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    inference = importlib.import_module(PKG_NAME + ".inference")
    metrics = importlib.import_module(PKG_NAME + ".metrics")
    n, ci, sl = 4, 8, 1024
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=24, sample_length=sl, seed=3), batch_size=4, shuffle=False)
    vloader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=3, sample_length=3 * sl + 17, seed=11, mode="validation"),
                                          batch_size=1, shuffle=False)
    cfg = {"root_dir": str(tmp_path), "experiment_name": "v",
           "trainer": {"epochs": 2, "save_checkpoint_interval": 0,
                       "validation": {"metric": "si_sdr", "interval": 1, "find_max": True, "custom": {"sample_length": sl}}}}
    m1, crit1 = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    opt1 = optim_mod.FusedAdam(m1.parameters(), lr=1e-3, betas=(0.9, 0.999))
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, vloader)
    assert tr.use_graph and tr.validation_interval == 1 and tr.validation_sample_length == sl
    tr.train()
    torch.cuda.synchronize()
    assert tr.captures == 1 and tr._graph is not None and m1.training
    # the written-out loop with the by-hand score after each epoch
    m2, crit2 = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    opt2 = optim_mod.FusedAdam(m2.parameters(), lr=1e-3, betas=(0.9, 0.999))
    scores = []
    for _ in range(2):
        m2.train()
        for mix, cl, _ in loader:
            opt2.zero_grad()
            crit2(cl.to(dev), m2(mix.to(dev))).backward()
            opt2.step()
        m2.eval()
        gains = []
        for mix, cl, _ in vloader:
            mix, cl = mix.to(dev), cl.to(dev)
            assert mix.shape == (1, 1, 3 * sl + 17)
            gains.append(metrics.si_sdr_improvement(cl, mix, inference.enhance(m2, mix, sl)))
        scores.append(torch.cat(gains).double().mean().item())
    m2.train()
    torch.cuda.synchronize()
    print(f"validation scores {tr.validation_scores} by hand {scores}")
    assert tr.validation_scores == scores and all(np.isfinite(scores))
    _same_state(m1, opt1, m2, opt2, 12)
    assert tr.best_score == max(scores)
    best = tr.checkpoints_dir / "best_model.tar"
    assert best.exists()
    ck = torch.load(best.as_posix(), map_location="cpu")
    assert set(ck) == {"epoch", "best_score", "optimizer", "model"} and ck["best_score"] == max(scores)
    assert ck["epoch"] == (2 if scores[1] >= scores[0] else 1)          # (base_trainer.py:152: a tie is a new best)
    m3 = pkg.Model(n_layers=n, channels_interval=ci)
    m3.load_state_dict(ck["model"])
    if ck["epoch"] == 2:
        for (k, a), (_, b) in zip(m3.state_dict().items(), m2.state_dict().items()):
            assert torch.equal(a, b.cpu()), k
    m4, crit4 = _make(pkg, dev, n, ci, pkg.si_sdr_loss)
    opt4 = optim_mod.FusedAdam(m4.parameters(), lr=1e-3, betas=(0.9, 0.999))
    tr4 = trainer_mod.Trainer(cfg, True, m4, crit4, opt4, loader, vloader)       # resumes from latest_model.tar, written with the best one
    assert tr4.best_score == tr.best_score and tr4.start_epoch == ck["epoch"] + 1
