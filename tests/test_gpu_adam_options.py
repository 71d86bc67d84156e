"""-m gpu: the options of the fused Adam step on the MI355X - gradient clipping by the global norm, decoupled weight decay
(FusedAdamW) and the lr read from device memory (wunet_adam_step_ex: grad_sqnorm_partial_kernel, then adam_hyper_kernel and
adam_kernel with the optional slots of the hyper buffer - the kernels of wunet_adam_step).  No reference counterpart (train.py:31-35 builds a plain Adam, trainer/trainer.py:34-38 does not clip): the
yardstick of the op tests is the float64 restatement of clip_grad_norm_ + Adam / AdamW of tests/adam_options_ref.py with the bars
of the emulator tests (tests/test_adam_options_emu.py), the yardstick of the Trainer test is the written-out eager loop.
"""
import importlib
import warnings

import pytest
import torch

import adam_options_ref as R
from conftest import PKG_NAME
from oracle import plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def optim_mod():
    return importlib.import_module(PKG_NAME + ".optim")


def _equal(a, b):
    return all(torch.equal(x, y) for k in range(3) for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("case", ["mixed", "many"])
def test_clipped_step_on_device_tensors(optim_mod, dev, case):
    """The emulator op tests on device tensors, same shapes and bars: FusedAdam and FusedAdamW with max_grad_norm=5 against the float64
    restatement; a norm that never clips and a device-side lr have the bits of the plain step / the host lr; grad_scale with clipping
    is clipping of pre-scaled gradients; two runs are bit-identical; p.grad is not modified (checked inside run_fused)."""
    run = lambda **kw: R.run_fused(optim_mod, case, device=dev, **kw)[0]         # noqa: E731
    clipped = {}
    for decoupled in (False, True):
        clipped[decoupled] = run(decoupled=decoupled)
        R.check_against_reference(f"{case} {'AdamW' if decoupled else 'Adam'}", clipped[decoupled], case, decoupled)
        assert _equal(clipped[decoupled], run(decoupled=decoupled, device_lr=True, device_step=True))
    for device_step in (False, True):
        assert _equal(run(max_grad_norm=None, device_step=device_step), run(max_grad_norm=1e30, device_step=device_step)), device_step
    again = run(decoupled=True)
    assert _equal(clipped[True], again) and clipped[True][3] == again[3]
    scaled, prescaled = run(grad_scale=0.25), run(prescale=0.25)
    R.check_against_reference(f"{case} grad_scale", scaled, case, False, grad_scale=0.25)
    R.check_against_reference(f"{case} prescaled", prescaled, case, False, grad_scale=0.25)
    assert scaled[3] == prescaled[3]


def test_each_entry_point_stays_inside_its_hyper_buffer(pkg, dev):
    """tests/test_adam_options_emu.py's test of the same name on the device: wunet_adam_step writes slots 0 and 1 of its hyper buffer
    and nothing behind them, takes a NULL buffer without a device counter, and wunet_adam_step_ex with everything off writes the
    neutral clip, norm and decay and nothing behind slot 4."""
    eng = importlib.import_module(PKG_NAME + ".engine").default_engine()
    with torch.cuda.device(dev):
        R.check_hyper_buffer_bounds(eng.lib, dev, eng._stream(dev))


def _make(pkg, dev, n, ci):
    m = pkg.Model(n_layers=n, channels_interval=ci)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(n, ci, 0).items()})
    return m.to(dev), pkg.mse_loss()


def test_trainer_keeps_its_graph_under_a_per_step_schedule(pkg, dev, optim_mod, tmp_path):
    """FusedAdamW(device_lr=True, max_grad_norm=...) under a LambdaLR that changes the lr every step (Trainer.lr_scheduler): no
    warning, the graph stays, it is captured ONCE, and every parameter and moment equals the written-out eager loop with the same
    options, device_lr=False and the same lrs - bit for bit.  max_grad_norm sits inside the range of the 12 recorded norms: some steps
    clip and some do not."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    n, ci, sl = 4, 8, 1024
    ds = dataset_mod.Dataset(n_items=48, sample_length=sl, seed=3)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)
    sched = lambda k: 0.97 ** k                                                 # noqa: E731
    kw = dict(lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01)

    def eager(max_norm):
        m, crit = _make(pkg, dev, n, ci)
        opt = optim_mod.FusedAdamW(m.parameters(), max_grad_norm=max_norm, **kw)
        sch = torch.optim.lr_scheduler.LambdaLR(opt, sched)
        m.train()
        norms, lrs = [], []
        for mix, cl, _ in loader:
            lrs.append(opt.param_groups[0]["lr"])
            opt.zero_grad()
            crit(cl.to(dev), m(mix.to(dev))).backward()
            opt.step()
            norms.append(float(opt.last_grad_norm))
            sch.step()
        return m, opt, norms, lrs

    # the norms of the run decide the threshold: a first loop that never clips, its median norm becomes max_grad_norm
    _, _, free, _ = eager(1e30)
    max_norm = sorted(free)[len(free) // 2]
    m2, opt2, norms, lrs = eager(max_norm)
    assert len(norms) == 12 and len(set(lrs)) == 12
    assert any(v > max_norm for v in norms) and any(v <= max_norm for v in norms), (max_norm, norms)

    cfg = {"root_dir": str(tmp_path), "experiment_name": "s", "trainer": {"epochs": 1, "save_checkpoint_interval": 0}}
    m1, crit1 = _make(pkg, dev, n, ci)
    opt1 = optim_mod.FusedAdamW(m1.parameters(), device_lr=True, max_grad_norm=max_norm, **kw)
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, None)
    assert tr.use_graph and tr.lr_scheduler is None and tr.captures == 0
    tr.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(opt1, sched)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr.train()
    torch.cuda.synchronize()
    # (the Trainer's fall-back is a RuntimeWarning, torch's schedulers complain with UserWarnings)
    assert not [w for w in caught if issubclass(w.category, (RuntimeWarning, UserWarning))], [str(w.message) for w in caught]
    assert tr.use_graph and tr.captures == 1 and tr._graph is not None
    assert opt1.param_groups[0]["lr"] == opt2.param_groups[0]["lr"]
    assert float(opt1.last_grad_norm) == norms[-1]
    for (k, a), (_, b) in zip(m1.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    for p1, p2 in zip(m1.parameters(), m2.parameters()):
        s1, s2 = opt1.state[p1], opt2.state[p2]
        assert int(s1["step"]) == int(s2["step"]) == 12
        assert torch.equal(s1["exp_avg"], s2["exp_avg"]) and torch.equal(s1["exp_avg_sq"], s2["exp_avg_sq"])


def test_ten_replays_of_the_clipped_step_are_bitwise_equal(pkg, dev, optim_mod):
    """The captured step with clipping, weight decay and the device lr, replayed 10 times from the same restored state
    (test_gpu_determinism.py's pattern at its smallest shape): the partial sums of the norm are added in a fixed order, so the state
    after the replay - parameters, moments, running statistics, counter, hyper buffer with clip and norm - is the same 10 times."""
    n, ci, B, T = 5, 16, 4, 4096
    m = pkg.Model(n_layers=n, channels_interval=ci)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(n, ci, 0).items()})
    m.to(dev).train()
    crit = pkg.smooth_l1_loss()
    opt = optim_mod.FusedAdamW(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.01, device_step=True, device_lr=True,
                               max_grad_norm=1e-4)
    noisy, clean = plan.golden_batch(B, T, 3)
    x, y = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)

    def step():
        opt.zero_grad(set_to_none=True)
        loss = crit(y, m(x))
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        loss_g = step()
    opt.advance_host_step(-1)
    torch.cuda.synchronize()
    state = [t for t in m.state_dict().values()]
    for st in opt.state.values():
        state += [st["exp_avg"], st["exp_avg_sq"]]
    state += [t for bufs in opt._dev.values() for t in bufs]
    saved = [t.clone() for t in state]
    ref = None
    for it in range(10):
        with torch.no_grad():
            for t, s in zip(state, saved):
                t.copy_(s)
        graph.replay()
        torch.cuda.synchronize()
        now = [t.clone() for t in state] + [loss_g.clone()]
        if ref is None:
            ref = now
            assert all(torch.isfinite(t.float()).all() for t in ref)
            assert 0.0 < float(opt._dev[0][1][2]) < 1.0                          # the step really clipped
            continue
        bad = [k for k, (a, b) in enumerate(zip(now, ref)) if not torch.equal(a, b)]
        assert not bad, f"replay #{it} differs from #0 in state tensors {bad[:10]}"
