"""-m "not gpu": the options of the fused Adam step on the CPU emulator - gradient clipping by the global norm
(grad_sqnorm_partial_kernel + adam_hyper_kernel), decoupled weight decay (FusedAdamW) and the lr read from device memory
(adam_kernel's optional slots, csrc/wunet_adam.h behind wunet_adam_step_ex).  No reference counterpart (train.py:31-35 builds a plain
Adam): the yardstick is a float64 restatement of torch.nn.utils.clip_grad_norm_ + torch.optim.Adam / AdamW in torch's operation
order (tests/adam_options_ref.py); torch's own fp32 pair is printed for information.  wunet_adam_step and wunet_adam_step_ex run
ONE pair of kernels: the "bits of the plain step" tests below hold the two entry points' paths through it against each other (host
or one-thread hyper launch and a 2-float buffer against the one-block hyper launch and the optional slots); that the kernels kept
the bits they had as two pairs is tools/emu_lib_ab.py's comparison with a library of the commit before (profiles/adam_unify_ab.txt).

Measured on the emulator, 4 steps, max_grad_norm=5, lr changing every step (worst over FusedAdam and FusedAdamW; bar in brackets):
  mixed shapes (1 ... 256*1024+5 elements): norm 4.9e-8 [2.5e-7], exp_avg 1.0e-7 [1e-6], exp_avg_sq 2.3e-7 [2e-6],
                                             params 6.3e-7 [2.2e-6]
  70 small tensors (two table launches):    norm 4.0e-8 [2.5e-7], exp_avg 1.4e-7 [1e-6], exp_avg_sq 1.8e-7 [2e-6],
                                             params 5.3e-7 [1.7e-6]
  torch-fp32 on the mixed shapes (CPU):     norm 2.3e-6, exp_avg 2.3e-6, exp_avg_sq 4.2e-6, params 6.3e-7 (its norm is an fp32 sum whose
                                             error depends on how torch splits it over threads; up to 1.7e-5 has been seen)
"""
import copy
import ctypes
import importlib

import pytest
import torch

import adam_options_ref as R
import emu_lib
from conftest import PKG_NAME


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.fixture(scope="module")
def optim_mod():
    return importlib.import_module(PKG_NAME + ".optim")


_RUNS = {}


def _run(optim_mod, emu_engine, case, **kw):
    """One run per distinct set of options, shared by the tests of this module (the results are only read)."""
    key = (case,) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        _RUNS[key] = R.run_fused(optim_mod, case, engine=emu_engine, **kw)[0]
    return _RUNS[key]


def _equal(a, b):
    return all(torch.equal(x, y) for k in range(3) for x, y in zip(a[k], b[k]))


@pytest.mark.parametrize("decoupled", [False, True], ids=["FusedAdam", "FusedAdamW"])
@pytest.mark.parametrize("case", ["mixed", "many"])
def test_clipped_step_matches_the_float64_restatement(optim_mod, emu_engine, case, decoupled):
    """Four steps with max_grad_norm=5, gradient magnitudes 10^(it-2) and another lr every step: norm, moments and parameters within
    the bars of adam_options_ref (derived from the roundings per step), p.grad untouched (checked inside run_fused)."""
    got = _run(optim_mod, emu_engine, case, decoupled=decoupled)
    R.check_against_reference(f"{case} {'AdamW' if decoupled else 'Adam'}", got, case, decoupled)
    clipped = R.reference(case, decoupled)[4]
    if case == "many":
        assert any(clipped) and not all(clipped), clipped       # some steps clip and some do not
    else:
        assert any(clipped), clipped                            # (a quarter of a million elements: every step is above 5)
    # torch's fp32 pair against the same yardstick, for information (its norm is accumulated in fp32 over up to 262149 elements)
    d = R.distances(R.torch_fp32(case, decoupled), R.reference(case, decoupled))
    print(f"torch fp32 {case}: norm {d[0]:.2e}  exp_avg {d[1]:.2e}  exp_avg_sq {d[2]:.2e}  params {d[3]:.2e} (bar {d[4]:.2e})")


@pytest.mark.parametrize("device_step", [False, True], ids=["host_step", "device_step"])
@pytest.mark.parametrize("case", ["mixed", "many"])
def test_a_norm_that_never_clips_has_the_bits_of_the_plain_step(optim_mod, emu_engine, case, device_step):
    """max_grad_norm=1e30: clip is exactly 1 and adam_kernel with its optional slots must produce what it produces without them -
    parameters and moments."""
    plain = _run(optim_mod, emu_engine, case, max_grad_norm=None, device_step=device_step)
    never = _run(optim_mod, emu_engine, case, max_grad_norm=1e30, device_step=device_step)
    assert _equal(plain, never)
    assert never[3] == _run(optim_mod, emu_engine, case)[3]              # ... and the norm it reports is the clipped run's


@pytest.mark.parametrize("decoupled", [False, True], ids=["FusedAdam", "FusedAdamW"])
def test_device_lr_has_the_bits_of_the_host_lr(optim_mod, emu_engine, decoupled):
    """device_lr=True under an lr that changes every step == device_lr=False with the same lrs (lr / bc1 and 1 - lr * weight_decay
    are computed from the same double either way), with and without the device-side step counter."""
    host = _run(optim_mod, emu_engine, "mixed", decoupled=decoupled)
    for device_step in (False, True):
        dev = _run(optim_mod, emu_engine, "mixed", decoupled=decoupled, device_lr=True, device_step=device_step)
        assert _equal(host, dev) and host[3] == dev[3], device_step
    # without clipping or decay the device lr alone selects the _ex entry: still the plain step's bits
    assert _equal(_run(optim_mod, emu_engine, "many", max_grad_norm=None),
                  _run(optim_mod, emu_engine, "many", max_grad_norm=None, device_lr=True))


def test_grad_scale_with_clipping_is_clipping_of_prescaled_gradients(optim_mod, emu_engine):
    """grad_scale = 0.25 (the 1/world of a data-parallel average, folded into the step): the norm is that of the SCALED gradients
    and the result is the clipped step on gradients scaled beforehand - both against the float64 restatement with its bars."""
    for case in ("mixed", "many"):
        a = _run(optim_mod, emu_engine, case, grad_scale=0.25)
        b = _run(optim_mod, emu_engine, case, prescale=0.25)
        R.check_against_reference(f"{case} grad_scale", a, case, False, grad_scale=0.25)
        R.check_against_reference(f"{case} prescaled", b, case, False, grad_scale=0.25)
        assert a[3] == b[3]                                              # (0.25 * g is exact: the same sum)


def test_two_runs_are_bit_identical(optim_mod, emu_engine):
    a = _run(optim_mod, emu_engine, "mixed", decoupled=True)
    b = R.run_fused(optim_mod, "mixed", engine=emu_engine, decoupled=True)[0]
    assert _equal(a, b) and a[3] == b[3]


def test_options_are_attributes_and_part_of_the_signature(optim_mod, emu_engine):
    p = [torch.nn.Parameter(torch.ones(3))]
    fa = optim_mod.FusedAdam(p, lr=1e-3, max_grad_norm=2.0, device_lr=True)
    assert set(fa.param_groups[0]) == set(torch.optim.Adam([torch.nn.Parameter(torch.ones(1))]).param_groups[0])
    assert fa.max_grad_norm == 2.0 and fa.device_lr is True and fa.last_grad_norm is None
    sig = fa.hyper_signature()
    fa.param_groups[0]["lr"] = 5e-4
    assert fa.hyper_signature() == sig                                   # device_lr: the lr is not baked into the launches
    fa.max_grad_norm = 3.0
    assert fa.hyper_signature() != sig
    fb = optim_mod.FusedAdam(p, lr=1e-3)
    sig = fb.hyper_signature()
    fb.param_groups[0]["lr"] = 5e-4
    assert fb.hyper_signature() != sig
    fw = optim_mod.FusedAdamW(p, lr=1e-3, weight_decay=0.1)
    sig = fw.hyper_signature()
    fw.param_groups[0]["weight_decay"] = 0.2
    assert fw.hyper_signature() != sig
    with pytest.raises(ValueError):
        optim_mod.FusedAdam(p, max_grad_norm=0.0)
    with pytest.raises(ValueError):
        optim_mod.FusedAdamW(p, amsgrad=True)
    with pytest.raises(ValueError):
        optim_mod.FusedAdamW(p, maximize=True)
    # _dev[gi][0] stays the step counter, [1] the hyper buffer; the lr double and the partial sums are appended
    fa._engine_override = emu_engine
    fa.device_step = True
    p[0].grad = torch.full((3,), 2.0)
    fa.step()
    dev = fa._dev[0]
    assert int(dev[0]) == 1 and dev[1].dtype == torch.float32 and dev[2].dtype == torch.float64 and float(dev[2]) == 5e-4
    assert abs(float(fa.last_grad_norm) - 12 ** 0.5) < 1e-6 and fa.last_grad_norm.data_ptr() == dev[1][3].data_ptr()
    # sync_device_hyper(): a changed lr is written once, an unchanged one not at all
    fa.param_groups[0]["lr"] = 2e-4
    fa.sync_device_hyper()
    assert float(dev[2]) == 2e-4
    dev[2].fill_(7.0)                                                    # (behind its back: an unchanged lr must not be rewritten)
    fa.sync_device_hyper()
    assert float(dev[2]) == 7.0


def test_fused_adamw_state_round_trips_with_torch_adamw(optim_mod, emu_engine):
    """FusedAdamW's state_dict loads into torch.optim.AdamW and steps there, torch's loads into FusedAdamW (the pattern of
    test_fused_adam_state_round_trips_with_torch_adam); FusedAdam itself keeps refusing a weight_decay."""
    def params():
        torch.manual_seed(3)
        return [torch.nn.Parameter(torch.randn(5, 3)), torch.nn.Parameter(torch.randn(7))]

    def grads(ps, k):
        g = torch.Generator().manual_seed(10 + k)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)

    kw = dict(lr=2e-3, betas=(0.8, 0.99), weight_decay=0.05)
    pa, pb = params(), params()
    fa = optim_mod.FusedAdamW(pa, **kw)
    fa._engine_override = emu_engine
    ta = torch.optim.AdamW(pb, **kw)
    assert set(fa.param_groups[0]) == set(ta.param_groups[0])
    assert {k: v for k, v in fa.param_groups[0].items() if k != "params"} == {k: v for k, v in ta.param_groups[0].items() if k != "params"}
    for k in range(2):
        grads(pa, k); grads(pb, k)
        fa.step(); ta.step()
    # FusedAdamW -> torch.optim.AdamW: load and keep stepping
    pc = params()
    tc = torch.optim.AdamW(pc, **kw)
    tc.load_state_dict(copy.deepcopy(fa.state_dict()))
    with torch.no_grad():
        for p, q in zip(pc, pa):
            p.copy_(q)
    grads(pa, 2); grads(pb, 2); grads(pc, 2)
    fa.step(); ta.step(); tc.step()
    for a, b, c in zip(pa, pb, pc):
        assert (a - b).abs().max() < 1e-6 and (a - c).abs().max() < 1e-6
    # torch.optim.AdamW -> FusedAdamW
    pd = params()
    fd = optim_mod.FusedAdamW(pd, **kw)
    fd._engine_override = emu_engine
    fd.load_state_dict(copy.deepcopy(ta.state_dict()))
    assert fd.param_groups[0]["weight_decay"] == 0.05
    with torch.no_grad():
        for p, q in zip(pd, pb):
            p.copy_(q)
    grads(pb, 3); grads(pd, 3)
    ta.step(); fd.step()
    for b, d in zip(pb, pd):
        assert (b - d).abs().max() < 1e-6
    # the decay is really applied (a FusedAdam on the same gradients ends somewhere else) ...
    pe = params()
    fe = optim_mod.FusedAdam(pe, lr=2e-3, betas=(0.8, 0.99))
    fe._engine_override = emu_engine
    for k in range(3):
        grads(pe, k)
        fe.step()
    assert (pe[0] - pa[0]).abs().max() > 1e-5
    # ... and FusedAdam still refuses a checkpoint that asks for it; FusedAdamW refuses amsgrad
    with pytest.raises(ValueError, match="weight_decay"):
        fe.load_state_dict(ta.state_dict())
    bad = ta.state_dict()
    bad["param_groups"][0]["amsgrad"] = True
    with pytest.raises(ValueError):
        fd.load_state_dict(bad)


def test_trainer_takes_the_options_from_its_config_and_steps_the_scheduler(emu_engine, optim_mod, tmp_path):
    """config["trainer"]["max_grad_norm"] / ["device_lr"] reach a fused optimiser and are refused - not ignored - with another one;
    Trainer.lr_scheduler.step() runs after every optimiser step: the run equals the written-out loop with the same schedule."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    loss_mod = importlib.import_module(PKG_NAME + ".loss")
    model_mod = importlib.import_module(PKG_NAME + ".model")
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=6, sample_length=64, seed=1), batch_size=3, shuffle=False)

    def make():
        torch.manual_seed(0)
        m = model_mod.Model(n_layers=2, channels_interval=4)
        m._engine_override = emu_engine
        crit = loss_mod.mse_loss()
        crit._engine_override = emu_engine
        opt = optim_mod.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
        opt._engine_override = emu_engine
        return m, crit, opt

    cfg = {"root_dir": str(tmp_path), "experiment_name": "c", "trainer": {"epochs": 2, "max_grad_norm": 0.05, "device_lr": True}}
    m1, crit1, opt1 = make()
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, None)
    assert opt1.max_grad_norm == 0.05 and opt1.device_lr is True and tr.lr_scheduler is None and tr.captures == 0
    tr.device = torch.device("cpu")                                      # the emulator engine takes host tensors
    tr.model = m1.to("cpu")
    tr.lr_scheduler = torch.optim.lr_scheduler.LambdaLR(opt1, lambda k: 0.9 ** k)
    tr.train()
    m2, crit2, opt2 = make()
    opt2.max_grad_norm = 0.05
    m2.train()
    k, norms = 0, []
    for _ in range(2):
        for mix, cl, _ in loader:
            opt2.param_groups[0]["lr"] = 1e-3 * 0.9 ** k
            k += 1
            opt2.zero_grad()
            crit2(cl, m2(mix)).backward()
            opt2.step()
            norms.append(float(opt2.last_grad_norm))
    assert max(norms) > 0.05                                             # (the option did something)
    for (name, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), name
    assert float(opt1.last_grad_norm) == norms[-1] and tr.captures == 0
    with pytest.raises(ValueError, match="max_grad_norm"):
        trainer_mod.Trainer(cfg, False, m2, crit2, torch.optim.Adam(m2.parameters(), lr=1e-3), loader, None)
    cfg["trainer"] = {"epochs": 1, "device_lr": True}
    with pytest.raises(ValueError, match="device_lr"):
        trainer_mod.Trainer(cfg, False, m2, crit2, torch.optim.Adam(m2.parameters(), lr=1e-3), loader, None)


def test_adam_step_ex_refuses_bad_arguments(emu_engine):
    """The C ABI: argument errors come back as WUNET_E_ARG with a message, before anything is enqueued."""
    lib = emu_engine.lib
    assert lib.wunet_adam_scratch_bytes(0) == 0 and lib.wunet_adam_scratch_bytes(102) >= 102 * 8
    p, g, m, v = (torch.zeros(4) for _ in range(4))
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())                 # noqa: E731
    numels = (ctypes.c_size_t * 1)(4)
    hyper = torch.zeros(8)
    step = torch.zeros((), dtype=torch.int64)

    def call(hyper_ptr, max_norm=0.0, scratch=None, wd=0.0, step_no=1):
        return lib.wunet_adam_step_ex(1, arr(p), arr(g), arr(m), arr(v), numels, 1e-3, 0.9, 0.999, 1e-8, step_no, 1.0, wd, max_norm,
                                      step.data_ptr(), hyper_ptr, None, scratch, None)

    assert call(None) == -1 and b"hyper" in lib.wunet_last_error()      # WUNET_E_ARG: NULL hyper_dev
    assert call(hyper.data_ptr(), max_norm=1.0) == -1 and b"scratch" in lib.wunet_last_error()
    assert call(hyper.data_ptr(), wd=-0.1) == -1 and b"weight_decay" in lib.wunet_last_error()
    assert int(step) == 0 and not p.any() and not hyper.any()           # nothing ran
    with pytest.raises(RuntimeError, match="hyper_dev"):
        emu_engine.adam_step([p], [g], [m], [v], 1e-3, 0.9, 0.999, 1e-8, 1, max_grad_norm=1.0)
    assert call(hyper.data_ptr()) == 0 and int(step) == 1               # all options off: the plain step through the _ex entry


def test_each_entry_point_stays_inside_its_hyper_buffer(emu_engine):
    """wunet_adam_step (2 floats, or no buffer at all) and wunet_adam_step_ex (8 floats) run the same two kernels: neither writes a
    slot the other's buffer does not have (adam_options_ref.check_hyper_buffer_bounds)."""
    R.check_hyper_buffer_bounds(emu_engine.lib)
