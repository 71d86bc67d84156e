"""-m "not gpu": the row losses - scale-invariant SDR and SNR per utterance (loss_rows_partial_kernel / loss_rows_final_kernel /
loss_rows_bwd_kernel, csrc/wunet_loss_rows.h behind wunet_loss_rows_forward / _backward) - on the CPU emulator, through the public
modules (loss.si_sdr_loss / snr_loss, metrics.si_sdr / snr).  No reference counterpart: the yardstick is the definition in float64
torch with autograd (tests/si_sdr_ref.py); the bars are the issue's: values 2^-22 * max(|ref|, 1) = 2.4e-7, gradient 1e-5 of each
row's largest element.

Measured on the emulator (worst over both kinds and zero_mean on / off; bar in brackets):
  shapes (1,1) ... (100,8200):             values 5.7e-8 [2.4e-7], gradient 5.7e-8 [1e-5]
  input-SNR ladder -10 ... 60 dB, T 4096: values 4.9e-8 [2.4e-7], gradient 5.1e-8 [1e-5]; the 80 dB row's gradient 4.7e-8 too
  4-byte-aligned bases:                   values 2.9e-8, gradient 4.7e-8
  degenerate rows (T 64):                 s = e = 0: exactly 0 dB and a zero gradient; s = 0: -98.31 dB; e = s: +96.77 dB, whose
                                          gradient is 1.1e-6 of its largest element off (A e and C s cancel to 1.6e-10 of themselves
                                          there, in the yardstick's float64 as in the kernel's)
(6e-8 = half an ulp of float: the one rounding of the output.)
"""
import ctypes
import importlib

import pytest
import torch

import emu_lib
import loss_rows_cases as C
import si_sdr_ref as R
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("zero_mean", [True, False], ids=["zero_mean", "raw"])
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_and_gradient_match_the_float64_definition(emu_engine, shape, kind, zero_mean):
    s, e = R.pair(*shape)
    C.check_case(f"{kind} {shape} zero_mean={zero_mean}", emu_engine, CPU, kind, zero_mean, s, e)


@pytest.mark.parametrize("zero_mean", [True, False], ids=["zero_mean", "raw"])
@pytest.mark.parametrize("kind", C.KINDS)
def test_the_input_snr_ladder(emu_engine, kind, zero_mean):
    """e = 0.7 s + noise at -10 ... 80 dB: the values at every row, the gradient bar at every row up to 60 dB (the issue's range);
    the 80 dB row's gradient is printed."""
    s, e = R.ladder(4096)
    upto60 = [k for k, db in enumerate(R.LADDER_DB) if db <= 60.0]
    _, _, _, rows, g = C.check_case(f"ladder {kind} zero_mean={zero_mean}", emu_engine, CPU, kind, zero_mean, s, e, grad_rows=upto60)
    if kind == "si_sdr":
        want = torch.tensor(R.LADDER_DB) + 20.0 * torch.log10(torch.tensor(0.7))
        # (the ladder is what it says, -13.1 ... 76.9 dB; at -10 dB the noise's chance correlation with s moves alpha by ~10 %: ~1 dB)
        assert (rows - want).abs().max() < 2.0, rows
    rg = R.reference(kind, s, e, zero_mean)[2]
    d80 = (g[-1].double() - rg[-1]).abs().max() / rg[-1].abs().max()
    print(f"ladder {kind}: 80 dB row, gradient {d80:.2e} of its largest element")


@pytest.mark.parametrize("kind", C.KINDS)
def test_a_base_with_4_byte_alignment_only(emu_engine, kind):
    """Inputs as views one float into their buffers (the loss's own gradient buffer is aligned: the backward's scalar path), then
    the C entry with the gradient one float into its buffer too (16-byte stores behind a scalar head), then inputs that disagree
    modulo 16 (the forward's scalar path)."""
    Rr, T = 3, 1031
    s, e, sv, ev = C.unaligned(Rr, T, CPU)
    assert sv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and sv.is_contiguous()
    _, _, loss, _, g = C.check_case(f"unaligned {kind}", emu_engine, CPU, kind, True, sv, ev)
    lib = emu_engine.lib
    _, coefs, _ = emu_engine.loss_rows_forward(kind, sv, ev)
    gbuf = torch.full((Rr * T + 8,), float("nan"))
    one = torch.ones(())
    assert lib.wunet_loss_rows_backward(3 if kind == "si_sdr" else 4, sv.data_ptr(), ev.data_ptr(), coefs.data_ptr(), one.data_ptr(), Rr, T, gbuf[1:].data_ptr(), None) == 0
    assert torch.equal(gbuf[1:1 + Rr * T].view(Rr, 1, T), g)             # same arithmetic per element, whichever path stores it
    assert torch.isnan(gbuf[0]) and torch.isnan(gbuf[1 + Rr * T:]).all()  # nothing written outside
    loss2, g2 = C.run(emu_engine, CPU, kind, True, sv, e)                # clean at 4 mod 16, enhanced at 0: scalar loads
    rl, _, rg = R.reference(kind, s, e, True)
    R.check_values(f"mixed alignment {kind}", loss2, None, rl, None)
    R.check_grad(f"mixed alignment {kind}", g2, rg)


@pytest.mark.parametrize("kind", C.KINDS)
def test_degenerate_rows_stay_finite(emu_engine, kind):
    C.check_degenerate(emu_engine, CPU, kind)


@pytest.mark.parametrize("kind", C.KINDS)
def test_grad_loss_scales_exactly_and_a_second_backward_works(emu_engine, kind):
    s, e = R.pair(5, 4099)
    _, g1 = C.run(emu_engine, CPU, kind, True, s, e)
    _, gq = C.run(emu_engine, CPU, kind, True, s, e, grad_loss=0.25)
    assert torch.equal(gq, 0.25 * g1)                                    # a power of two: exact
    loss_mod, _ = C.mods()
    crit = loss_mod.si_sdr_loss() if kind == "si_sdr" else loss_mod.snr_loss()
    crit._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(s, x)
    loss.backward(retain_graph=True)
    loss.backward()                                                      # the saved coefficients are still there
    assert torch.equal(x.grad, 2.0 * g1)
    with pytest.raises(NotImplementedError, match="clean"):
        crit(s.clone().requires_grad_(True), x)


def test_two_runs_are_bit_identical(emu_engine):
    s, e = R.pair(1, 200003)
    for kind in C.KINDS:
        la, ga = C.run(emu_engine, CPU, kind, True, s, e)
        lb, gb = C.run(emu_engine, CPU, kind, True, s, e)
        assert torch.equal(la, lb) and torch.equal(ga, gb)
        assert torch.equal(C.rows_db(emu_engine, CPU, kind, True, s, e), C.rows_db(emu_engine, CPU, kind, True, s, e))


def test_metrics_are_the_loss_rows_bit_for_bit(emu_engine):
    """metrics.si_sdr / snr return what the loss's forward computes per row (the coefficient tensor's fourth column rounded once);
    the loss is minus their mean; si_sdr_improvement is the difference of two such calls."""
    _, metrics = C.mods()
    s, e = R.pair(70, 257)
    noisy = s + 0.5 * torch.randn(s.shape, generator=torch.Generator().manual_seed(9))
    for kind in C.KINDS:
        loss, coefs, rows = emu_engine.loss_rows_forward(kind, s, e, per_row=True)
        got = C.rows_db(emu_engine, CPU, kind, True, s, e)
        assert got.shape == (70,) and got.dtype == torch.float32
        assert torch.equal(got, rows) and torch.equal(got, coefs[:, 3].float())
        assert abs(float(loss) + coefs[:, 3].mean().item()) <= 2.0 ** -22 * max(1.0, abs(float(loss)))
    imp = metrics.si_sdr_improvement(s, noisy, e, engine=emu_engine)
    assert torch.equal(imp, metrics.si_sdr(s, e, engine=emu_engine) - metrics.si_sdr(s, noisy, engine=emu_engine))
    pkg = importlib.import_module(PKG_NAME)
    for name in ("si_sdr_loss", "snr_loss", "si_sdr", "snr", "si_sdr_improvement"):
        assert callable(getattr(pkg, name))


def test_argument_errors_come_back_as_codes(emu_engine):
    lib = emu_engine.lib
    s, e = R.pair(2, 64)
    out, coefs = torch.zeros(()), torch.zeros(2, 6, dtype=torch.float64)
    assert lib.wunet_loss_rows_scratch_bytes(0, 64) == 0
    nbytes = lib.wunet_loss_rows_scratch_bytes(2, 64)
    assert nbytes >= 2 * 5 * 8 and lib.wunet_loss_rows_scratch_bytes(1, 1 << 22) >= 256 * 5 * 8     # one long row: many pieces
    assert lib.wunet_loss_rows_scratch_bytes(256, 16384) <= 2 * 256 * 5 * 8                          # many rows: no piece per CU each
    scratch = torch.zeros(nbytes // 8, dtype=torch.float64)

    def fwd(kind=3, eps=1e-8, rows=2, T=64, clean=s.data_ptr(), enh=e.data_ptr(), loss=out.data_ptr(), scr=scratch.data_ptr()):
        return lib.wunet_loss_rows_forward(kind, 1, eps, clean, enh, rows, T, loss, None, coefs.data_ptr(), scr, None)

    for bad in (dict(kind=0), dict(kind=2), dict(kind=5), dict(rows=0), dict(T=0), dict(clean=None), dict(enh=None), dict(loss=None),
                dict(scr=None), dict(eps=-1e-8), dict(eps=float("inf")), dict(eps=float("nan"))):
        assert fwd(**bad) == -1 and lib.wunet_last_error(), bad           # WUNET_E_ARG with a message
    assert b"eps" in lib.wunet_last_error()
    assert not out.any() and not coefs.any()                             # nothing ran
    assert fwd() == 0 and fwd(eps=0.0) == 0
    one = torch.ones(())
    g = torch.zeros_like(e)
    args = [3, s.data_ptr(), e.data_ptr(), coefs.data_ptr(), one.data_ptr(), 2, 64, g.data_ptr(), None]
    for k, v in ((0, 0), (0, 5), (1, None), (2, None), (3, None), (4, None), (7, None), (5, 0), (6, 0)):
        a = list(args)
        a[k] = v
        assert lib.wunet_loss_rows_backward(*a) == -1, k
    assert not g.any() and lib.wunet_loss_rows_backward(*args) == 0 and g.any()
    # the element-wise entry keeps refusing the row kinds
    scr = torch.zeros(lib.wunet_loss_scratch_bytes() // 8, dtype=torch.float64)
    for kind in (3, 4):
        assert lib.wunet_loss_forward(kind, s.data_ptr(), e.data_ptr(), 128, out.data_ptr(), scr.data_ptr(), None) == -1
        assert lib.wunet_loss_backward(kind, s.data_ptr(), e.data_ptr(), one.data_ptr(), 128, g.data_ptr(), None) == -1
    # ... and the Python face refuses what the C entry cannot see
    with pytest.raises(RuntimeError, match="mismatch"):
        emu_engine.loss_rows_forward("si_sdr", s, e[:1])
    with pytest.raises(RuntimeError, match="unknown kind"):
        emu_engine.loss_rows_forward("mse", s, e)
    _, good, _ = emu_engine.loss_rows_forward("si_sdr", s, e)
    with pytest.raises(RuntimeError, match="mismatch"):
        emu_engine.loss_rows_backward("si_sdr", s, e[:1], good, one)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.loss_rows_backward("si_sdr", s.long(), e, good, one)
    with pytest.raises(RuntimeError, match="coefs"):
        emu_engine.loss_rows_backward("si_sdr", s, e, good[:1], one)
    with pytest.raises(ValueError, match="eps"):
        C.mods()[0].si_sdr_loss(eps=-1.0)


def test_mse_through_the_old_entry_keeps_its_bits(emu_engine):
    """loss.mse_loss (the element-wise family, untouched) == wunet_loss_forward / _backward called directly, loss and gradient."""
    loss_mod, _ = C.mods()
    s, e = R.pair(5, 4099)
    crit = loss_mod.mse_loss()
    crit._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(s, x)
    loss.backward()
    lib = emu_engine.lib
    out, one, g = torch.zeros(()), torch.ones(()), torch.zeros_like(e)
    scr = torch.zeros(lib.wunet_loss_scratch_bytes() // 8, dtype=torch.float64)
    assert lib.wunet_loss_forward(0, s.data_ptr(), e.data_ptr(), e.numel(), out.data_ptr(), scr.data_ptr(), None) == 0
    assert lib.wunet_loss_backward(0, s.data_ptr(), e.data_ptr(), one.data_ptr(), e.numel(), g.data_ptr(), None) == 0
    assert torch.equal(loss.detach(), out) and torch.equal(x.grad, g)
    ref = ((e.double() - s.double()) ** 2).mean()
    assert abs(float(out) - float(ref)) < 1e-6 * float(ref)


def test_no_cpu_fallback_for_the_row_losses(pkg):
    if torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_loss_rows.py covers a GPU box)
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.si_sdr_loss()(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.si_sdr(torch.zeros(1, 1, 64), torch.zeros(1, 1, 64))


def test_trainer_validation_is_opt_in_and_restores_every_training_flag(emu_engine, tmp_path):
    """Without "metric" the validation loader stays unused; with it, every `interval` epochs the score is the mean SI-SDR improvement
    of inference.enhance's output over the recordings (by hand here), best_model.tar is written in the checkpoint layout, best_score
    comes back on resume - and a validation epoch leaves every module's training flag as it found it (a frozen BatchNorm layer)."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    model_mod = importlib.import_module(PKG_NAME + ".model")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    inference = importlib.import_module(PKG_NAME + ".inference")
    loss_mod, metrics = C.mods()
    sl = 64
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=6, sample_length=sl, seed=1), batch_size=3, shuffle=False)
    vloader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=2, sample_length=3 * sl + 17, seed=4, mode="validation"),
                                          batch_size=1, shuffle=False)

    def make():
        torch.manual_seed(0)
        m = model_mod.Model(n_layers=2, channels_interval=4)
        m._engine_override = emu_engine
        crit = loss_mod.si_sdr_loss()
        crit._engine_override = emu_engine
        opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3)
        opt._engine_override = emu_engine
        return m, crit, opt

    def by_hand(m):
        was = m.training
        m.eval()
        gains = [metrics.si_sdr_improvement(cl, mix, inference.enhance(m, mix, sl), engine=emu_engine) for mix, cl, _ in vloader]
        m.train(was)
        return torch.cat(gains).double().mean().item()

    # no "metric": nothing changes
    cfg = {"root_dir": str(tmp_path), "experiment_name": "a", "trainer": {"epochs": 1, "validation": {"interval": 1}}}
    m0, crit0, opt0 = make()
    tr0 = trainer_mod.Trainer(cfg, False, m0, crit0, opt0, loader, vloader)
    assert tr0.validation_interval == 0
    tr0.train()
    assert tr0.validation_scores == [] and tr0.best_score == float("-inf") and not (tr0.checkpoints_dir / "best_model.tar").exists()
    with pytest.raises(ValueError, match="si_sdr"):
        trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": {"metric": "stoi", "interval": 1}}}, False, m0, crit0, opt0, loader, vloader)
    # opted in, interval 2 of 4 epochs
    cfg = {"root_dir": str(tmp_path), "experiment_name": "b",
           "trainer": {"epochs": 4, "validation": {"metric": "si_sdr", "interval": 2, "custom": {"sample_length": sl}}}}
    m1, crit1, opt1 = make()
    tr = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, vloader)
    m2, crit2, opt2 = make()
    m2.train()
    scores = []
    for epoch in range(1, 5):
        for mix, cl, _ in loader:
            opt2.zero_grad()
            crit2(cl, m2(mix)).backward()
            opt2.step()
        if epoch % 2 == 0:
            scores.append(by_hand(m2))
    tr.train()
    assert tr.validation_scores == scores and len(scores) == 2
    assert tr.best_score == max(scores) and (tr.checkpoints_dir / "best_model.tar").exists()
    ck = torch.load((tr.checkpoints_dir / "best_model.tar").as_posix())
    assert set(ck) == {"epoch", "best_score", "optimizer", "model"} and ck["best_score"] == max(scores)
    assert ck["epoch"] == (4 if scores[1] >= scores[0] else 2)
    m3, crit3, opt3 = make()
    tr3 = trainer_mod.Trainer(cfg, True, m3, crit3, opt3, loader, vloader)
    assert tr3.best_score == max(scores) and tr3.start_epoch == ck["epoch"] + 1
    # find_max false starts from +inf and keeps the smallest
    cfg["trainer"]["validation"]["find_max"] = False
    cfg["experiment_name"] = "c"
    trm = trainer_mod.Trainer(cfg, False, m1, crit1, opt1, loader, vloader)
    assert trm.best_score == float("inf") and trm._is_best(1.0) and not trm._is_best(2.0) and trm.best_score == 1.0
    # the flags: one frozen BatchNorm layer in a training model
    m1.train()
    m1.encoder[1].main[1].eval()
    before = [(mod, mod.training) for mod in m1.modules()]
    frozen = m1._bn_frozen()
    assert any(frozen) and not all(frozen)
    score = tr._validation_epoch(5)
    assert all(mod.training == was for mod, was in before) and m1._bn_frozen() == frozen
    assert score == by_hand_keeping_flags(m1, vloader, sl, emu_engine) == tr.validation_scores[-1]


def by_hand_keeping_flags(m, vloader, sl, engine):
    inference = importlib.import_module(PKG_NAME + ".inference")
    _, metrics = C.mods()
    flags = [(mod, mod.training) for mod in m.modules()]
    m.eval()
    gains = [metrics.si_sdr_improvement(cl, mix, inference.enhance(m, mix, sl), engine=engine) for mix, cl, _ in vloader]
    for mod, was in flags:
        mod.training = was
    return torch.cat(gains).double().mean().item()
