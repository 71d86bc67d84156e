"""-m "not gpu": the STOI loss (stoi_spec_kernel<save> / stoi_loss_final_kernel / stoi_segment_bwd_kernel / stoi_spec_bwd_kernel /
stoi_unframe_kernel / stoi_resample_bwd_kernel, csrc/wunet_stoi.h behind wunet_stoi_loss_*) on the CPU emulator, through the public
loss.stoi_loss.  The yardstick is the float64 autograd gradient of tests/stoi_loss_ref.py; conditions and bars are those of
tests/stoi_loss_cases.py, and every case prints its d beside d_ref."""
import importlib

import numpy as np
import pytest
import torch

import emu_lib
import stoi_cases as C
import stoi_loss_cases as LC
import stoi_ref as R
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("name", C.EMU_CASES)
def test_loss_and_gradient_match_the_float64_oracle(emu_engine, name):
    LC.check_case(name, emu_engine, CPU)


def test_two_runs_are_bit_identical_and_grad_loss_scales_exactly(emu_engine):
    l1, g1 = LC.run(emu_engine, CPU, "b")
    l2, g2 = LC.run(emu_engine, CPU, "b")
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and g1.abs().max() > 0
    lh, gh = LC.run(emu_engine, CPU, "b", grad_loss=0.5)
    assert torch.equal(lh, l1) and torch.equal(gh, 0.5 * g1)             # (a power of two: exact through every stage)


def test_leading_dimensions_are_flattened(emu_engine):
    ref = LC.reference("f")
    c = ref["c"][:, None, :].repeat(1, 2, 1)
    e = ref["e"][:, None, :].repeat(1, 2, 1)
    loss, g = LC.run(emu_engine, CPU, "f", c, e)
    l1, g1 = LC.run(emu_engine, CPU, "f")
    assert g.shape == (2, 2, 5000) and torch.equal(g, (0.5 * g1)[:, None, :].repeat(1, 2, 1))      # (four rows: half the weight each)
    assert abs(float(loss) - float(l1)) <= 2.0 ** -23


def test_the_metric_keeps_its_bits_around_a_loss_call(emu_engine):
    """The loss and the metric share the per-rate tables and nothing else: metrics.stoi before and after a loss call, same bits."""
    before = C.run(emu_engine, CPU, "b")
    tables = emu_engine.stoi_tables(16000, CPU)
    snapshot = tables.clone()
    LC.run(emu_engine, CPU, "b")
    after = C.run(emu_engine, CPU, "b")
    assert emu_engine.stoi_tables(16000, CPU) is tables and torch.equal(tables, snapshot)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


@pytest.mark.parametrize("name", ("a", "b"))
def test_an_all_zero_estimate_and_an_all_zero_clean_row_give_zero_gradients(emu_engine, name):
    """The stated departure from autograd (NaN): a band magnitude of exactly 0 passes no gradient."""
    ref = LC.reference(name)
    e = ref["e"].clone()
    e[0] = 0.0
    loss, g = LC.run(emu_engine, CPU, name, ref["c"], e)
    assert torch.isfinite(loss) and torch.isfinite(g).all() and not g[0].any() and g[1].any()
    c = ref["c"].clone()
    c[1] = 0.0
    loss, g = LC.run(emu_engine, CPU, name, c, ref["e"])
    assert torch.isfinite(loss) and torch.isfinite(g).all() and not g[1].any() and g[0].any()


def test_weighted_loss_is_the_hand_written_sum(emu_engine):
    loss_mod = LC.loss_mod()
    ref = LC.reference("a")
    c, e = ref["c"], ref["e"]
    crit = loss_mod.weighted_loss([["l1_loss", 1.0], ["stoi_loss", 0.25, {"sample_rate": 10000}]])
    l1, st = loss_mod.l1_loss(), loss_mod.stoi_loss(sample_rate=10000)
    for m in list(crit.terms) + [l1, st]:
        m._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 1.0 * l1(c, y) + 0.25 * st(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = LC.run(emu_engine, CPU, "a")
    assert (x.grad - 0.25 * gs).abs().max() > 0 and gs.abs().max() > 0   # ... and both terms are in it


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    loss_mod = LC.loss_mod()
    c, e = R.pair(2, 5000, 10000)
    tables = emu_engine.stoi_tables(10000, CPU)
    scr = torch.zeros(lib.wunet_stoi_loss_scratch_bytes(2, 5000, 10000) // 8, dtype=torch.float64)
    saved = torch.zeros(lib.wunet_stoi_loss_saved_bytes(2, 5000, 10000) // 4 + 4)
    assert saved.data_ptr() % 16 == 0 and scr.data_ptr() % 16 == 0
    out, rows, frames = torch.zeros(()), torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    fwd = [c.data_ptr(), e.data_ptr(), 2, 5000, 10000, tables.data_ptr(), scr.data_ptr(), saved.data_ptr(), out.data_ptr(), rows.data_ptr(),
           frames.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (8, None, b"null"),
                       (2, 0, b"rows"), (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, 44100, b"taps"), (7, saved.data_ptr() + 4, b"aligned")):
        a = list(fwd)
        a[k] = v
        assert lib.wunet_stoi_loss_forward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not saved.any() and not out.any() and not rows.any()          # nothing ran
    assert lib.wunet_stoi_loss_scratch_bytes(0, 5000, 10000) == 0 and lib.wunet_stoi_loss_saved_bytes(2, 5000, 44100) == 0
    assert lib.wunet_stoi_loss_saved_bytes(70000, 5000, 10000) == 0 and lib.wunet_stoi_loss_scratch_bytes(2, 5000, 0) == 0
    fwd[9] = fwd[10] = None                                               # per_row_out and frames_out are optional
    assert lib.wunet_stoi_loss_forward(*fwd) == 0 and float(out) < -0.5 and not rows.any()
    fwd[9], fwd[10] = rows.data_ptr(), frames.data_ptr()
    assert lib.wunet_stoi_loss_forward(*fwd) == 0 and frames.tolist() == [33, 33]
    assert abs(float(out) + float(rows.double().mean())) <= 2.0 ** -22
    one, g = torch.ones(()), torch.zeros_like(e)
    bwd = [saved.data_ptr(), one.data_ptr(), 2, 5000, 10000, tables.data_ptr(), scr.data_ptr(), g.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (2, 0, b"rows"),
                       (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, 44100, b"taps"), (0, saved.data_ptr() + 4, b"aligned")):
        a = list(bwd)
        a[k] = v
        assert lib.wunet_stoi_loss_backward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not g.any() and lib.wunet_stoi_loss_backward(*bwd) == 0 and g.any()
    # rows too short for one frame: the constant, and zeros
    crit = LC.make(emu_engine, 10000)
    for T in (1, 256, 257, 3000):
        x = e[:, :T].clone().requires_grad_(True)
        loss = crit(c[:, :T], x)
        loss.backward()
        assert loss.item() == np.float32(-1e-5) and not x.grad.any(), T
    # the Python face
    for fs in (0, -16000, 44100):
        with pytest.raises(ValueError, match="stoi"):
            loss_mod.stoi_loss(sample_rate=fs)
    with pytest.raises(RuntimeError, match="mismatch"):
        crit(c, e[:1])
    with pytest.raises(RuntimeError, match="float32"):
        crit(c.double(), e.double())
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.clone().requires_grad_(True), e)


def test_the_new_symbols_are_exported_and_the_factory_is_reachable_by_name(pkg):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_stoi_loss_scratch_bytes", "wunet_stoi_loss_saved_bytes", "wunet_stoi_loss_forward", "wunet_stoi_loss_backward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    # the way the reference's initialize_config builds a loss from a config's "module" / "main" / "args"
    crit = getattr(importlib.import_module(PKG_NAME + ".loss"), "stoi_loss")(**{"sample_rate": 8000})
    assert crit.sample_rate == 8000 and callable(pkg.stoi_loss) and "stoi_loss" in LC.loss_mod()._FACTORIES
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_stoi_loss.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.stoi_loss()(torch.zeros(1, 1, 8192), torch.zeros(1, 1, 8192))


def test_one_training_step_reaches_every_parameter(emu_engine):
    model_mod = importlib.import_module(PKG_NAME + ".model")
    ref = LC.reference("a")
    torch.manual_seed(0)
    m = model_mod.Model(n_layers=2, channels_interval=4)
    m._engine_override = emu_engine
    crit = LC.make(emu_engine, 10000)
    out = m(ref["e"][:, None, :])
    assert out.shape == (2, 1, 5000)
    loss = crit(ref["c"][:, None, :], out)
    loss.backward()
    grads = [p.grad for p in m.parameters()]
    assert torch.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.any() for g in grads)
