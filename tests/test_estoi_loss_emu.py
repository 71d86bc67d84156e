"""-m "not gpu": the ESTOI loss (estoi_segment_kernel forward; estoi_segment_bwd_kernel + estoi_gather_kernel in stoi_segment_bwd_kernel's
place, csrc/wunet_estoi.h behind wunet_estoi_loss_*) on the CPU emulator, through the public loss.stoi_loss(extended=True).  The
yardstick is the float64 autograd gradient of tests/estoi_ref.py; conditions and bars are those of tests/estoi_cases.py, and every case
prints its d beside d_ref."""
import importlib

import numpy as np
import pytest
import torch

import emu_lib
import estoi_cases as EC
import estoi_ref as E
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
    EC.check_loss_case(name, emu_engine, CPU)


def test_two_runs_are_bit_identical_and_grad_loss_scales_exactly(emu_engine):
    l1, g1 = EC.run_loss(emu_engine, CPU, "b")
    l2, g2 = EC.run_loss(emu_engine, CPU, "b")
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and g1.abs().max() > 0
    lh, gh = EC.run_loss(emu_engine, CPU, "b", grad_loss=0.5)
    assert torch.equal(lh, l1) and torch.equal(gh, 0.5 * g1)             # (a power of two: exact through every stage)


def test_leading_dimensions_are_flattened(emu_engine):
    ref = E.case_reference(*C.CASES["f"])
    c = ref["c"][:, None, :].repeat(1, 2, 1)
    e = ref["e"][:, None, :].repeat(1, 2, 1)
    loss, g = EC.run_loss(emu_engine, CPU, "f", c, e)
    l1, g1 = EC.run_loss(emu_engine, CPU, "f")
    assert g.shape == (2, 2, 5000) and torch.equal(g, (0.5 * g1)[:, None, :].repeat(1, 2, 1))      # (four rows: half the weight each)
    assert abs(float(loss) - float(l1)) <= 2.0 ** -23


@pytest.mark.parametrize("name", ("a", "b"))
def test_inputs_with_4_byte_alignment_only(emu_engine, name):
    cv, ev = EC.offset_views(name, CPU)
    loss, g = EC.check_loss_case(name, emu_engine, CPU, c=cv, e=ev)
    la, ga = EC.run_loss(emu_engine, CPU, name)
    assert torch.equal(loss, la) and torch.equal(g, ga)


def test_an_all_zero_estimate_gives_loss_zero_and_a_zero_gradient(emu_engine):
    """The stated conventions: an all-zero estimate scores exactly 0.0 with an all-zero, finite gradient (autograd: NaN); a zero row
    beside a live one leaves the live row's gradient alone (up to its weight)."""
    ref = E.case_reference(*C.CASES["a"])
    loss, g = EC.run_loss(emu_engine, CPU, "a", ref["c"], torch.zeros_like(ref["e"]))
    assert float(loss) == 0.0 and torch.isfinite(g).all() and not g.any()
    e = ref["e"].clone()
    e[0] = 0.0
    loss, g = EC.run_loss(emu_engine, CPU, "a", ref["c"], e)
    _, g_full = EC.run_loss(emu_engine, CPU, "a")
    assert torch.isfinite(loss) and torch.isfinite(g).all() and not g[0].any() and torch.equal(g[1], g_full[1])
    c = ref["c"].clone()
    c[1] = 0.0
    loss, g = EC.run_loss(emu_engine, CPU, "a", c, ref["e"])
    assert torch.isfinite(loss) and torch.isfinite(g).all() and not g[1].any() and g[0].any()


def test_the_keyword_off_is_the_loss_without_it(emu_engine):
    loss_mod = EC.loss_mod()
    assert loss_mod.stoi_loss().extended is False and loss_mod.stoi_loss(16000, True).extended is True
    assert loss_mod.stoi_loss(sample_rate=8000, extended=True).sample_rate == 8000
    plain = LC.run(emu_engine, CPU, "a")
    crit = loss_mod.stoi_loss(sample_rate=10000, extended=False)
    crit._engine_override = emu_engine
    ref = E.case_reference(*C.CASES["a"])
    e = ref["e"].clone().requires_grad_(True)
    loss = crit(ref["c"], e)
    loss.backward()
    ext = EC.run_loss(emu_engine, CPU, "a")
    assert torch.equal(loss.detach(), plain[0]) and torch.equal(e.grad, plain[1])
    assert abs(float(ext[0]) - float(plain[0])) > 0.1 and not torch.equal(ext[1], plain[1])
    again = LC.run(emu_engine, CPU, "a")
    assert torch.equal(again[0], plain[0]) and torch.equal(again[1], plain[1])


def test_weighted_loss_reaches_the_extended_term(emu_engine):
    loss_mod = EC.loss_mod()
    ref = E.case_reference(*C.CASES["a"])
    c, e = ref["c"], ref["e"]
    crit = loss_mod.weighted_loss([["l1_loss", 1.0], ["stoi_loss", 0.25, {"sample_rate": 10000, "extended": True}]])
    assert crit.terms[1].extended is True and crit.terms[1].sample_rate == 10000
    l1, st = loss_mod.l1_loss(), loss_mod.stoi_loss(sample_rate=10000, extended=True)
    for m in list(crit.terms) + [l1, st]:
        m._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 1.0 * l1(c, y) + 0.25 * st(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = EC.run_loss(emu_engine, CPU, "a")
    assert (x.grad - 0.25 * gs).abs().max() > 0 and gs.abs().max() > 0   # ... and both terms are in it
    assert loss_mod._FACTORIES == ("mse_loss", "l1_loss", "smooth_l1_loss", "si_sdr_loss", "snr_loss", "stft_loss", "stoi_loss")


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    """wunet_estoi_loss_*: the cases of the wunet_stoi_loss_* test, with the words the STOI entry points use."""
    lib = emu_engine.lib
    c, e = R.pair(2, 5000, 10000)
    tables = emu_engine.stoi_tables(10000, CPU)
    n_scr, n_saved = lib.wunet_estoi_loss_scratch_bytes(2, 5000, 10000), lib.wunet_estoi_loss_saved_bytes(2, 5000, 10000)
    assert n_saved == lib.wunet_stoi_loss_saved_bytes(2, 5000, 10000)
    assert n_scr >= 2 * (33 - 29) * 450 * 8 and n_scr > lib.wunet_stoi_loss_scratch_bytes(2, 5000, 10000)     # (the segments' gradient blocks)
    scr = torch.zeros(n_scr // 8, dtype=torch.float64)
    saved = torch.zeros(n_saved // 4 + 4)
    assert saved.data_ptr() % 16 == 0 and scr.data_ptr() % 16 == 0
    out, rows, frames = torch.zeros(()), torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    fwd = [c.data_ptr(), e.data_ptr(), 2, 5000, 10000, tables.data_ptr(), scr.data_ptr(), saved.data_ptr(), out.data_ptr(), rows.data_ptr(),
           frames.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (8, None, b"null"),
                       (2, 0, b"rows"), (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, 44100, b"taps"), (7, saved.data_ptr() + 4, b"aligned")):
        a = list(fwd)
        a[k] = v
        assert lib.wunet_estoi_loss_forward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
        want = lib.wunet_last_error()
        assert lib.wunet_stoi_loss_forward(*a) == -1 and lib.wunet_last_error() == want
    assert not saved.any() and not out.any() and not rows.any()          # nothing ran
    assert lib.wunet_estoi_loss_scratch_bytes(0, 5000, 10000) == 0 and lib.wunet_estoi_loss_saved_bytes(2, 5000, 44100) == 0
    assert lib.wunet_estoi_loss_saved_bytes(70000, 5000, 10000) == 0 and lib.wunet_estoi_loss_scratch_bytes(2, 5000, 0) == 0
    fwd[9] = fwd[10] = None                                               # per_row_out and frames_out are optional
    assert lib.wunet_estoi_loss_forward(*fwd) == 0 and -0.5 < float(out) < -0.1 and not rows.any()
    fwd[9], fwd[10] = rows.data_ptr(), frames.data_ptr()
    assert lib.wunet_estoi_loss_forward(*fwd) == 0 and frames.tolist() == [33, 33]
    assert abs(float(out) + float(rows.double().mean())) <= 2.0 ** -22
    one, g = torch.ones(()), torch.zeros_like(e)
    bwd = [saved.data_ptr(), one.data_ptr(), 2, 5000, 10000, tables.data_ptr(), scr.data_ptr(), g.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (2, 0, b"rows"),
                       (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, 44100, b"taps"), (0, saved.data_ptr() + 4, b"aligned")):
        a = list(bwd)
        a[k] = v
        assert lib.wunet_estoi_loss_backward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not g.any() and lib.wunet_estoi_loss_backward(*bwd) == 0 and g.any()
    # rows too short for one frame: the constant, and zeros
    crit = EC.make_loss(emu_engine, 10000)
    for T in (1, 256, 257, 3000):
        x = e[:, :T].clone().requires_grad_(True)
        loss = crit(c[:, :T], x)
        loss.backward()
        assert loss.item() == np.float32(-1e-5) and not x.grad.any(), T
    # the Python face
    for fs in (0, -16000, 44100):
        with pytest.raises(ValueError, match="stoi"):
            EC.loss_mod().stoi_loss(sample_rate=fs, extended=True)
    with pytest.raises(RuntimeError, match="mismatch"):
        crit(c, e[:1])
    with pytest.raises(RuntimeError, match="float32"):
        crit(c.double(), e.double())
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.clone().requires_grad_(True), e)
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_estoi.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            EC.loss_mod().stoi_loss(extended=True)(torch.zeros(1, 1, 8192), torch.zeros(1, 1, 8192))


def test_one_training_step_reaches_every_parameter(emu_engine):
    model_mod = importlib.import_module(PKG_NAME + ".model")
    ref = E.case_reference(*C.CASES["a"])
    torch.manual_seed(0)
    m = model_mod.Model(n_layers=2, channels_interval=4)
    m._engine_override = emu_engine
    crit = EC.make_loss(emu_engine, 10000)
    out = m(ref["e"][:, None, :])
    loss = crit(ref["c"][:, None, :], out)
    loss.backward()
    grads = [p.grad for p in m.parameters()]
    assert torch.isfinite(loss) and all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.any() for g in grads)
