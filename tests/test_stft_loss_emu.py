"""-m "not gpu": the multi-resolution STFT loss (stft_basis_kernel / stft_fwd_kernel / stft_final_kernel / stft_bwd_kernel /
stft_ola_kernel, csrc/wunet_stft.h behind wunet_stft_*) on the CPU emulator, through the public modules (loss.stft_loss,
loss.weighted_loss, metrics.stft_magnitude).  No reference counterpart: the yardstick is the definition in float64 on torch.stft
under autograd (tests/stft_loss_ref.py); the bars are multiples of the distance d_ref at which two float32 computations on the CPU
land from it on the same inputs - loss 4 d_ref + 2^-23, gradient 4 d_ref, magnitudes 4 d_ref - and every test prints its d and d_ref."""
import ctypes
import importlib

import pytest
import torch

import emu_lib
import stft_loss_cases as C
import stft_loss_ref as R
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("name", C.EMU_CASES)
def test_loss_and_gradient_match_the_float64_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


@pytest.mark.parametrize("name", C.EMU_CASES)
def test_stft_magnitude_matches_torch_stft(emu_engine, name):
    C.check_magnitudes(name, emu_engine, CPU)


def test_a_zero_row_gets_a_zero_gradient_and_a_zero_clean_stays_finite(emu_engine):
    rows, T, res = C.CASES["a"]
    c, e = R.pair(rows, T)
    e = e.clone()
    e[1] = 0.0
    loss, g = C.run(emu_engine, CPU, res, c, e)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert not g[1].any() and g[0].any() and g[2].any()                 # every bin of the row sits below the clamp: no gradient
    l64, g64 = R.oracle64(c, e, res)
    assert R.d_loss(loss, l64) < 1e-5 and not g64[1].any()
    loss, g = C.run(emu_engine, CPU, res, torch.zeros_like(c), e)
    assert torch.isfinite(loss) and torch.isfinite(g).all() and float(loss) > 0.0


def test_equal_signals_give_exactly_zero_and_a_finite_gradient(emu_engine):
    """The stated departure from autograd: sum (S_c - S_e)^2 == 0 contributes 0 to the gradient, not NaN."""
    rows, T, res = C.CASES["d"]
    c, _ = R.pair(rows, T)
    loss, g = C.run(emu_engine, CPU, res, c, c.clone())
    assert float(loss) == 0.0 and torch.isfinite(g).all()


def test_grad_loss_scales_exactly_and_two_runs_are_bit_identical(emu_engine):
    rows, T, res = C.CASES["d"]
    c, e = R.pair(rows, T)
    l1, g1 = C.run(emu_engine, CPU, res, c, e)
    l2, g2 = C.run(emu_engine, CPU, res, c, e)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _, gh = C.run(emu_engine, CPU, res, c, e, grad_loss=0.5)
    assert torch.equal(gh, 0.5 * g1)                                     # a power of two: exact, through every resolution's accumulation


def test_weighted_loss_is_the_hand_written_sum(emu_engine):
    loss_mod, _ = C.mods()
    rows, T, res = C.CASES["a"]
    c, e = R.pair(rows, T)
    args = {"fft_sizes": [64], "hop_sizes": [16], "win_lengths": [48]}
    crit = loss_mod.weighted_loss([["l1_loss", 1.0], ["stft_loss", 0.5, args]])
    l1, st = loss_mod.l1_loss(), loss_mod.stft_loss(**args)
    for m in list(crit.terms) + [l1, st]:
        m._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 1.0 * l1(c, y) + 0.5 * st(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = C.run(emu_engine, CPU, res, c, e)
    assert (x.grad - 0.5 * gs).abs().max() > 0                           # ... and the l1 term is in it
    with pytest.raises(ValueError, match="unknown loss"):
        loss_mod.weighted_loss([["nope", 1.0]])
    with pytest.raises(ValueError, match="at least one"):
        loss_mod.weighted_loss([])


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    loss_mod, metrics = C.mods()
    lib = emu_engine.lib
    c, e = R.pair(2, 128)
    T = 128
    basis = emu_engine.stft_basis(64, 48, CPU)
    scr = torch.zeros(lib.wunet_stft_scratch_bytes(2, T, 64, 16, 1) // 8 + 1, dtype=torch.float64)
    saved = torch.zeros(lib.wunet_stft_saved_bytes(2, T, 64, 16) // 4)
    assert saved.numel() == 3 * 2 * (1 + T // 16) * 64 and basis.numel() == 64 * 2 * 64

    def fwd(N=64, H=16, W=48, T_=T, clamp=1e-7, clean=c.data_ptr(), enh=e.data_ptr(), bas=basis.data_ptr(), scratch=scr.data_ptr()):
        return lib.wunet_stft_forward(clean, enh, 2, T_, N, H, W, clamp, bas, scratch, saved.data_ptr(), None, None)

    for bad, word in ((dict(N=24), b"n_fft"), (dict(N=8), b"n_fft"), (dict(N=8192), b"n_fft"), (dict(H=0), b"hop"), (dict(H=65), b"hop"),
                      (dict(W=65), b"win_length"), (dict(W=0), b"win_length"), (dict(T_=32), b"reflect"), (dict(clamp=0.0), b"clamp"),
                      (dict(clamp=float("nan")), b"clamp"), (dict(enh=None), b"null"), (dict(bas=None), b"null"),
                      (dict(scratch=None), b"scratch")):
        assert fwd(**bad) == -1 and word in lib.wunet_last_error(), (bad, lib.wunet_last_error())
    assert not saved.any()                                                # nothing ran
    assert lib.wunet_stft_basis_bytes(24) == 0 and lib.wunet_stft_basis_bytes(320) == 320 * 2 * 192 * 4
    assert lib.wunet_stft_basis(64, 65, basis.data_ptr(), None) == -1 and lib.wunet_stft_scratch_bytes(2, 32, 64, 16, 0) == 0
    assert fwd() == 0 and saved.any()
    out, coefs = torch.zeros(()), torch.zeros(1, 4, dtype=torch.float64)
    tab = (ctypes.c_void_p * 1)(scr.data_ptr())
    n1, h1 = (ctypes.c_int * 1)(64), (ctypes.c_int * 1)(16)
    assert lib.wunet_stft_finalize(0, tab, 2, T, n1, h1, 1.0, 1.0, out.data_ptr(), coefs.data_ptr(), None) == -1
    assert lib.wunet_stft_finalize(9, tab, 2, T, n1, h1, 1.0, 1.0, out.data_ptr(), coefs.data_ptr(), None) == -1
    assert lib.wunet_stft_finalize(1, tab, 2, T, n1, h1, 1.0, 1.0, None, coefs.data_ptr(), None) == -1
    assert lib.wunet_stft_finalize(1, tab, 2, T, n1, h1, 1.0, 1.0, out.data_ptr(), coefs.data_ptr(), None) == 0 and float(out) > 0
    one, g = torch.ones(()), torch.zeros_like(e)
    args = [saved.data_ptr(), coefs.data_ptr(), one.data_ptr(), 2, T, 64, 16, 48, 1e-7, basis.data_ptr(), scr.data_ptr(), g.data_ptr(), 0, None]
    for k, v in ((0, None), (1, None), (2, None), (9, None), (10, None), (11, None), (5, 24), (6, 0), (7, 65), (4, 32), (8, 0.0)):
        a = list(args)
        a[k] = v
        assert lib.wunet_stft_backward(*a) == -1 and lib.wunet_last_error(), k
    assert not g.any() and lib.wunet_stft_backward(*args) == 0 and g.any()
    # the Python face: constraint violations in __init__, the rest when the waveform is seen
    for kw in (dict(fft_sizes=[24]), dict(hop_sizes=[0]), dict(win_lengths=[65]), dict(clamp=0.0), dict(clamp=-1.0)):
        full = dict(fft_sizes=[64], hop_sizes=[16], win_lengths=[48])
        full.update(kw)
        with pytest.raises(ValueError, match="stft"):
            loss_mod.stft_loss(**full)
    with pytest.raises(ValueError, match="equal lengths"):
        loss_mod.stft_loss(fft_sizes=[64, 128], hop_sizes=[16], win_lengths=[48, 128])
    crit = C.criterion(emu_engine, ((64, 16, 48),))
    with pytest.raises(RuntimeError, match="reflect"):
        crit(c[..., :32].contiguous(), e[..., :32].contiguous())
    with pytest.raises(RuntimeError, match="mismatch"):
        crit(c, e[:1])
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.clone().requires_grad_(True), e)
    with pytest.raises(RuntimeError, match="reflect"):
        metrics.stft_magnitude(e[..., :32].contiguous(), n_fft=64, hop=16, win_length=64, engine=emu_engine)
    with pytest.raises(ValueError, match="n_fft"):
        metrics.stft_magnitude(e, n_fft=24, engine=emu_engine)


def test_the_new_symbols_are_exported_and_public(pkg):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_stft_basis_bytes", "wunet_stft_basis", "wunet_stft_scratch_bytes", "wunet_stft_saved_bytes", "wunet_stft_forward",
                 "wunet_stft_finalize", "wunet_stft_backward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    for name in ("stft_loss", "weighted_loss", "stft_magnitude"):
        assert callable(getattr(pkg, name))
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_stft_loss.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.stft_loss()(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.stft_magnitude(torch.zeros(1, 1, 4096))
