"""-m "not gpu": the compressed spectral loss (cspec_fwd_kernel / cspec_final_kernel / cspec_bwd_kernel of csrc/wunet_cspec.h and
stft_ola_kernel, behind wunet_cspec_*) on the CPU emulator, through the public modules (loss.compressed_spectral_loss,
loss.weighted_loss).  No reference counterpart: the yardstick is the definition in float64 on torch.stft under autograd
(tests/cspec_loss_ref.py); the bars are multiples of the distance d_ref at which two float32 computations on the CPU land from it on
the same inputs - loss 4 d_ref + 2^-23, gradient 4 d_ref - and every test prints its d and d_ref."""
import ctypes
import importlib

import pytest
import torch

import cspec_loss_cases as C
import cspec_loss_ref as R
import emu_lib
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("name,compress,complex_weight", C.params(C.EMU_CASES))
def test_loss_and_gradient_match_the_float64_oracle(emu_engine, name, compress, complex_weight):
    C.check_case(name, compress, complex_weight, emu_engine, CPU)


def test_equal_signals_give_exactly_zero_and_a_zero_gradient(emu_engine):
    rows, T, res = C.CASES["d"]
    c, _ = R.pair(rows, T)
    for knobs in (C.DEFAULT,) + C.EXTRA:
        loss, g = C.run(emu_engine, CPU, res, c, c.clone(), compress=knobs[0], complex_weight=knobs[1])
        assert float(loss) == 0.0 and not g.any(), knobs


def test_an_all_zero_enhanced_row_gets_a_finite_non_zero_gradient(emu_engine):
    """Below the clamp the compression factors are constants and Z_e stays linear in (re, im): the complex term pulls a silent row
    towards the clean one.  The row's gradient against the oracle's: 4 d_ref of the two float32 yardsticks on this very input (an
    exact zero spectrum cannot cross the clamp in any float32 computation, so the bar needs no condition on the row)."""
    rows, T, res = C.CASES["a"]
    c, e = R.pair(rows, T)
    e = e.clone()
    e[1] = 0.0
    loss, g = C.run(emu_engine, CPU, res, c, e)
    assert torch.isfinite(loss) and torch.isfinite(g).all()
    assert g[1].any() and g[0].any() and g[2].any()
    l64, g64 = R.oracle64(c, e, res)
    d_ref = max(R.d_max(R.restate32(c, e, res)[1][1], g64[1]), R.d_max(R.fft32(c, e, res)[1][1], g64[1]))
    d = R.d_max(g[1], g64[1])
    print(f"zero row: gradient d {d:.2e} (d_ref {d_ref:.2e}, bar {4.0 * d_ref:.2e})")
    assert g64[1].any() and d <= 4.0 * d_ref
    # magnitude only: the row's bins sit below the clamp and A_e passes nothing
    _, g0 = C.run(emu_engine, CPU, res, c, e, compress=0.5, complex_weight=0.0)
    assert not g0[1].any() and g0[0].any()


def test_grad_loss_scales_exactly_and_two_runs_are_bit_identical(emu_engine):
    rows, T, res = C.CASES["d"]
    c, e = R.pair(rows, T)
    l1, g1 = C.run(emu_engine, CPU, res, c, e)
    l2, g2 = C.run(emu_engine, CPU, res, c, e)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _, gh = C.run(emu_engine, CPU, res, c, e, grad_loss=0.5)
    assert torch.equal(gh, 0.5 * g1)                                     # a power of two: exact, through every resolution's accumulation


def test_weighted_loss_is_the_hand_written_sum(emu_engine):
    loss_mod = C.loss_mod()
    rows, T, res = C.CASES["a"]
    c, e = R.pair(rows, T)
    args = {"fft_sizes": [64], "hop_sizes": [16], "win_lengths": [48], "compress": 0.3, "complex_weight": 0.3}
    crit = loss_mod.weighted_loss([["l1_loss", 1.0], ["compressed_spectral_loss", 0.5, args]])
    l1, cs = loss_mod.l1_loss(), loss_mod.compressed_spectral_loss(**args)
    for m in list(crit.terms) + [l1, cs]:
        m._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 1.0 * l1(c, y) + 0.5 * cs(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = C.run(emu_engine, CPU, res, c, e)
    assert (x.grad - 0.5 * gs).abs().max() > 0                           # ... and the l1 term is in it
    with pytest.raises(ValueError, match="unknown loss.*compressed_spectral_loss.*stft_loss"):
        loss_mod.weighted_loss([["nope", 1.0]])


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    c, e = R.pair(2, 128)
    T = 128
    basis = emu_engine.stft_basis(64, 48, CPU)
    scr_bytes = lib.wunet_cspec_scratch_bytes(2, T, 64, 16, 1)
    fwd_bytes = lib.wunet_cspec_scratch_bytes(2, T, 64, 16, 0)
    sv_bytes = lib.wunet_cspec_saved_bytes(2, T, 64, 16)
    assert sv_bytes == 5 * 2 * (1 + T // 16) * 64 * 4 and fwd_bytes == 2 * 2 * 8 and scr_bytes == 2 * (1 + T // 16) * 64 * 4
    assert lib.wunet_cspec_scratch_bytes(2, 32, 64, 16, 0) == 0 and b"reflect" in lib.wunet_last_error()
    assert lib.wunet_cspec_saved_bytes(2, T, 24, 16) == 0 and b"n_fft" in lib.wunet_last_error()
    other_sv = lib.wunet_cspec_saved_bytes(2, T, 128, 16)                # the buffers of other resolutions on the same waveforms
    small_scr = lib.wunet_cspec_scratch_bytes(2, T, 32, 16, 0)
    assert other_sv != sv_bytes and 0 < small_scr < fwd_bytes
    scr = torch.zeros(scr_bytes // 8 + 1, dtype=torch.float64)
    saved = torch.zeros(sv_bytes // 4)

    def fwd(N=64, H=16, W=48, T_=T, compress=0.3, clamp=1e-7, clean=c.data_ptr(), enh=e.data_ptr(), bas=basis.data_ptr(),
            scratch=scr.data_ptr(), sb=scr_bytes, sv=saved.data_ptr(), svb=sv_bytes):
        return lib.wunet_cspec_forward(clean, enh, 2, T_, N, H, W, compress, clamp, bas, scratch, sb, sv, svb, None)

    for bad, word in ((dict(N=24), b"n_fft"), (dict(N=8), b"n_fft"), (dict(N=8192), b"n_fft"), (dict(H=0), b"hop"), (dict(H=65), b"hop"),
                      (dict(W=65), b"win_length"), (dict(W=0), b"win_length"), (dict(T_=32), b"reflect"),
                      (dict(compress=0.0), b"compress"), (dict(compress=1.5), b"compress"), (dict(compress=float("nan")), b"compress"),
                      (dict(clamp=0.0), b"clamp"), (dict(clamp=-1.0), b"clamp"), (dict(clamp=float("nan")), b"clamp"),
                      (dict(clean=None), b"null"), (dict(enh=None), b"null"), (dict(bas=None), b"null"),
                      (dict(scratch=None), b"scratch"), (dict(sb=small_scr), b"scratch"), (dict(svb=other_sv), b"saved"),
                      (dict(sv=None), b"saved")):
        assert fwd(**bad) == -1 and word in lib.wunet_last_error(), (bad, lib.wunet_last_error())
    assert not saved.any()                                                # nothing ran
    assert fwd() == 0 and saved.any()
    out, coefs = torch.zeros(()), torch.zeros(1, 4, dtype=torch.float64)
    tab = (ctypes.c_void_p * 1)(scr.data_ptr())
    n1, h1 = (ctypes.c_int * 1)(64), (ctypes.c_int * 1)(16)
    for n_res, lam, lo, word in ((0, 0.3, out.data_ptr(), b"resolutions"), (9, 0.3, out.data_ptr(), b"resolutions"),
                                 (1, 0.3, None, b"null"), (1, -0.1, out.data_ptr(), b"complex_weight"),
                                 (1, 1.5, out.data_ptr(), b"complex_weight"), (1, float("nan"), out.data_ptr(), b"complex_weight")):
        assert lib.wunet_cspec_finalize(n_res, tab, 2, T, n1, h1, lam, lo, coefs.data_ptr(), None) == -1
        assert word in lib.wunet_last_error(), (n_res, lam, lib.wunet_last_error())
    assert lib.wunet_cspec_finalize(1, tab, 2, T, n1, h1, 0.3, out.data_ptr(), coefs.data_ptr(), None) == 0 and float(out) > 0
    count = 2 * (1 + T // 16) * 33
    assert coefs[0, 0] == (1.0 - 0.3) / count and coefs[0, 1] == 0.3 / count
    assert abs(float(0.7 * coefs[0, 2] + 0.3 * coefs[0, 3]) - float(out)) <= 2.0 ** -23 * float(out)
    one, g = torch.ones(()), torch.zeros_like(e)
    args = [saved.data_ptr(), sv_bytes, coefs.data_ptr(), one.data_ptr(), 2, T, 64, 16, 48, 0.3, 1e-7, basis.data_ptr(), scr.data_ptr(),
            scr_bytes, g.data_ptr(), 0, None]
    for k, v, word in ((0, None, b"null"), (2, None, b"null"), (3, None, b"null"), (11, None, b"null"), (14, None, b"null"),
                       (12, None, b"scratch"), (13, fwd_bytes, b"scratch"), (1, other_sv, b"saved"), (6, 24, b"n_fft"), (7, 0, b"hop"),
                       (8, 65, b"win_length"), (5, 32, b"reflect"), (9, 0.0, b"compress"), (9, 1.01, b"compress"), (10, 0.0, b"clamp")):
        a = list(args)
        a[k] = v
        assert lib.wunet_cspec_backward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not g.any() and lib.wunet_cspec_backward(*args) == 0 and g.any()


def test_the_constructor_and_the_module_refuse_what_the_library_would(emu_engine):
    loss_mod = C.loss_mod()
    c, e = R.pair(2, 128)
    for kw in (dict(fft_sizes=[24]), dict(hop_sizes=[0]), dict(win_lengths=[65]), dict(clamp=0.0), dict(clamp=-1.0),
               dict(clamp=float("inf")), dict(compress=0.0), dict(compress=1.5), dict(compress=float("nan")), dict(complex_weight=-0.1),
               dict(complex_weight=1.5), dict(complex_weight=float("nan"))):
        full = dict(fft_sizes=[64], hop_sizes=[16], win_lengths=[48])
        full.update(kw)
        with pytest.raises(ValueError):
            loss_mod.compressed_spectral_loss(**full)
    with pytest.raises(ValueError, match="equal lengths"):
        loss_mod.compressed_spectral_loss(fft_sizes=[64, 128], hop_sizes=[16], win_lengths=[48, 128])
    with pytest.raises(ValueError, match="resolutions"):
        loss_mod.compressed_spectral_loss(fft_sizes=[64] * 9, hop_sizes=[16] * 9, win_lengths=[48] * 9)
    crit = C.criterion(emu_engine, ((64, 16, 48),))
    with pytest.raises(RuntimeError, match="reflect"):
        crit(c[..., :32].contiguous(), e[..., :32].contiguous())
    with pytest.raises(RuntimeError, match="mismatch"):
        crit(c, e[:1])
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.clone().requires_grad_(True), e)
    d = loss_mod.compressed_spectral_loss()
    assert d.resolutions == ((512, 128, 512),) and (d.compress, d.complex_weight, d.clamp) == (0.3, 0.3, 1e-7)


def test_the_new_symbols_are_exported_and_public(pkg):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    loss_mod = C.loss_mod()
    for name in ("wunet_cspec_scratch_bytes", "wunet_cspec_saved_bytes", "wunet_cspec_forward", "wunet_cspec_finalize",
                 "wunet_cspec_backward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    assert callable(pkg.compressed_spectral_loss) and isinstance(pkg.compressed_spectral_loss(), pkg.HipCompressedSpectralLoss)
    assert "compressed_spectral_loss" not in loss_mod._FACTORIES and "compressed_spectral_loss" in loss_mod._SPECTRAL_FACTORIES
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_cspec_loss.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.compressed_spectral_loss()(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096))
