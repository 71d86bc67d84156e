"""-m "not gpu": the mel loss (mel_spec_kernel / mel_proj_kernel / mel_proj_bwd_kernel / mel_bwd_kernel of csrc/wunet_mel.h with
cspec_final_kernel and stft_ola_kernel, behind wunet_mel_*) on the CPU emulator, through the public modules (loss.mel_loss,
loss.weighted_loss, metrics.mel_spectrogram), and loss.mel_filterbank on the host.  No reference counterpart: the yardstick is the
definition in float64 on torch.stft under autograd with the test's own restatement of the filterbank (tests/mel_loss_ref.py); the bars
are multiples of the distance d_ref at which two float32 computations on the CPU land from it on the same inputs - loss 4 d_ref +
2^-23, gradient and mel spectrogram 4 d_ref - and every test prints its d and d_ref."""
import ctypes
import importlib
import warnings

import pytest
import torch

import emu_lib
import mel_loss_cases as C
import mel_loss_ref as R
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


@pytest.mark.parametrize("name", ("a", "f"))
def test_mel_spectrogram_matches_float64(emu_engine, name):
    C.check_spectrogram(name, emu_engine, CPU)


def test_equal_signals_give_exactly_zero_and_a_zero_gradient(emu_engine):
    rows, T, res, n_mels, _ = C.CASES["d"]
    c, _ = R.pair(rows, T)
    for kw in ({}, dict(power=2, lin_weight=1.0)):
        loss, g = C.run(emu_engine, CPU, res, n_mels, c, c.clone(), **kw)
        assert float(loss) == 0.0 and not g.any(), kw


def test_an_all_zero_enhanced_row_gets_an_exactly_zero_gradient(emu_engine):
    """Every bin of the row lies below the clamp, which passes nothing (and its mel cells sit on clamp^(1/2) sum Phi, a constant): the
    row's gradient is exactly zero.  The loss and the other rows' gradients against the oracle on this very input: the bars of
    mel_loss_ref.bars from the two float32 yardsticks on it (an exact zero spectrum cannot cross the clamp in any float32 computation,
    so the conditions hold for the row as they do for the others)."""
    rows, T, res, n_mels, _ = C.CASES["a"]
    c, e = R.pair(rows, T)
    e = e.clone()
    e[1] = 0.0
    loss, g = C.run(emu_engine, CPU, res, n_mels, c, e)
    assert torch.isfinite(loss) and not g[1].any() and g[0].any() and g[2].any()
    l64, g64 = R.oracle64(c, e, res, n_mels)
    assert not g64[1].any()
    (l_r, g_r), (l_f, g_f) = R.restate32(c, e, res, n_mels), R.fft32(c, e, res, n_mels)
    ref = {"d_loss": max(R.d_loss(l_r, l64), R.d_loss(l_f, l64)), "d_grad": max(R.d_max(g_r, g64), R.d_max(g_f, g64))}
    bar_l, bar_g = R.bars(ref)
    dl, dg = R.d_loss(loss, l64), R.d_max(g, g64)
    print(f"zero row: loss d {dl:.2e} (bar {bar_l:.2e}), gradient d {dg:.2e} (bar {bar_g:.2e})")
    assert dl <= bar_l and dg <= bar_g


def test_grad_loss_scales_and_two_runs_are_bit_identical(emu_engine):
    rows, T, res, n_mels, _ = C.CASES["d"]
    c, e = R.pair(rows, T)
    l1, g1 = C.run(emu_engine, CPU, res, n_mels, c, e)
    l2, g2 = C.run(emu_engine, CPU, res, n_mels, c, e)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _, gh = C.run(emu_engine, CPU, res, n_mels, c, e, grad_loss=0.5)
    assert torch.equal(gh, 0.5 * g1)                                     # a power of two: exact, through every resolution's accumulation
    rows, T, res, n_mels, _ = C.CASES["a"]                               # one resolution: grad_loss multiplies each sample's sum once,
    c, e = R.pair(rows, T)                                               # so any factor scales to the bits of the same product
    _, g1 = C.run(emu_engine, CPU, res, n_mels, c, e)
    _, gs = C.run(emu_engine, CPU, res, n_mels, c, e, grad_loss=2.5)
    assert torch.equal(gs, 2.5 * g1) and g1.any()


def test_inputs_with_4_byte_alignment_only(emu_engine):
    """Case b with both inputs as views one float into their buffers: the same bars, and the same bits as the aligned run."""
    rows, T, res, n_mels, _ = C.CASES["b"]
    ref = R.case_reference(*C.CASES["b"])
    bc, be = torch.zeros(rows * T + 8), torch.zeros(rows * T + 8)
    off = 1 + (-(bc.data_ptr() // 4) % 4)                               # the first float at an address that is 4 mod 16
    off_e = 1 + (-(be.data_ptr() // 4) % 4)
    bc[off:off + rows * T] = ref["c"].reshape(-1)
    be[off_e:off_e + rows * T] = ref["e"].reshape(-1)
    cv, ev = bc[off:off + rows * T].view(rows, 1, T), be[off_e:off_e + rows * T].view(rows, 1, T)
    assert cv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and cv.is_contiguous()
    loss, g = C.check_case("b", emu_engine, CPU, c=cv, e=ev)
    la, ga = C.run(emu_engine, CPU, res, n_mels, ref["c"], ref["e"])
    assert torch.equal(loss, la) and torch.equal(g, ga)


def test_weighted_loss_is_the_hand_written_sum(emu_engine):
    loss_mod, _ = C.mods()
    rows, T, res, n_mels, _ = C.CASES["a"]
    c, e = R.pair(rows, T)
    args = {"fft_sizes": [64], "hop_sizes": [16], "win_lengths": [48], "n_mels": 8}
    crit = loss_mod.weighted_loss([["mel_loss", 0.5, args], ["l1_loss", 1.0]])
    l1, ml = loss_mod.l1_loss(), loss_mod.mel_loss(**args)
    for m in list(crit.terms) + [l1, ml]:
        m._engine_override = emu_engine
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 0.5 * ml(c, y) + 1.0 * l1(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = C.run(emu_engine, CPU, res, n_mels, c, e)
    assert (x.grad - 0.5 * gs).abs().max() > 0                           # ... and the l1 term is in it
    assert "mel_loss" in loss_mod._SPECTRAL_FACTORIES and "mel_loss" not in loss_mod._FACTORIES
    with pytest.raises(ValueError, match="unknown loss.*mel_loss"):
        loss_mod.weighted_loss([["nope", 1.0]])


# ---------------------------------------------------------------------------------------------------------- loss.mel_filterbank (host only)
BANKS = ((16000, 512, 80, {}), (16000, 128, 20, {}), (16000, 320, 40, dict(mel_scale="htk", norm=None, fmin=50.0, fmax=7000.0)),
         (8000, 320, 40, {}), (16000, 2048, 128, {}), (22050, 1024, 64, dict(mel_scale="htk")), (16000, 256, 40, dict(norm=None)))


@pytest.mark.parametrize("sr,n_fft,n_mels,kw", BANKS)
def test_filterbank_matches_the_restatement_to_float32_rounding(sr, n_fft, n_mels, kw):
    loss_mod, _ = C.mods()
    fb = loss_mod.mel_filterbank(sr, n_fft, n_mels, **kw)
    assert fb.shape == (n_mels, n_fft // 2 + 1) and fb.dtype == torch.float32 and fb.device.type == "cpu" and (fb >= 0).all()
    ref = R.filterbank64(sr, n_fft, n_mels, **kw)
    # float32 rounding of the cell (2^-24 relative) and the two float64 computations' own difference: a triangle's value is a quotient
    # of differences of p, whose last-place errors (2^-52 of ~1e4 Hz) over a width of a few Hz stay below 1e-12 of the peak
    err = (fb.double() - ref).abs()
    assert (err <= 2.0 ** -24 * ref.abs() + 1e-12 * ref.max()).all(), float(err.max())


def test_filterbank_partition_of_unity_peaks_and_warning():
    loss_mod, _ = C.mods()
    for sr, n_fft, n_mels, scale in ((16000, 512, 40, "slaney"), (16000, 1024, 64, "htk")):
        fb = loss_mod.mel_filterbank(sr, n_fft, n_mels, norm=None, mel_scale=scale).double()
        p = R.mel_points(sr, n_mels, 0.0, None, scale)
        f = torch.arange(n_fft // 2 + 1, dtype=torch.float64) * sr / n_fft
        inside = (f >= p[1]) & (f <= p[n_mels])
        assert inside.sum() > n_mels and ((fb.sum(dim=0)[inside] - 1.0).abs() <= 1e-6).all()      # neighbouring triangles sum to 1
        for j in range(n_mels):                          # a triangle rises up to its centre and falls behind it: its largest bin is one of the
            width = min(p[j + 1] - p[j], p[j + 2] - p[j + 1])                                      # two next to the centre frequency
            if width >= sr / n_fft:                                                                # (where both of them lie under it)
                assert abs(float(f[fb[j].argmax()]) - p[j + 1]) < sr / n_fft, (scale, j)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        loss_mod.mel_filterbank(16000, 512, 40)                          # no empty filter: no warning
    with pytest.warns(UserWarning, match="1 of 48 filters"):
        fb = loss_mod.mel_filterbank(16000, 128, 48)
    assert int((fb.max(dim=1).values == 0).sum()) == 1
    with pytest.warns(UserWarning, match="filters"):
        loss_mod.mel_loss(fft_sizes=[128], hop_sizes=[50], win_lengths=[128], n_mels=48)


def test_the_constructor_and_the_module_refuse_what_the_library_would(emu_engine):
    loss_mod, metrics = C.mods()
    c, e = R.pair(2, 128)
    for kw in (dict(fft_sizes=[24]), dict(hop_sizes=[0]), dict(win_lengths=[65]), dict(n_mels=0), dict(n_mels=129), dict(n_mels=[8, 8]),
               dict(n_mels=[]), dict(fmin=-1.0), dict(fmin=4000.0, fmax=4000.0), dict(fmin=5000.0, fmax=4000.0), dict(fmax=8000.5),
               dict(sample_rate=8000, fmax=4001.0), dict(power=0), dict(power=3), dict(power=1.5), dict(log_weight=-1.0),
               dict(lin_weight=-0.5), dict(log_weight=float("nan")), dict(lin_weight=float("inf")), dict(log_weight=0.0, lin_weight=0.0),
               dict(clamp=0.0), dict(clamp=-1.0), dict(clamp=float("inf")), dict(floor=0.0), dict(floor=float("nan")),
               dict(mel_scale="bark"), dict(norm="l2")):
        full = dict(fft_sizes=[64], hop_sizes=[16], win_lengths=[48], n_mels=8)
        full.update(kw)
        with pytest.raises(ValueError):
            loss_mod.mel_loss(**full)
    with pytest.raises(ValueError, match="equal lengths"):
        loss_mod.mel_loss(fft_sizes=[64, 128], hop_sizes=[16], win_lengths=[48, 128])
    with pytest.raises(ValueError, match="resolutions"):
        loss_mod.mel_loss(fft_sizes=[64] * 9, hop_sizes=[16] * 9, win_lengths=[48] * 9, n_mels=8)
    crit = C.criterion(emu_engine, ((64, 16, 48),), (8,))
    with pytest.raises(RuntimeError, match="reflect"):
        crit(c[..., :32].contiguous(), e[..., :32].contiguous())
    with pytest.raises(RuntimeError, match="mismatch"):
        crit(c, e[:1])
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.clone().requires_grad_(True), e)
    with pytest.raises(ValueError, match="power"):
        metrics.mel_spectrogram(e, n_fft=64, hop=16, win_length=48, n_mels=8, power=3, engine=emu_engine)
    with pytest.raises(ValueError, match="floor"):
        metrics.mel_spectrogram(e, n_fft=64, hop=16, win_length=48, n_mels=8, log=True, floor=0.0, engine=emu_engine)
    d = loss_mod.mel_loss()
    assert d.resolutions == ((512, 128, 512), (1024, 256, 1024), (2048, 512, 2048)) and d.n_mels == (40, 80, 128)
    assert (d.power, d.log_weight, d.lin_weight, d.clamp, d.floor, d.sample_rate) == (1, 1.0, 0.0, 1e-7, 1e-5, 16000.0)
    assert loss_mod.mel_loss(fft_sizes=[64, 128], hop_sizes=[16, 32], win_lengths=[64, 128], n_mels=8).n_mels == (8, 8)


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    c, e = R.pair(2, 128)
    T, M, BP, MP = 128, 2 * (1 + 128 // 16), 64, 16
    basis = emu_engine.stft_basis(64, 48, CPU)
    n_mels, filt = emu_engine.mel_bank(CPU, 16000, 64, 8)
    assert n_mels == 8 and filt.shape == (8, BP) and not filt[:, 33:].any()
    scr_bytes = lib.wunet_mel_scratch_bytes(2, T, 64, 16, 1)
    fwd_bytes = lib.wunet_mel_scratch_bytes(2, T, 64, 16, 0)
    sv_bytes = lib.wunet_mel_saved_bytes(2, T, 64, 16, 8)
    assert sv_bytes == (3 * BP + 2 * MP) * M * 4 and fwd_bytes == (M + 15) // 16 * 2 * 8 + 2 * M * BP * 4 and scr_bytes == max(fwd_bytes, M * 64 * 4)
    assert lib.wunet_mel_scratch_bytes(2, 32, 64, 16, 0) == 0 and b"reflect" in lib.wunet_last_error()
    assert lib.wunet_mel_saved_bytes(2, T, 24, 16, 8) == 0 and b"n_fft" in lib.wunet_last_error()
    assert lib.wunet_mel_saved_bytes(2, T, 64, 16, 0) == 0 and b"n_mels" in lib.wunet_last_error()
    assert lib.wunet_mel_saved_bytes(2, T, 64, 16, 129) == 0 and b"n_mels" in lib.wunet_last_error()
    other_sv = lib.wunet_mel_saved_bytes(2, T, 64, 16, 20)               # the buffer of another bank on the same waveforms
    small_scr = lib.wunet_mel_scratch_bytes(2, T, 32, 16, 0)
    assert other_sv != sv_bytes and 0 < small_scr < fwd_bytes
    scr = torch.zeros(scr_bytes // 8 + 2, dtype=torch.float64)
    saved = torch.zeros(sv_bytes // 4 + 4)
    skew = torch.zeros(8 * BP + 4)                                        # the filterbank at an address that is 4 mod 16
    off = 1 + (-(skew.data_ptr() // 4) % 4)
    skew[off:off + 8 * BP] = filt.reshape(-1)
    assert skew[off:].data_ptr() % 16 == 4

    def fwd(N=64, H=16, W=48, T_=T, nm=8, fl=filt.data_ptr(), power=1, clamp=1e-7, floor=1e-5, clean=c.data_ptr(), enh=e.data_ptr(),
            bas=basis.data_ptr(), scratch=scr.data_ptr(), sb=scr_bytes, sv=saved.data_ptr(), svb=sv_bytes, out=None):
        return lib.wunet_mel_forward(clean, enh, 2, T_, N, H, W, nm, fl, power, clamp, floor, bas, scratch, sb, sv, svb, out, None)

    spec_out = torch.zeros(M, 8)
    for bad, word in ((dict(N=24), b"n_fft"), (dict(N=8192), b"n_fft"), (dict(H=0), b"hop"), (dict(H=65), b"hop"),
                      (dict(W=65), b"win_length"), (dict(W=0), b"win_length"), (dict(T_=32), b"reflect"),
                      (dict(nm=0), b"n_mels"), (dict(nm=129), b"n_mels"), (dict(power=0), b"power"), (dict(power=3), b"power"),
                      (dict(clamp=0.0), b"clamp"), (dict(clamp=-1.0), b"clamp"), (dict(clamp=float("nan")), b"clamp"),
                      (dict(floor=0.0), b"floor"), (dict(floor=float("inf")), b"floor"),
                      (dict(enh=None), b"null"), (dict(bas=None), b"null"), (dict(fl=None), b"null"),
                      (dict(fl=skew[off:].data_ptr()), b"aligned"),
                      (dict(scratch=None), b"scratch"), (dict(sb=small_scr), b"scratch"), (dict(svb=other_sv), b"saved"),
                      (dict(sv=None), b"saved"), (dict(out=spec_out.data_ptr()), b"mel_out"),
                      (dict(clean=None), b"without"), (dict(clean=None, sv=None, svb=0, clamp=-1.0, out=spec_out.data_ptr()), b"clamp")):
        assert fwd(**bad) == -1 and word in lib.wunet_last_error(), (bad, lib.wunet_last_error())
    assert not saved.any() and not spec_out.any()                        # nothing ran
    assert fwd() == 0 and saved.any()
    assert fwd(clean=None, sv=None, svb=0, clamp=0.0, floor=0.0, out=spec_out.data_ptr()) == 0 and (spec_out > 0).all()
    out, coefs = torch.zeros(()), torch.zeros(1, 4, dtype=torch.float64)
    tab = (ctypes.c_void_p * 1)(scr.data_ptr())
    n1, h1, m1 = (ctypes.c_int * 1)(64), (ctypes.c_int * 1)(16), (ctypes.c_int * 1)(8)

    def fin(n_res=1, lw=1.0, nw=0.5, lo=out.data_ptr(), mels=m1):
        return lib.wunet_mel_finalize(n_res, tab, 2, T, n1, h1, mels, lw, nw, lo, coefs.data_ptr(), None)

    for bad, word in ((dict(n_res=0), b"resolutions"), (dict(n_res=9), b"resolutions"), (dict(lo=None), b"null"), (dict(mels=None), b"null"),
                      (dict(lw=-0.1), b"weight"), (dict(nw=float("nan")), b"weight"), (dict(lw=float("inf")), b"weight"),
                      (dict(lw=0.0, nw=0.0), b"weight"), (dict(mels=(ctypes.c_int * 1)(0)), b"n_mels"),
                      (dict(mels=(ctypes.c_int * 1)(129)), b"n_mels")):
        assert fin(**bad) == -1 and word in lib.wunet_last_error(), (bad, lib.wunet_last_error())
    assert fin() == 0 and float(out) > 0
    count = M * 8
    assert coefs[0, 0] == 1.0 / count and coefs[0, 1] == 0.5 / count
    assert abs(float(1.0 * coefs[0, 2] + 0.5 * coefs[0, 3]) - float(out)) <= 2.0 ** -23 * float(out)
    one, g = torch.ones(()), torch.zeros_like(e)
    args = [saved.data_ptr(), sv_bytes, coefs.data_ptr(), one.data_ptr(), 2, T, 64, 16, 48, 8, filt.data_ptr(), 1, 1e-7, 1e-5,
            basis.data_ptr(), scr.data_ptr(), scr_bytes, g.data_ptr(), 0, None]
    for k, v, word in ((0, None, b"null"), (2, None, b"null"), (3, None, b"null"), (10, None, b"null"), (14, None, b"null"),
                       (17, None, b"null"), (10, skew[off:].data_ptr(), b"aligned"), (15, None, b"scratch"), (16, 16, b"scratch"),
                       (1, other_sv, b"saved"), (6, 24, b"n_fft"), (7, 0, b"hop"), (8, 65, b"win_length"), (5, 32, b"reflect"),
                       (9, 0, b"n_mels"), (9, 129, b"n_mels"), (11, 3, b"power"), (12, 0.0, b"clamp"), (13, 0.0, b"floor")):
        a = list(args)
        a[k] = v
        assert lib.wunet_mel_backward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not g.any() and lib.wunet_mel_backward(*args) == 0 and g.any()


def test_the_new_symbols_are_exported_and_public(pkg):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_mel_scratch_bytes", "wunet_mel_saved_bytes", "wunet_mel_forward", "wunet_mel_finalize", "wunet_mel_backward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    assert callable(pkg.mel_loss) and isinstance(pkg.mel_loss(), pkg.HipMelLoss) and callable(pkg.mel_spectrogram)
    assert callable(pkg.mel_filterbank)
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_mel_loss.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.mel_loss()(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096))


# ------------------------------------------------------------------------------- the reference's train.py with the loss named by config string
_MEL_ARGS = {"fft_sizes": [64], "hop_sizes": [16], "win_lengths": [48], "n_mels": 8}


def _bound_to_the_emulator(crit):
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    engine = eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)
    for m in crit.modules():
        if hasattr(m, "_engine_override"):
            m._engine_override = engine
    return crit


def emu_mel_loss(**kw):
    """`loss.mel_loss` as a config names it, bound to the CPU emulator engine (the product path has no CPU fallback)."""
    return _bound_to_the_emulator(C.mods()[0].mel_loss(**kw))


def emu_weighted_loss(terms):
    return _bound_to_the_emulator(C.mods()[0].weighted_loss(terms))


@pytest.mark.parametrize("main,args", (("emu_mel_loss", _MEL_ARGS), ("emu_weighted_loss", {"terms": [["l1_loss", 1.0], ["mel_loss", 0.5, _MEL_ARGS]]})))
def test_reference_train_py_runs_an_epoch_with_the_loss_named_by_config(tmp_path, main, args):
    """train.py:main as tests/test_reference_loader.py restates it, one epoch of its config with `loss_function` naming the mel loss
    (alone, and as a weighted_loss term) by module / main / args: the epoch runs, the checkpoint is written, and the weights are those
    of the same two steps written out with the loss built by hand."""
    import numpy as np
    import emu_plugins
    import test_reference_loader as L
    cfg = L.main_config(tmp_path)
    cfg["loss_function"] = {"module": __name__, "main": main, "args": args}
    L.reference_main(cfg, resume=False)
    ck = torch.load((tmp_path / "ref_main" / "checkpoints" / "latest_model.tar").as_posix())
    assert ck["epoch"] == 1
    torch.manual_seed(0)
    np.random.seed(0)
    ds = importlib.import_module(PKG_NAME + ".dataset").Dataset(n_items=6, sample_length=64, seed=1)
    m = emu_plugins.Model(n_layers=2, channels_interval=4)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.Adam(params=m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    crit = emu_mel_loss(**args) if main == "emu_mel_loss" else emu_weighted_loss(**args)
    m.train()
    for mix, cl, _ in torch.utils.data.DataLoader(ds, batch_size=3, shuffle=False):
        opt.zero_grad()
        loss = crit(cl, m(mix))
        assert torch.isfinite(loss) and float(loss.detach()) > 0
        loss.backward()
        opt.step()
    for k, v in m.state_dict().items():
        assert torch.equal(v, ck["model"][k]), k
    assert any(not torch.equal(v, start[k]) for k, v in m.state_dict().items() if v.dtype == torch.float32)
