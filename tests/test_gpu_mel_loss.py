"""-m gpu: the mel loss (mel_spec_kernel / mel_proj_kernel / mel_proj_bwd_kernel / mel_bwd_kernel of csrc/wunet_mel.h with
cspec_final_kernel and stft_ola_kernel, behind wunet_mel_*) on the MI355X: every case of tests/mel_loss_cases.py on device tensors
against the float64 oracle of tests/mel_loss_ref.py with the same bars as tests/test_mel_loss_emu.py (loss 4 d_ref + 2^-23, gradient
and mel spectrogram 4 d_ref, d_ref measured on the CPU at test time and printed beside every d), equal signals, an all-zero row,
determinism, inputs with 4-byte alignment only, weighted_loss, the ABI's refusals, one captured graph."""
import ctypes

import pytest
import torch

import mel_loss_cases as C
import mel_loss_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_loss_and_gradient_on_device_tensors(dev, name):
    C.check_case(name, None, dev)


@pytest.mark.parametrize("name", ("a", "c2", "f"))
def test_mel_spectrogram_on_device_tensors(dev, name):
    C.check_spectrogram(name, None, dev)


def test_two_runs_are_bit_identical_and_grad_loss_scales(dev):
    rows, T, res, n_mels, _ = C.CASES["d"]
    c, e = R.pair(rows, T)
    l1, g1 = C.run(None, dev, res, n_mels, c, e)
    l2, g2 = C.run(None, dev, res, n_mels, c, e)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _, gh = C.run(None, dev, res, n_mels, c, e, grad_loss=0.5)
    assert torch.equal(gh, 0.5 * g1)
    rows, T, res, n_mels, _ = C.CASES["a"]                               # one resolution: grad_loss multiplies each sample's sum once
    c, e = R.pair(rows, T)
    _, g1 = C.run(None, dev, res, n_mels, c, e)
    _, gs = C.run(None, dev, res, n_mels, c, e, grad_loss=2.5)
    assert torch.equal(gs, 2.5 * g1) and g1.any()
    crit = C.criterion(None, res, n_mels)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(c, e)
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.to(dev).requires_grad_(True), e.to(dev))


def test_equal_signals_and_an_all_zero_row(dev):
    """Equal signals: exactly 0.0 and an all-zero gradient (both signals run through the same instructions).  An all-zero enhanced
    row: its gradient row is exactly zero (the clamp passes nothing); the loss and the other rows against the oracle on this input."""
    rows, T, res, n_mels, _ = C.CASES["d"]
    c, _ = R.pair(rows, T)
    for kw in ({}, dict(power=2, lin_weight=1.0)):
        loss, g = C.run(None, dev, res, n_mels, c, c.clone(), **kw)
        assert float(loss) == 0.0 and not g.any(), kw
    rows, T, res, n_mels, _ = C.CASES["a"]
    c, e = R.pair(rows, T)
    e = e.clone()
    e[1] = 0.0
    loss, g = C.run(None, dev, res, n_mels, c, e)
    assert torch.isfinite(loss) and not g[1].any() and g[0].any() and g[2].any()
    l64, g64 = R.oracle64(c, e, res, n_mels)
    (l_r, g_r), (l_f, g_f) = R.restate32(c, e, res, n_mels), R.fft32(c, e, res, n_mels)
    ref = {"d_loss": max(R.d_loss(l_r, l64), R.d_loss(l_f, l64)), "d_grad": max(R.d_max(g_r, g64), R.d_max(g_f, g64))}
    bar_l, bar_g = R.bars(ref)
    dl, dg = R.d_loss(loss, l64), R.d_max(g, g64)
    print(f"zero row: loss d {dl:.2e} (bar {bar_l:.2e}), gradient d {dg:.2e} (bar {bar_g:.2e})")
    assert dl <= bar_l and dg <= bar_g


def test_inputs_with_4_byte_alignment_only(dev):
    """Case b with both inputs as views one float into their buffers: the same bars, and the same bits as the aligned run (the loaders
    read single floats of the waveforms, no path depends on their alignment)."""
    rows, T, res, n_mels, _ = C.CASES["b"]
    ref = R.case_reference(*C.CASES["b"])
    bc = torch.zeros(rows * T + 8, device=dev)
    be = torch.zeros(rows * T + 8, device=dev)
    bc[1:1 + rows * T] = ref["c"].reshape(-1).to(dev)
    be[1:1 + rows * T] = ref["e"].reshape(-1).to(dev)
    cv, ev = bc[1:1 + rows * T].view(rows, 1, T), be[1:1 + rows * T].view(rows, 1, T)
    assert cv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and cv.is_contiguous()
    loss, g = C.check_case("b", None, dev, c=cv, e=ev)
    la, ga = C.run(None, dev, res, n_mels, ref["c"], ref["e"])
    assert torch.equal(loss, la) and torch.equal(g, ga)


def test_weighted_loss_is_the_hand_written_sum(pkg, dev):
    rows, T, res, n_mels, _ = C.CASES["a"]
    c, e = R.pair(rows, T)
    c, e = c.to(dev), e.to(dev)
    args = {"fft_sizes": [64], "hop_sizes": [16], "win_lengths": [48], "n_mels": 8}
    crit = pkg.weighted_loss([["mel_loss", 0.5, args], ["l1_loss", 1.0]])
    l1, ml = pkg.l1_loss(), pkg.mel_loss(**args)
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 0.5 * ml(c, y) + 1.0 * l1(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad) and x.grad.any()


def test_the_abi_refuses_on_the_device_too(pkg, dev):
    """Null pointers, a misaligned filterbank, a wrong saved_bytes, n_mels = 0 and 129 through ctypes on device buffers: a code and a
    message, and nothing runs."""
    eng = pkg.engine.default_engine()
    lib = eng.lib
    c, e = (x.to(dev) for x in R.pair(2, 128))
    T = 128
    basis = eng.stft_basis(64, 48, dev)
    n_mels, filt = eng.mel_bank(dev, 16000, 64, 8)
    scr_bytes = lib.wunet_mel_scratch_bytes(2, T, 64, 16, 1)
    sv_bytes = lib.wunet_mel_saved_bytes(2, T, 64, 16, 8)
    other_sv = lib.wunet_mel_saved_bytes(2, T, 64, 16, 20)
    assert lib.wunet_mel_saved_bytes(2, T, 64, 16, 0) == 0 and lib.wunet_mel_saved_bytes(2, T, 64, 16, 129) == 0
    scr = torch.zeros(scr_bytes // 8, dtype=torch.float64, device=dev)
    saved = torch.zeros(sv_bytes // 4, device=dev)
    skew = torch.zeros(filt.numel() + 4, device=dev)
    skew[1:1 + filt.numel()] = filt.reshape(-1)
    assert skew[1:].data_ptr() % 16 == 4
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def fwd(nm=8, fl=filt.data_ptr(), clean=c.data_ptr(), enh=e.data_ptr(), bas=basis.data_ptr(), scratch=scr.data_ptr(), sv=saved.data_ptr(),
            svb=sv_bytes):
        return lib.wunet_mel_forward(clean, enh, 2, T, 64, 16, 48, nm, fl, 1, 1e-7, 1e-5, bas, scratch, scr_bytes, sv, svb, None, st)

    for bad, word in ((dict(enh=None), b"null"), (dict(bas=None), b"null"), (dict(fl=None), b"null"), (dict(scratch=None), b"scratch"),
                      (dict(fl=skew[1:].data_ptr()), b"aligned"), (dict(svb=other_sv), b"saved"), (dict(sv=None), b"saved"),
                      (dict(nm=0), b"n_mels"), (dict(nm=129), b"n_mels")):
        assert fwd(**bad) == -1 and word in lib.wunet_last_error(), (bad, lib.wunet_last_error())
    torch.cuda.synchronize()
    assert not saved.any()                                                # nothing ran
    assert fwd() == 0
    torch.cuda.synchronize()
    assert saved.any()


def test_a_captured_graph_replays_the_eager_result(dev):
    """Forward + backward of case a captured with plain torch.cuda.graph after one eager call (which builds the basis and uploads the
    filterbank), replayed twice: loss and gradient equal the eager ones bit for bit."""
    rows, T, res, n_mels, _ = C.CASES["a"]
    c, e = R.pair(rows, T)
    l_eager, g_eager = C.run(None, dev, res, n_mels, c, e)
    crit = C.criterion(None, res, n_mels)
    cs = c.to(dev)
    x = e.to(dev).requires_grad_(True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        crit(cs, x).backward()
    torch.cuda.current_stream(dev).wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(cs, x)
        loss.backward()
    for _ in range(2):
        loss.zero_()
        x.grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l_eager) and torch.equal(x.grad, g_eager)
