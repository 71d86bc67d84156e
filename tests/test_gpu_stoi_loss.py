"""-m gpu: the STOI loss (stoi_spec_kernel<save> / stoi_loss_final_kernel / stoi_segment_bwd_kernel / stoi_spec_bwd_kernel /
stoi_unframe_kernel / stoi_resample_bwd_kernel behind wunet_stoi_loss_*) on the MI355X: the six cases of tests/stoi_cases.py on device
tensors against the float64 autograd gradient of tests/stoi_loss_ref.py with the conditions and bars of tests/stoi_loss_cases.py
(d_ref measured on the CPU at test time and printed beside every d), determinism, inputs and gradient with 4-byte alignment only, one
captured graph of forward + backward, leading dimensions, the weighted sum.  Measured d_ref of the gradient per case (fft / matmul
yardstick) and the kernels' d are recorded in tests/stoi_loss_cases.py."""
import pytest
import torch

import stoi_loss_cases as LC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_loss_and_gradient_on_device_tensors(dev, name):
    LC.check_case(name, None, dev)


def test_two_runs_are_bit_identical_and_cpu_tensors_are_refused(dev):
    l1, g1 = LC.run(None, dev, "d")
    l2, g2 = LC.run(None, dev, "d")
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and g1.abs().max() > 0
    lh, gh = LC.run(None, dev, "d", grad_loss=0.5)
    assert torch.equal(lh, l1) and torch.equal(gh, 0.5 * g1)
    ref = LC.reference("d")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LC.make(None, 16000)(ref["c"], ref["e"])


@pytest.mark.parametrize("name", ("a", "b"))
def test_inputs_and_gradient_with_4_byte_alignment_only(dev, name):
    """Both inputs as views one float into their buffers, and the gradient handed on into such a view (case a: the spectrum's loader
    and the frame gather touch them; case b: the resampler and its adjoint do): the same checks, and the same bits as the aligned run."""
    rows, T = LC.CASES[name][:2]
    ref = LC.reference(name)
    bc = torch.zeros(rows * T + 8, device=dev)
    be = torch.zeros(rows * T + 8, device=dev)
    bc[1:1 + rows * T] = ref["c"].reshape(-1).to(dev)
    be[1:1 + rows * T] = ref["e"].reshape(-1).to(dev)
    cv, ev = bc[1:1 + rows * T].view(rows, T), be[1:1 + rows * T].view(rows, T)
    assert cv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and cv.is_contiguous()
    loss, g = LC.check_case(name, None, dev, c=cv, e=ev)
    la, ga = LC.run(None, dev, name)
    assert torch.equal(loss, la) and torch.equal(g, ga)
    # the gradient buffer itself at 4-byte alignment: the engine's backward writing into a view one float into a buffer
    engine = LC.loss_mod().default_engine()
    _, saved, _ = engine.stoi_loss_forward(cv, ev, LC.CASES[name][2])
    lib = engine.lib
    fs = LC.CASES[name][2]
    gb = torch.full((rows * T + 8,), 7.0, device=dev)
    gv = gb[1:1 + rows * T]
    assert gv.data_ptr() % 16 == 4
    scr = torch.empty(lib.wunet_stoi_loss_scratch_bytes(rows, T, fs) // 8, dtype=torch.float64, device=dev)
    one = torch.ones((), device=dev)
    rc = lib.wunet_stoi_loss_backward(saved.data_ptr(), one.data_ptr(), rows, T, fs, engine.stoi_tables(fs, dev).data_ptr(), scr.data_ptr(),
                                      gv.data_ptr(), engine._stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(gv.view(rows, T), ga) and gb[0] == 7.0 and (gb[1 + rows * T:] == 7.0).all()


def test_a_captured_graph_replays_the_eager_result(dev):
    """Forward + backward of case d captured with plain torch.cuda.graph after one eager call (which builds the tables), replayed twice:
    loss and gradient equal the eager ones bit for bit."""
    fs = LC.CASES["d"][2]
    ref = LC.reference("d")
    c = ref["c"].to(dev)
    e = ref["e"].to(dev).requires_grad_(True)
    crit = LC.make(None, fs)
    l_eager, g_eager = LC.run(None, dev, "d")
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        crit(c, e).backward()                                             # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    e.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss = crit(c, e)
        loss.backward()
    g = e.grad
    for _ in range(2):
        loss.detach().zero_()
        g.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), l_eager) and torch.equal(g, g_eager)


def test_leading_dimensions_are_flattened(dev):
    ref = LC.reference("a")
    c = ref["c"][:, None, :].repeat(1, 2, 1).to(dev)
    e = ref["e"][:, None, :].repeat(1, 2, 1).to(dev)
    loss, g = LC.run(None, dev, "a", c, e)
    l1, g1 = LC.run(None, dev, "a")
    assert g.shape == (2, 2, 5000) and g.device.type == "cuda" and torch.equal(g, (0.5 * g1)[:, None, :].repeat(1, 2, 1))
    assert abs(float(loss) - float(l1)) <= 2.0 ** -23


def test_weighted_loss_is_the_hand_written_sum(dev):
    loss_mod = LC.loss_mod()
    ref = LC.reference("a")
    c, e = ref["c"].to(dev), ref["e"].to(dev)
    crit = loss_mod.weighted_loss([["l1_loss", 1.0], ["stoi_loss", 0.25, {"sample_rate": 10000}]])
    l1, st = loss_mod.l1_loss(), loss_mod.stoi_loss(sample_rate=10000)
    x = e.clone().requires_grad_(True)
    loss = crit(c, x)
    loss.backward()
    y = e.clone().requires_grad_(True)
    hand = 1.0 * l1(c, y) + 0.25 * st(c, y)
    hand.backward()
    assert torch.equal(loss.detach(), hand.detach()) and torch.equal(x.grad, y.grad)
    _, gs = LC.run(None, dev, "a")
    assert (x.grad - 0.25 * gs).abs().max() > 0 and gs.abs().max() > 0
