"""-m gpu: the compressed spectral loss (cspec_fwd_kernel / cspec_final_kernel / cspec_bwd_kernel / stft_ola_kernel behind
wunet_cspec_*) on the MI355X: the six cases of tests/cspec_loss_cases.py on device tensors against the float64 oracle of
tests/cspec_loss_ref.py with the same bars as tests/test_cspec_loss_emu.py (loss 4 d_ref + 2^-23, gradient 4 d_ref, d_ref measured on
the CPU at test time and printed beside every d), determinism, inputs with 4-byte alignment only, one captured graph, one training
step of a small net through weighted_loss(l1 + compressed spectral)."""
import importlib

import pytest
import torch

import cspec_loss_cases as C
import cspec_loss_ref as R
from conftest import PKG_NAME
from oracle import plan

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name,compress,complex_weight", C.params(sorted(C.CASES)))
def test_loss_and_gradient_on_device_tensors(dev, name, compress, complex_weight):
    C.check_case(name, compress, complex_weight, None, dev)


def test_two_runs_are_bit_identical_and_grad_loss_scales_exactly(dev):
    rows, T, res = C.CASES["d"]
    c, e = R.pair(rows, T)
    l1, g1 = C.run(None, dev, res, c, e)
    l2, g2 = C.run(None, dev, res, c, e)
    assert torch.equal(l1, l2) and torch.equal(g1, g2)
    _, gh = C.run(None, dev, res, c, e, grad_loss=0.5)
    assert torch.equal(gh, 0.5 * g1)
    crit = C.criterion(None, res)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(c, e)
    with pytest.raises(NotImplementedError, match="clean"):
        crit(c.to(dev).requires_grad_(True), e.to(dev))


def test_equal_signals_and_an_all_zero_row(dev):
    """Equal signals: exactly 0.0 and an all-zero gradient (the backward meets the forward's bits).  An all-zero enhanced row: a
    finite, non-zero gradient on that row."""
    rows, T, res = C.CASES["d"]
    c, e = R.pair(rows, T)
    loss, g = C.run(None, dev, res, c, c.clone())
    assert float(loss) == 0.0 and not g.any()
    e = e.clone()
    e[1] = 0.0
    loss, g = C.run(None, dev, res, c, e)
    assert torch.isfinite(loss) and torch.isfinite(g).all() and g[1].any() and g[0].any()


def test_inputs_with_4_byte_alignment_only(dev):
    """Case b with both inputs as views one float into their buffers: the same bars, and the same bits as the aligned run (the loaders
    read single floats, no path depends on the alignment)."""
    rows, T, res = C.CASES["b"]
    ref = R.case_reference(rows, T, res, *C.DEFAULT)
    bc = torch.zeros(rows * T + 8, device=dev)
    be = torch.zeros(rows * T + 8, device=dev)
    bc[1:1 + rows * T] = ref["c"].reshape(-1).to(dev)
    be[1:1 + rows * T] = ref["e"].reshape(-1).to(dev)
    cv, ev = bc[1:1 + rows * T].view(rows, 1, T), be[1:1 + rows * T].view(rows, 1, T)
    assert cv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and cv.is_contiguous()
    loss, g = C.check_case("b", *C.DEFAULT, None, dev, c=cv, e=ev)
    la, ga = C.run(None, dev, res, ref["c"], ref["e"])
    assert torch.equal(loss, la) and torch.equal(g, ga)


def test_a_captured_graph_replays_the_eager_result(dev):
    """Forward + backward of case a captured with plain torch.cuda.graph after one eager call (which builds the basis), replayed
    twice: loss and gradient equal the eager ones bit for bit."""
    rows, T, res = C.CASES["a"]
    c, e = R.pair(rows, T)
    l_eager, g_eager = C.run(None, dev, res, c, e)
    crit = C.criterion(None, res)
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


def test_one_training_step_through_weighted_loss(pkg, dev):
    """A 4-level Model at B = 2, T = 1024 trained through weighted_loss(l1 + 0.5 compressed spectral, case d's resolutions): one eager
    step runs, every parameter gradient is finite, and at least half of them differ from those of the l1-only step."""
    n, ci, B, T = 4, 8, 2, 1024
    res = C.CASES["d"][2]
    noisy, clean = plan.golden_batch(B, T, 0)
    noisy, clean = torch.from_numpy(noisy).to(dev), torch.from_numpy(clean).to(dev)
    args = {"fft_sizes": [r[0] for r in res], "hop_sizes": [r[1] for r in res], "win_lengths": [r[2] for r in res]}
    grads = []
    for terms in ([["l1_loss", 1.0]], [["l1_loss", 1.0], ["compressed_spectral_loss", 0.5, args]]):
        m = pkg.Model(n_layers=n, channels_interval=ci)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in plan.golden_state(n, ci, 0).items()})
        m.to(dev).train()
        opt = importlib.import_module(PKG_NAME + ".optim").FusedAdam(m.parameters(), lr=1e-3)
        crit = pkg.weighted_loss(terms)
        opt.zero_grad()
        loss = crit(clean, m(noisy))
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        assert torch.isfinite(loss)
        grads.append({k: p.grad.clone() for k, p in m.named_parameters()})
    assert all(torch.isfinite(g).all() for g in grads[1].values())
    differing = [k for k in grads[0] if not torch.equal(grads[0][k], grads[1][k])]
    print(f"weighted step: {len(differing)} of {len(grads[0])} parameter gradients differ from the l1-only step")
    assert len(differing) >= len(grads[0]) // 2
