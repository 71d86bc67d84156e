"""-m gpu: ESTOI (estoi_segment_kernel / estoi_segment_bwd_kernel / estoi_gather_kernel of csrc/wunet_estoi.h behind wunet_estoi_*) on the
MI355X, through the default engine: the six cases of tests/stoi_cases.py on device tensors against the float64 yardsticks of
tests/estoi_ref.py with the conditions and bars of tests/estoi_cases.py (d_ref measured on the CPU at test time and printed beside
every d), determinism, one captured graph of forward + backward, the refusal of CPU tensors."""
import pytest
import torch

import estoi_cases as EC
import estoi_ref as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_scores_and_frame_counts_on_device_tensors(dev, name):
    EC.check_case(name, None, dev)


@pytest.mark.parametrize("name", sorted(EC.CASES))
def test_loss_and_gradient_on_device_tensors(dev, name):
    EC.check_loss_case(name, None, dev)


def test_two_runs_are_bit_identical_and_cpu_tensors_are_refused(dev):
    s1, f1 = EC.run(None, dev, "d")
    s2, f2 = EC.run(None, dev, "d")
    assert torch.equal(s1, s2) and torch.equal(f1, f2)
    l1, g1 = EC.run_loss(None, dev, "d")
    l2, g2 = EC.run_loss(None, dev, "d")
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and g1.abs().max() > 0
    lh, gh = EC.run_loss(None, dev, "d", grad_loss=0.5)
    assert torch.equal(lh, l1) and torch.equal(gh, 0.5 * g1)
    ref = E.case_reference(*EC.CASES["d"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EC.C.metrics().stoi(ref["c"], ref["e"], extended=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EC.make_loss(None, 16000)(ref["c"], ref["e"])


def test_inputs_with_4_byte_alignment_only(dev):
    cv, ev = EC.offset_views("b", dev)
    loss, g = EC.check_loss_case("b", None, dev, c=cv, e=ev)
    la, ga = EC.run_loss(None, dev, "b")
    assert torch.equal(loss, la) and torch.equal(g, ga)


def test_a_captured_graph_replays_the_eager_result(dev):
    """Forward + backward of case d captured with plain torch.cuda.graph after one eager call (which builds the tables), replayed twice:
    loss and gradient equal the eager ones bit for bit."""
    fs = EC.CASES["d"][2]
    ref = E.case_reference(*EC.CASES["d"])
    c = ref["c"].to(dev)
    e = ref["e"].to(dev).requires_grad_(True)
    crit = EC.make_loss(None, fs)
    l_eager, g_eager = EC.run_loss(None, dev, "d")
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
