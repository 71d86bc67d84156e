"""-m gpu: STOI per row (stoi_resample_kernel / stoi_mask_kernel / stoi_spec_kernel / stoi_segment_kernel / stoi_final_kernel behind
wunet_stoi_*) on the MI355X: the six cases of tests/stoi_cases.py on device tensors against the float64 oracle of tests/stoi_ref.py
with the bars of tests/test_stoi_emu.py (frames exactly, |score - oracle64| <= 4 d_ref + 2^-23, d_ref measured on the CPU at test time
and printed beside every d), determinism, inputs with 4-byte alignment only, one captured graph, leading dimensions."""
import pytest
import torch

import stoi_cases as C
import stoi_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_scores_and_frame_counts_on_device_tensors(dev, name):
    C.check_case(name, None, dev)


def test_two_runs_are_bit_identical_and_cpu_tensors_are_refused(dev):
    s1, f1 = C.run(None, dev, "d")
    s2, f2 = C.run(None, dev, "d")
    assert torch.equal(s1, s2) and torch.equal(f1, f2)
    ref = R.case_reference(*C.CASES["d"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.metrics().stoi(ref["c"], ref["e"])


@pytest.mark.parametrize("name", ("a", "b"))
def test_inputs_with_4_byte_alignment_only(dev, name):
    """Both inputs as views one float into their buffers (case a: the spectrum's loader reads them; case b: the resampler does): the
    same checks, and the same bits as the aligned run - every loader reads single floats."""
    rows, T = C.CASES[name][:2]
    ref = R.case_reference(*C.CASES[name])
    bc = torch.zeros(rows * T + 8, device=dev)
    be = torch.zeros(rows * T + 8, device=dev)
    bc[1:1 + rows * T] = ref["c"].reshape(-1).to(dev)
    be[1:1 + rows * T] = ref["e"].reshape(-1).to(dev)
    cv, ev = bc[1:1 + rows * T].view(rows, T), be[1:1 + rows * T].view(rows, T)
    assert cv.data_ptr() % 16 == 4 and ev.data_ptr() % 16 == 4 and cv.is_contiguous()
    s, f = C.check_case(name, None, dev, c=cv, e=ev)
    sa, fa = C.run(None, dev, name)
    assert torch.equal(s, sa) and torch.equal(f, fa)


def test_a_captured_graph_replays_the_eager_result(dev):
    """Case d captured with plain torch.cuda.graph after one eager call (which builds the tables), replayed twice: scores and frame
    counts equal the eager ones bit for bit."""
    fs = C.CASES["d"][2]
    ref = R.case_reference(*C.CASES["d"])
    c, e = ref["c"].to(dev), ref["e"].to(dev)
    s_eager, f_eager = C.metrics().stoi(c, e, sample_rate=fs, return_frames=True)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        C.metrics().stoi(c, e, sample_rate=fs, return_frames=True)      # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s, f = C.metrics().stoi(c, e, sample_rate=fs, return_frames=True)
    for _ in range(2):
        s.zero_()
        f.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(s, s_eager) and torch.equal(f, f_eager)


def test_leading_dimensions_are_flattened(dev):
    ref = R.case_reference(*C.CASES["a"])
    c = ref["c"][:, None, :].repeat(1, 3, 1).to(dev)
    e = ref["e"][:, None, :].repeat(1, 3, 1).to(dev)
    s = C.metrics().stoi(c, e, sample_rate=10000)
    s2, _ = C.run(None, dev, "a")
    assert s.shape == (6,) and s.device.type == "cuda" and torch.equal(s, s2.repeat_interleave(3))
