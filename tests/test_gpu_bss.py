"""-m gpu: BSS Eval SDR (bss_corr_kernel / bss_solve_kernel behind wunet_bss_sdr_forward) on the MI355X: the cases of tests/bss_cases.py
on device tensors against the oracle of tests/bss_ref.py with the bar derived there, one captured call replayed after its signals and
lengths were overwritten, and the Trainer's "validation.sdr" key on a three-layer Model."""
import numpy as np
import pytest
import torch

import bss_cases as C
import bss_ref as R
import mix_cases as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_sdr_matches_the_long_double_oracle_on_device_tensors(dev, name):
    C.check_case(name, None, dev)


def test_cpu_tensors_are_refused(dev):
    eng = M.engine_or_default(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.bss_sdr(torch.ones(2, 64), torch.ones(2, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.metrics().sdr(torch.ones(2, 64), torch.ones(2, 64))
    x = torch.ones(2, 64, device=dev)
    with pytest.raises(RuntimeError, match="lives on"):
        eng.bss_sdr(x, x, lengths=torch.tensor([64, 64], dtype=torch.int64))
    with pytest.raises(RuntimeError, match="int64"):
        eng.bss_sdr(x, x, lengths=torch.tensor([64, 64], dtype=torch.int32, device=dev))


def test_a_captured_call_follows_its_signals_and_lengths(dev):
    """Case d (ragged lengths) captured on static tensors: one replay on the capture-time contents, one after other signals and other
    lengths were copied in; each equals the eager call on those contents bit for bit, and the oracle."""
    C.require_long_double()
    eng = M.engine_or_default(None)
    t = C.tile(None)
    d = C.case("d", t)
    rows, T = d["clean"].shape
    clean, est = torch.from_numpy(np.array(d["clean"])).to(dev), torch.from_numpy(np.array(d["est"])).to(dev)
    lengths = torch.from_numpy(np.array(d["lengths"])).to(dev)
    out, eager = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.bss_sdr(clean, est, d["n"], lengths=lengths, out=out)        # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.bss_sdr(clean, est, d["n"], lengths=lengths, out=out)
    rng = np.random.default_rng(41)
    clean2 = (0.1 * rng.standard_normal((rows, T))).astype(np.float32)
    est2 = (clean2 + 0.03 * rng.standard_normal((rows, T))).astype(np.float32)
    lengths2 = np.array([T, 700, 0, t + 1, 33], np.int64)
    first = None
    for k, contents in enumerate((None, (clean2, est2, lengths2))):
        if contents is not None:
            clean.copy_(torch.from_numpy(contents[0]))
            est.copy_(torch.from_numpy(contents[1]))
            lengths.copy_(torch.from_numpy(contents[2]))
        out.fill_(123.0)
        graph.replay()
        eng.bss_sdr(clean, est, d["n"], lengths=lengths, out=eager)
        torch.cuda.synchronize()
        assert M.bit_equal(out, eager), f"replay {k} differs from the eager call"
        ref = R.bss_reference(clean.cpu().numpy(), est.cpu().numpy(), d["n"], lengths.cpu().numpy(), K=C.K)
        C.check_against(ref, out, f"case d, replay {k}")
        if first is None:
            first = out.clone()
    assert torch.isnan(out[2]) and bool(torch.isfinite(out[[0, 1, 3, 4]]).all())
    assert not M.bit_equal(first[3:], out[3:])                            # (the second replay really scored the other batch)


def test_trainer_validation_reports_and_scores_sdr_on_the_device(dev, tmp_path):
    C.check_trainer(None, dev, tmp_path)
