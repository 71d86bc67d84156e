"""-m gpu: sample-rate conversion (resample_rows_kernel behind wunet_resample_rows) on the MI355X: the cases of tests/resample_cases.py
on device tensors against the float64 oracle of tests/resample_ref.py with the bar derived there, the identity-model enhance at 48 kHz,
and one captured launch replayed after its row table and its input were overwritten in place."""
import numpy as np
import pytest
import torch

import chunks_cases as CC
import resample_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_cases_a_to_e_and_h_match_the_float64_oracle_on_device_tensors(dev, name):
    C.check_case(name, None, dev)                      # (two runs bit-equal is part of every case)


@pytest.mark.parametrize("rates", C.RAGGED_RATES)
def test_case_f_a_ragged_table_in_guarded_arrays(dev, rates):
    C.check_case_f(None, dev, rates)


@pytest.mark.parametrize("rates", C.RAGGED_RATES + ((16000, 44100),))
def test_case_g_output_lengths_off_the_natural_one_and_at_the_block_size(dev, rates):
    C.check_case_g(None, dev, rates)


def test_enhance_with_the_identity_model_at_48_khz(dev):
    out, stub = C.check_enhance_round_trip(None, dev, 48000)
    assert all(s.is_cuda for s in stub.seen)
    host, _ = C.check_enhance_round_trip(None, dev, 48000, to_host=True)
    assert host.device.type == "cpu" and host.is_pinned() and CC.bit_equal(host, out.cpu())      # one pinned copy, the same bits


def test_cpu_tensors_are_refused(dev):
    rs, eng = C.resample_mod(), C.engine_or_default(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.resample(torch.zeros(100), 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.resample_rows(torch.zeros(100), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(34), 48000, 16000, 34)


def test_a_captured_launch_follows_its_table_and_its_input(dev):
    """resample_rows at 160 / 441 captured after an eager call (which makes the device copy of the filter): the replay on the
    capture-time table, then one after the table and the input were overwritten in place - other row lengths, other samples.  Each
    equals the eager call bit for bit and meets the bar against the oracle for the table it ran on.  One stream, no parallel branches."""
    eng, rs = C.engine_or_default(None), C.resample_mod()
    rate_in, rate_out = 44100, 16000
    tables = []
    for lengths in ((1000, 255), (257, 700)):
        rows = [(T, rs.resampled_length(T, rate_in, rate_out)) for T in lengths]
        a, _ = C.odd_layout([r[0] for r in rows])
        b, _ = C.odd_layout([r[1] for r in rows], first=3)
        tables.append((rows, np.asarray([(s, T, o, To) for (T, To), s, o in zip(rows, a, b)], np.int64)))
    in_total, out_total, max_out = 1300, 480, 363

    def source(k):
        src = np.zeros(in_total, np.float32)
        for j, (s, T, _, _) in enumerate(tables[k][1].tolist()):
            src[s:s + T] = C.signal(T, seed=j % 3)
        return torch.from_numpy(src)

    flat, table = source(0).to(dev), torch.from_numpy(tables[0][1]).to(dev)
    out = torch.empty(out_total, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.resample_rows(flat, table, out, rate_in, rate_out, max_out)              # the eager call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.resample_rows(flat, table, out, rate_in, rate_out, max_out)
    results = []
    for k, (rows, table_np) in enumerate(tables):
        flat.copy_(source(k))
        table.copy_(torch.from_numpy(table_np))
        out.fill_(float("nan"))
        graph.replay()
        eager = torch.full_like(out, float("nan"))
        eng.resample_rows(flat, table, eager, rate_in, rate_out, max_out)
        torch.cuda.synchronize()
        assert CC.bit_equal(out, eager), f"replay {k} differs from the eager call"
        for j, ((T, To), (_, _, o, _)) in enumerate(zip(rows, table_np.tolist())):
            ref, bar = C.reference(rate_in, rate_out, T, j % 3, To)
            C.check_against(ref, bar, out[o:o + To], f"replay {k}, row {j} (T_in {T})")
        results.append(out.clone())
    assert not CC.bit_equal(results[0], results[1])                                   # (the second replay really followed the other table)
