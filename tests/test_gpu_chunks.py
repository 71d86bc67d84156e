"""-m gpu: chunked enhancement with overlap (chunk_gather_kernel / chunk_overlap_add_kernel behind wunet_chunk_gather /
wunet_chunk_overlap_add) on the MI355X: the cases of tests/chunks_cases.py on device tensors against the float64 oracle of
tests/chunks_ref.py with the bar derived there, one real-size row with the stub and with the 12-level model, and a captured pair of
launches replayed on its capture-time tables and on new table contents."""
import numpy as np
import pytest
import torch

import chunks_cases as C
import chunks_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("window", C.WINDOWS)
@pytest.mark.parametrize("name", ["b", "c", "d", "e"])
def test_overlapped_chunks_match_the_float64_oracle_on_device_tensors(dev, name, window):
    C.check_stub_case(name, None, dev, window)


def test_case_e_unaligned_guarded_arrays(dev):
    C.check_case_e_guards(None, dev)


@pytest.mark.parametrize("window", C.WINDOWS)
def test_case_f_many_recordings_share_the_slabs(dev, window):
    C.check_many(None, dev, window)


def test_an_identity_model_gives_the_input_back(dev):
    C.check_stub_case("b", None, dev, "hann", identity=True)


def test_case_g_one_real_size_row_with_the_stub(dev):
    L, m, f, T = C.REAL
    stub = C.Stub(L).to(dev)
    out, ref = C.check_recorded(None, dev, stub, L, m, f, T, label="case g")
    assert R.count(T, L, m, f) == 5 and int(ref["faded"].sum()) == 4 * f
    # the stub's own arithmetic on the host gives the same chunk outputs: the oracle of the small cases, at this size
    C.check_against(C.reference_for(C.recording(T, seed=2), L, m, f, "hann", stub=stub), out, "case g, the oracle's own chunks")
    # to_host: one pinned buffer, the same bits
    host = C.enhance_one(None, dev, C.recording(T, seed=2), L, m, f, "hann", C.Stub(L).to(dev), to_host=True)
    assert host.device.type == "cpu" and host.is_pinned() and C.bit_equal(host, out.cpu())


def test_case_h_the_twelve_level_model(dev, pkg):
    L, m, f, T = C.REAL
    torch.manual_seed(0)
    model = pkg.Model().to(dev).eval()
    out, _ = C.check_recorded(None, dev, model, L, m, f, T, label="case h")
    assert float(out.abs().max()) > 0.0
    # slabs of two chunks (2 + 2 + 1): the same check on the chunk outputs of those forwards
    C.check_recorded(None, dev, model, L, m, f, T, label="case h, max_batch 2", max_batch=2)


def test_cpu_tensors_are_refused(dev):
    inf, eng = C.inference(), C.engine_or_default(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inf.enhance(C.Stub(64), torch.zeros(1, 1, 100), 64, margin=8, fade=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.chunk_gather(torch.zeros(100), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 1, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.chunk_overlap_add(torch.zeros(1, 1, 64), torch.zeros(1, 4, dtype=torch.int64), torch.zeros(100), 8, 16, torch.zeros(16), 100)


def test_a_captured_pair_follows_its_tables(dev):
    """gather -> stub -> overlap-add captured on static tensors (case b's geometry, two recordings of 100 and 60 samples: 3 + 2 chunks):
    one replay on the capture-time tables, one after the tables of two other recordings with the same table sizes (70 and 90 samples:
    2 + 3 chunks) were copied in; each equals the eager calls on those tables bit for bit, and the oracle."""
    L, m, f = 64, 8, 16
    inf, eng = C.inference(), C.engine_or_default(None)
    stub = C.Stub(L).to(dev)
    flat = torch.from_numpy(np.array(C.recording(200, seed=3))).to(dev)
    ramp = inf.chunk_ramp(f).to(dev)
    tables = [inf.chunk_tables(lengths, L, m, f) for lengths in ((100, 60), (70, 90))]
    assert all(rows.shape == (5, 3) and recs.shape == (2, 4) and total <= 200 for rows, recs, total in tables)
    rows, recs = torch.from_numpy(tables[0][0]).to(dev), torch.from_numpy(tables[0][1]).to(dev)
    chunks, out = torch.empty(5, 1, L, device=dev), torch.empty(200, device=dev)

    def run(chunks, out):
        eng.chunk_gather(flat, rows, chunks)
        eng.chunk_overlap_add(chunks * stub.a + stub.b, recs, out, m, f, ramp, 100)

    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        run(chunks, out)                                                             # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(chunks, out)
    results = []
    for k, (rows_np, recs_np, _) in enumerate(tables):
        rows.copy_(torch.from_numpy(rows_np))
        recs.copy_(torch.from_numpy(recs_np))
        out.fill_(float("nan"))
        graph.replay()
        eager_chunks, eager = torch.empty_like(chunks), torch.full_like(out, float("nan"))
        run(eager_chunks, eager)
        torch.cuda.synchronize()
        assert C.bit_equal(chunks, eager_chunks) and C.bit_equal(out, eager), f"replay {k} differs from the eager calls"
        for start, T, _, _ in recs_np.tolist():
            x = flat[start:start + T].cpu().numpy()
            C.check_against(C.reference_for(x, L, m, f, "hann", stub=stub), out[start:start + T], f"replay {k}, recording at {start}")
        results.append(out.clone())
    assert not C.bit_equal(results[0], results[1])                                    # (the second replay really followed the other tables)
