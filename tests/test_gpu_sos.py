"""-m gpu: cascades of second-order sections (sos_windows_kernel behind wunet_sos_windows) on the MI355X: the cases of tests/sos_cases.py
on device tensors against the oracle of tests/sos_ref.py with the bar derived there, one captured graph replayed on its capture-time
tables and on new table contents, filters.sosfilt, MixLoader with the equalisers end to end, its captured batch as one linear chain of
kernel nodes, and three optimiser steps fed by it."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import scipy.signal
import torch

import mix_cases as M
import sos_cases as C
import sos_ref as R
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wd():
    return importlib.import_module(PKG_NAME + ".waveform_dataset")


@pytest.fixture(scope="module")
def filters():
    return importlib.import_module(PKG_NAME + ".filters")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_filtered_windows_match_the_long_double_oracle_on_device_tensors(dev, name):
    C.check_case(name, None, dev)


def test_cpu_tensors_are_refused(dev, filters):
    eng = M.engine_or_default(None)
    rows = torch.zeros(2, 4, dtype=torch.int64)
    coefs = torch.tensor([[[1.0, 0.0, 0.0, 0.0, 0.0]]]).repeat(2, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.sos_windows(torch.zeros(100), rows, coefs, torch.empty(2, 1, 40))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        filters.sosfilt(torch.zeros(2, 64), np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]))


def test_sosfilt_on_the_device_is_scipys(dev, filters):
    C.require_long_double()
    rng = np.random.default_rng(8)
    T = 1000
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 1, T)).astype(np.float32)).to(dev)
    sos = np.stack([scipy.signal.butter(4, 3400.0, "lowpass", fs=16000.0, output="sos"), 2.0 * scipy.signal.butter(4, 300.0, "highpass", fs=16000.0, output="sos")])
    y = filters.sosfilt(x, sos)
    assert y.shape == x.shape and y.device == x.device and y.dtype == torch.float32
    k = (sos[..., [0, 1, 2, 4, 5]] / sos[..., 3:4]).astype(np.float32)
    start = np.arange(2) * T
    ref = R.sos_reference(x.cpu().numpy().reshape(-1), np.stack([start, start, 0 * start, 0 * start], 1), k, T, 0)
    C.check_against(ref, y, "sosfilt, per-row table with a0 = 2")


def test_a_captured_launch_follows_its_tables(dev):
    """Case d (linear rows, lead-ins of different lengths) captured on static table tensors: one replay on the capture-time tables, one
    after other rows and coefficients were copied in; each equals the eager call on those tables bit for bit, and the oracle."""
    C.require_long_double()
    eng = M.engine_or_default(None)
    d = C.case("d", *C.tile(None))
    B, L, lead = d["rows"].shape[0], d["L"], d["lead"]
    flat = M.guarded_flat(d["flat"], dev)
    rows, coefs = torch.from_numpy(np.array(d["rows"])).to(dev), torch.from_numpy(np.array(d["coefs"])).to(dev)
    out, eager = torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.sos_windows(flat, rows, coefs, out, lead=lead)               # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.sos_windows(flat, rows, coefs, out, lead=lead)
    rows2 = torch.tensor([[700, 650, 0, 0], [0, 20, 33, 5], [400, 0, 0, 0], [10, 900, 250, 249], [1000, 1000, 0, 0]], dtype=torch.int64)
    coefs2 = torch.from_numpy(np.stack([C._random(np.random.default_rng(40 + b), 2) for b in range(B)]))
    first = None
    for k, tables in enumerate((None, (rows2, coefs2))):
        if tables is not None:
            rows.copy_(tables[0])
            coefs.copy_(tables[1])
        out.fill_(float("nan"))
        graph.replay()
        eng.sos_windows(flat, rows, coefs, eager, lead=lead)
        torch.cuda.synchronize()
        assert M.bit_equal(out, eager), f"replay {k} differs from the eager call"
        ref = R.sos_reference(d["flat"], rows.cpu().numpy(), coefs.cpu().numpy(), L, lead)
        C.check_against(ref, out, f"case d, replay {k}")
        if first is None:
            first = out.clone()
    assert not M.bit_equal(first, out)                                    # (the second replay really filtered the other batch)


def _loaded_hip_runtime():
    """The HIP runtime this process already runs on, opened by its path (a second copy would not know the graph)."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def _packed(wd, tmp_path):
    cl_list, no_list, _, _ = M.corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    return cp, npfx


def test_the_captured_equalised_batch_is_one_linear_chain(dev, wd, tmp_path):
    """The launches of a MixLoader batch with both equalisers (MixLoader.enqueue_equalised on the batch's tables, copied to the device
    beforehand), captured: kernel launches only - the speech filter, the noise filter, the mix's two -, each depending on the one
    before it: one root, n - 1 edges, no node with two successors or two predecessors.  The replay is the eager batch bit for bit."""
    cp, npfx = _packed(wd, tmp_path)
    loader = wd.MixLoader(cp, npfx, batch_size=4, sample_length=256, device=dev, seed=3, steps_per_epoch=1, **C.EQ)
    mixture, clean, names = next(iter(loader))
    draw = loader.last_draw
    pick_starts = torch.tensor([int(loader.starts[loader.names.index(nm)]) for nm in names], dtype=torch.int64)
    zero = torch.zeros(4, dtype=torch.int64)
    speech_table = torch.stack([draw["rows"][:, 0], pick_starts, zero, zero], dim=1)
    host = loader.eq_tables(speech_table, draw["rows"], draw["eq_speech"], draw["eq_noise"])
    tables = {"speech": tuple(t.to(dev) for t in host["speech"]), "noise": tuple(t.to(dev) for t in host["noise"]), "rows": host["rows"].to(dev)}
    params = draw["params"].to(dev)
    chain = lambda: loader.enqueue_equalised(loader.clean, tables, params, loader.eq_lead)          # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain()                                                          # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        outs = chain()
    hip = _loaded_hip_runtime()
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    assert n.value == 4, n.value                                          # sos_windows_kernel twice, mix_partial_kernel, mix_apply_kernel
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kinds = []
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        kinds.append(kind.value)
    assert kinds == [0] * n.value, kinds                                  # hipGraphNodeTypeKernel
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    assert e.value == n.value - 1, e.value
    src, dst = (ctypes.c_void_p * e.value)(), (ctypes.c_void_p * e.value)()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    assert len(set(src)) == e.value and len(set(dst)) == e.value          # no fork, no join
    r = ctypes.c_size_t(0)
    assert hip.hipGraphGetRootNodes(g, None, ctypes.byref(r)) == 0 and r.value == 1
    graph.instantiate()
    graph.replay()
    torch.cuda.synchronize()
    assert M.bit_equal(outs[0], mixture) and M.bit_equal(outs[1], clean) and M.bit_equal(outs[2], draw["gains"])


def test_mix_loader_with_equalisers_end_to_end_on_the_device(dev, wd, tmp_path):
    C.check_loader(wd, tmp_path, None, dev)


def test_mix_loader_with_equalisers_and_an_rir_shard_on_the_device(dev, wd, tmp_path):
    C.check_rir_loader(wd, tmp_path, None, dev)


def test_three_optimiser_steps_fed_by_the_equalised_loader(pkg, dev, wd, tmp_path):
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    cp, npfx = _packed(wd, tmp_path)
    loader = wd.MixLoader(cp, npfx, batch_size=4, sample_length=256, snr_db=(0.0, 20.0), level_db=(-6.0, 3.0), device=dev, seed=2, steps_per_epoch=3,
                          **C.EQ)
    torch.manual_seed(0)
    m = pkg.Model(n_layers=3, channels_interval=4).to(dev)
    opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    before = [p.detach().clone() for p in m.parameters()]
    cfg = {"root_dir": str(tmp_path), "experiment_name": "eq", "trainer": {"epochs": 1, "save_checkpoint_interval": 0}}
    tr = trainer_mod.Trainer(cfg, False, m, pkg.mse_loss(), opt, loader, None)
    tr.train()
    torch.cuda.synchronize()
    assert len(tr.epoch_losses) == 1 and all(math.isfinite(v) for v in tr.epoch_losses), tr.epoch_losses
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))     # the three steps moved the weights
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert loader.last_draw["eq_speech"].shape == (4, 3, 6) and loader.last_draw["eq_noise"].shape == (4, 2, 6)
