"""-m gpu: mixtures made on the device (mix_partial_kernel / mix_apply_kernel behind wunet_mix_windows) on the MI355X: the six cases of
tests/mix_cases.py on device tensors against the float64 oracle of tests/mix_ref.py with the bars derived there, one captured graph
replayed on its capture-time tables and on new table contents, MixLoader end to end and three optimiser steps fed by it."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch

import mix_cases as C
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wd():
    return importlib.import_module(PKG_NAME + ".waveform_dataset")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_mixed_batches_match_the_float64_oracle_on_device_tensors(dev, name):
    C.check_case(name, None, dev)


def test_cpu_tensors_are_refused(dev):
    d = C.case("a")
    t = lambda x: torch.from_numpy(np.array(x))          # noqa: E731
    B, L = d["rows"].shape[0], d["L"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.engine_or_default(None).mix_windows(t(d["clean"]), t(d["noise"]), t(d["rows"]), t(d["params"]), torch.empty(B, 1, L), torch.empty(B, 1, L))


def _static(dev, name):
    d = C.case(name)
    B, L = d["rows"].shape[0], d["L"]
    cf, nf = C.guarded_flat(d["clean"], dev), C.guarded_flat(d["noise"], dev)
    rows, params = torch.from_numpy(np.array(d["rows"])).to(dev), torch.from_numpy(np.array(d["params"])).to(dev)
    outs = [torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev), torch.empty(B, 2, device=dev)]
    return d, cf, nf, rows, params, outs


def _capture(dev, eng, cf, nf, rows, params, outs, graph):
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        eng.mix_windows(cf, nf, rows, params, *outs, peak_limit=C.PEAK)          # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    with torch.cuda.graph(graph):
        eng.mix_windows(cf, nf, rows, params, *outs, peak_limit=C.PEAK)


def test_a_captured_pair_of_launches_follows_its_tables(dev):
    """Case c (16 pieces per row) captured on static table tensors: one replay on the capture-time tables, one after other table
    contents were copied in; each equals the eager call on those tables bit for bit."""
    eng = C.engine_or_default(None)
    d, cf, nf, rows, params, outs = _static(dev, "c")
    graph = torch.cuda.CUDAGraph()
    _capture(dev, eng, cf, nf, rows, params, outs, graph)
    eager = [torch.empty_like(o) for o in outs]
    rows2 = torch.tensor([[12345, 20000, 3001, 77], [9, 100, 19000, 18999]], dtype=torch.int64)
    params2 = torch.tensor([[15.0, 2.0], [2.5, 0.25]], dtype=torch.float32)
    for k, (r, p) in enumerate(((None, None), (rows2, params2))):
        if r is not None:
            rows.copy_(r)
            params.copy_(p)
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        eng.mix_windows(cf, nf, rows, params, *eager, peak_limit=C.PEAK)
        torch.cuda.synchronize()
        assert all(C.bit_equal(a, b) for a, b in zip(outs, eager)), f"replay {k} differs from the eager call"
        ref = C.R.mix_reference(d["clean"], d["noise"], rows.cpu().numpy(), params.cpu().numpy(), d["L"], C.PEAK)
        C.check_against(ref, *outs, f"case c, replay {k}")
    assert not C.bit_equal(outs[0], C.run(None, dev, "c")[0])                     # (the second replay really mixed the other batch)


def _loaded_hip_runtime():
    """The HIP runtime this process already runs on, opened by its path (a second copy would not know the graph)."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert len(paths) == 1, paths
    return ctypes.CDLL(paths.pop())


def test_the_captured_graph_is_one_linear_chain(dev):
    """The capture of one call holds kernel launches only, each depending on the one before it: one root, n - 1 edges, no node with two
    successors or two predecessors - nothing was forked to a side stream."""
    eng = C.engine_or_default(None)
    _, cf, nf, rows, params, outs = _static(dev, "b")
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    _capture(dev, eng, cf, nf, rows, params, outs, graph)
    hip = _loaded_hip_runtime()
    g = ctypes.c_void_p(graph.raw_cuda_graph())
    n = ctypes.c_size_t(0)
    assert hip.hipGraphGetNodes(g, None, ctypes.byref(n)) == 0
    assert n.value == 2, n.value                                                  # mix_partial_kernel, mix_apply_kernel
    nodes = (ctypes.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(g, nodes, ctypes.byref(n)) == 0
    kinds = []
    for node in nodes:
        kind = ctypes.c_int(-1)
        assert hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) == 0
        kinds.append(kind.value)
    assert kinds == [0] * n.value, kinds                                          # hipGraphNodeTypeKernel
    e = ctypes.c_size_t(0)
    assert hip.hipGraphGetEdges(g, None, None, ctypes.byref(e)) == 0
    assert e.value == n.value - 1, e.value
    src, dst = (ctypes.c_void_p * e.value)(), (ctypes.c_void_p * e.value)()
    assert hip.hipGraphGetEdges(g, src, dst, ctypes.byref(e)) == 0
    assert len(set(src)) == e.value and len(set(dst)) == e.value                  # no fork, no join
    r = ctypes.c_size_t(0)
    assert hip.hipGraphGetRootNodes(g, None, ctypes.byref(r)) == 0 and r.value == 1


def test_mix_loader_end_to_end_on_the_device(dev, wd, tmp_path):
    C.check_loader(wd, tmp_path, None, dev)


def test_three_optimiser_steps_fed_by_the_mix_loader(pkg, dev, wd, tmp_path):
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    cl_list, no_list, _, _ = C.corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    loader = wd.MixLoader(cp, npfx, batch_size=4, sample_length=256, snr_db=(0.0, 20.0), level_db=(-6.0, 3.0), device=dev, seed=2, steps_per_epoch=3)
    torch.manual_seed(0)
    m = pkg.Model(n_layers=3, channels_interval=4).to(dev)
    opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    before = [p.detach().clone() for p in m.parameters()]
    cfg = {"root_dir": str(tmp_path), "experiment_name": "mix", "trainer": {"epochs": 1, "save_checkpoint_interval": 0}}
    tr = trainer_mod.Trainer(cfg, False, m, pkg.mse_loss(), opt, loader, None)
    tr.train()
    torch.cuda.synchronize()
    assert len(tr.epoch_losses) == 1 and all(math.isfinite(v) for v in tr.epoch_losses), tr.epoch_losses
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))     # the three steps moved the weights
    assert all(torch.isfinite(p).all() for p in m.parameters())
