"""-m gpu: reverberant speech made on the device (reverb_kernel behind wunet_reverb_windows, apply_level_kernel behind
wunet_apply_level) on the MI355X: the cases of tests/reverb_cases.py on device tensors against the float64 oracle of
tests/reverb_ref.py with the bar derived there (and one row of 16384 samples x 16384 taps), one captured graph of the loader's
four-launch batch replayed on its capture-time tables and on new table contents, MixLoader with an RIR shard end to end and three
optimiser steps fed by it."""
import importlib
import math

import numpy as np
import pytest
import torch

import mix_cases as C
import mix_ref
import reverb_cases as V
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def wd():
    return importlib.import_module(PKG_NAME + ".waveform_dataset")


@pytest.mark.parametrize("name", sorted(V.GPU_CASES))
def test_reverberant_batches_match_the_float64_oracle_on_device_tensors(dev, name):
    V.check_case(name, None, dev)


def test_apply_level_is_the_one_multiply_of_the_mix(dev):
    V.check_apply_level(None, dev)


def test_cpu_tensors_are_refused(dev):
    d = V.case("a")
    t = lambda x: torch.from_numpy(np.array(x))          # noqa: E731
    B, L = d["rows"].shape[0], d["L"]
    eng = C.engine_or_default(None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.reverb_windows(t(d["clean"]), t(d["rir"]), t(d["rows"]), torch.empty(B, 1, L), torch.empty(B, 1, L))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eng.apply_level(torch.empty(B, 1, L), torch.empty(B, 2))


def test_a_captured_four_launch_batch_follows_its_tables(dev):
    """The loader's chain (reverb -> mix on the staged batch -> level of the target) on case d's arrays and static table tensors: one
    replay on the capture-time tables, one after other table contents were copied in; each equals the eager chain on those tables
    bit for bit, and the oracle stage by stage."""
    eng = C.engine_or_default(None)
    d, m = V.case("d"), C.case("b")
    B, L, E = 2, d["L"], d["E"]
    cf, rf, nf = C.guarded_flat(d["clean"], dev), C.guarded_flat(d["rir"], dev), C.guarded_flat(m["noise"], dev)
    rir_rows = torch.from_numpy(np.array(d["rows"])).to(dev)
    mix_rows_np = np.array(m["rows"])
    mix_rows_np[:, 0] = np.arange(B) * L
    mix_rows, params = torch.from_numpy(mix_rows_np).to(dev), torch.from_numpy(np.array(m["params"])).to(dev)
    new = lambda: [torch.empty(B, 1, L, device=dev) for _ in range(4)] + [torch.empty(B, 2, device=dev)]          # noqa: E731
    outs, eager = new(), new()                            # staged, direct (the target after the chain), mixture, a r, gains
    chain = lambda o: V.four_launches(eng, cf, rf, nf, rir_rows, mix_rows, params, *o, early_taps=E)          # noqa: E731
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain(outs)                                       # the warm-up call
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain(outs)
    first = None
    rir_rows2 = torch.tensor([[4000, 3000, 5, 700], [100, 0, 1010, 0]], dtype=torch.int64)
    mix_rows2 = torch.tensor([[0, 100, 5000, 77], [L, 0, 1000, 999]], dtype=torch.int64)
    params2 = torch.tensor([[15.0, 2.0], [2.5, 0.25]], dtype=torch.float32)
    for k, tables in enumerate((None, (rir_rows2, mix_rows2, params2))):
        if tables is not None:
            rir_rows.copy_(tables[0])
            mix_rows.copy_(tables[1])
            params.copy_(tables[2])
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        chain(eager)
        torch.cuda.synchronize()
        assert all(C.bit_equal(a, b) for a, b in zip(outs, eager)), f"replay {k} differs from the eager chain"
        staged, target, mixture, ar, gains = outs
        ref = V.R.reverb_reference(d["clean"], d["rir"], rir_rows.cpu().numpy(), L, E)
        V.check_against(ref, d["clean"], staged, torch.from_numpy(ref["direct"]).float()[:, None], f"case d, replay {k}")       # (direct was scaled in place)
        mref = mix_ref.mix_reference(staged.cpu().numpy().reshape(-1), m["noise"], mix_rows.cpu().numpy(), params.cpu().numpy(), L, C.PEAK)
        C.check_against(mref, mixture, ar, gains, f"case d, replay {k}")
        # the target: a * direct, direct within its bar -> |target - a direct_ref| <= a gamma Sd + u |target| / (1 - u) (the one multiply)
        a = gains[:, 1].double().cpu().numpy()[:, None]
        t = target.double().cpu().numpy()[:, 0]
        bar = a * V.R.gamma(ref["nd"])[:, None] * ref["Sd"] + 2.0 ** -24 * (1.0 + 2.0 ** -23) * np.abs(t)
        err = np.abs(t - a * ref["direct"])
        print(f"case d, replay {k}: target worst |diff| / bar {np.nan_to_num(err / bar).max():.4f}")
        assert (err <= bar).all()
        if first is None:
            first = mixture.clone()
    assert not C.bit_equal(first, outs[2])                # (the second replay really made the other batch)
    assert C.bit_equal(outs[0][1], cf[100:100 + L].view(1, L))           # its dry row is the window's bits


def test_mix_loader_with_an_rir_shard_end_to_end_on_the_device(dev, wd, tmp_path):
    V.check_loader(wd, tmp_path, None, dev)


def test_three_optimiser_steps_fed_by_the_reverberant_loader(pkg, dev, wd, tmp_path):
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    cl_list, no_list, _, _ = C.corpus(tmp_path)
    rir_list, _ = V.rir_corpus(tmp_path)
    cp, npfx, rp = str(tmp_path / "speech"), str(tmp_path / "noise"), str(tmp_path / "rir")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    wd.pack_rir_shard(str(rir_list), rp)
    loader = wd.MixLoader(cp, npfx, batch_size=4, sample_length=256, snr_db=(0.0, 20.0), level_db=(-6.0, 3.0), device=dev, seed=2, steps_per_epoch=3,
                          rir_prefix=rp, p_reverb=0.8, target="early", early_ms=2.0)
    torch.manual_seed(0)
    m = pkg.Model(n_layers=3, channels_interval=4).to(dev)
    opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3, betas=(0.9, 0.999))
    before = [p.detach().clone() for p in m.parameters()]
    cfg = {"root_dir": str(tmp_path), "experiment_name": "reverb", "trainer": {"epochs": 1, "save_checkpoint_interval": 0}}
    tr = trainer_mod.Trainer(cfg, False, m, pkg.mse_loss(), opt, loader, None)
    tr.train()
    torch.cuda.synchronize()
    assert len(tr.epoch_losses) == 1 and all(math.isfinite(v) for v in tr.epoch_losses), tr.epoch_losses
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))     # the three steps moved the weights
    assert all(torch.isfinite(p).all() for p in m.parameters())
    assert set(loader.last_draw) == {"rows", "params", "gains", "rir_rows", "reverberant"}
