"""-m "not gpu": mixtures made on the device (mix_partial_kernel / mix_apply_kernel, csrc/wunet_mix.h behind wunet_mix_windows) on the
CPU emulator, through Engine.mix_windows and waveform_dataset.MixLoader.  The yardstick is the float64 oracle of tests/mix_ref.py; the
bars are derived in tests/mix_cases.py and every case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import emu_lib
import mix_cases as C
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.fixture(scope="module")
def wd():
    return importlib.import_module(PKG_NAME + ".waveform_dataset")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_mixed_batches_match_the_float64_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


def test_gains_are_optional_and_the_tables_decide_everything(emu_engine):
    """gains = None writes the same waveforms; other table contents on the same tensors give the other batch (nothing about a row is
    kept on the host side of the call)."""
    d = C.case("a")
    mix, cl, _ = C.run(emu_engine, CPU, "a")
    cf, nf = C.guarded_flat(d["clean"], CPU), C.guarded_flat(d["noise"], CPU)
    rows, params = torch.from_numpy(np.array(d["rows"])), torch.from_numpy(np.array(d["params"]))
    m2, c2 = torch.full_like(mix, float("nan")), torch.full_like(cl, float("nan"))
    emu_engine.mix_windows(cf, nf, rows, params, m2, c2, None, peak_limit=C.PEAK)
    assert C.bit_equal(m2, mix) and C.bit_equal(c2, cl)
    rows[:, 0] += 2
    params[:, 0] -= 3.0
    emu_engine.mix_windows(cf, nf, rows, params, m2, c2, None, peak_limit=C.PEAK)
    ref = C.R.mix_reference(d["clean"], d["noise"], rows.numpy(), params.numpy(), d["L"], C.PEAK)
    g = torch.tensor(np.stack([ref["g"], ref["a"]], 1), dtype=torch.float32)       # (the gains were not asked for: the oracle's, rounded)
    C.check_against(ref, m2, c2, g, "case a, moved tables")


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    d = C.case("f")
    B, L = 5, d["L"]
    cf, nf = torch.from_numpy(np.array(d["clean"])), torch.from_numpy(np.array(d["noise"]))
    rows, params = torch.from_numpy(np.array(d["rows"])), torch.from_numpy(np.array(d["params"]))
    scr = torch.zeros(lib.wunet_mix_scratch_bytes(B, L) // 8, dtype=torch.float64)
    mix, cl = torch.zeros(B, 1, L), torch.zeros(B, 1, L)
    assert lib.wunet_mix_scratch_bytes(B, L) == B * 1 * 4 * 8 and lib.wunet_mix_scratch_bytes(2, 16384) == 2 * 16 * 4 * 8
    assert lib.wunet_mix_scratch_bytes(0, L) == 0 and lib.wunet_mix_scratch_bytes(B, 0) == 0

    def call(**over):
        a = dict(clean=cf.data_ptr(), ct=cf.numel(), noise=nf.data_ptr(), nt=nf.numel(), rows=rows.data_ptr(), params=params.data_ptr(),
                 peak=0.99, batch=B, length=L, scratch=scr.data_ptr(), mix=mix.data_ptr(), cl=cl.data_ptr(), gains=None)
        a.update(over)
        return lib.wunet_mix_windows(a["clean"], a["ct"], a["noise"], a["nt"], a["rows"], a["params"], a["peak"], a["batch"], a["length"],
                                     a["scratch"], a["mix"], a["cl"], a["gains"], None)

    for over, word in (({"batch": 0}, b"batch"), ({"length": 0}, b"length"), ({"ct": L - 1}, b"clean"), ({"nt": 0}, b"noise"),
                       ({"clean": None}, b"null"), ({"rows": None}, b"null"), ({"scratch": None}, b"null"), ({"mix": None}, b"null")):
        assert call(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not mix.any() and not cl.any()                                # nothing ran
    assert call() == 0 and mix.any() and cl.any()
    # the Python face
    g = torch.zeros(B, 2)
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.mix_windows(cf, nf, rows.int(), params, mix, cl, g)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.mix_windows(cf.double(), nf, rows, params, mix, cl, g)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.mix_windows(cf, nf, rows[:4], params, mix, cl, g)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.mix_windows(cf, nf, rows, params, mix, cl, g[:, :1].contiguous())


def test_the_new_symbols_are_exported():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_mix_scratch_bytes", "wunet_mix_windows"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)


def test_mix_loader_end_to_end(emu_engine, wd, tmp_path):
    cp, npfx = C.check_loader(wd, tmp_path, emu_engine, CPU)
    # there is no host implementation of the mix
    with pytest.raises(ValueError, match="engine"):
        wd.MixLoader(cp, npfx, batch_size=2, sample_length=256, device="cpu")
    with pytest.raises(ValueError, match="sample_length"):
        wd.MixLoader(cp, npfx, batch_size=2, sample_length=100000, engine=emu_engine)


def test_mismatched_sample_rates_raise(emu_engine, wd, tmp_path):
    cl_list, no_list, _, _ = C.corpus(tmp_path, noise_rate=8000)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx, limit=3, offset=1)
    idx = importlib.import_module("json").load(open(npfx + ".index.json"))
    assert idx["names"] == ["noise1", "noise2", "noise3"] and idx["starts"] == [0, 150, 550] and idx["sample_rate"] == 8000
    assert set(idx) == {"names", "starts", "lengths", "sample_rate"}
    with pytest.raises(ValueError, match="sample rates"):
        wd.MixLoader(cp, npfx, batch_size=2, sample_length=256, engine=emu_engine)
