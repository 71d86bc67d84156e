"""-m "not gpu": reverberant speech made on the device (reverb_kernel, csrc/wunet_reverb.h behind wunet_reverb_windows; apply_level_kernel
behind wunet_apply_level) on the CPU emulator, through Engine.reverb_windows / Engine.apply_level and waveform_dataset.MixLoader with
an RIR shard.  The yardstick is the float64 oracle of tests/reverb_ref.py; the bar is derived in tests/reverb_cases.py and every case
prints its figures before it asserts."""
import importlib
import wave

import numpy as np
import pytest
import torch

import emu_lib
import mix_cases as C
import reverb_cases as V
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


@pytest.mark.parametrize("name", sorted(V.CASES))
def test_reverberant_batches_match_the_float64_oracle(emu_engine, name):
    V.check_case(name, emu_engine, CPU)


def test_apply_level_is_the_one_multiply_of_the_mix(emu_engine):
    V.check_apply_level(emu_engine, CPU)


def test_the_tables_decide_everything(emu_engine):
    """Other table contents on the same tensors give the other batch: nothing about a row is kept on the host side of the call."""
    d = V.case("c")
    B, L = d["rows"].shape[0], d["L"]
    cf, rf = C.guarded_flat(d["clean"], CPU), C.guarded_flat(d["rir"], CPU)
    rows = torch.from_numpy(np.array(d["rows"]))
    rev, direct = torch.full((B, 1, L), float("nan")), torch.full((B, 1, L), float("nan"))
    rows[:, 0] += 3
    rows[:, 3] -= 50
    emu_engine.reverb_windows(cf, rf, rows, rev, direct, early_taps=d["E"])
    ref = V.R.reverb_reference(d["clean"], d["rir"], rows.numpy(), L, d["E"])
    V.check_against(ref, d["clean"], rev, direct, "case c, moved tables")
    assert not V.bit_equal(rev, V.run(emu_engine, CPU, "c")[0])


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    d = V.case("f")
    B, L = 5, d["L"]
    cf, rf = torch.from_numpy(np.array(d["clean"])), torch.from_numpy(np.array(d["rir"]))
    rows = torch.from_numpy(np.array(d["rows"]))
    rev, direct = torch.zeros(B, 1, L), torch.zeros(B, 1, L)

    def call(**over):
        a = dict(clean=cf.data_ptr(), ct=cf.numel(), rir=rf.data_ptr(), rt=rf.numel(), rows=rows.data_ptr(), early=8, batch=B, length=L,
                 rev=rev.data_ptr(), direct=direct.data_ptr())
        a.update(over)
        return lib.wunet_reverb_windows(a["clean"], a["ct"], a["rir"], a["rt"], a["rows"], a["early"], a["batch"], a["length"], a["rev"],
                                        a["direct"], None)

    for over, word in (({"batch": 0}, b"batch"), ({"batch": -1}, b"batch"), ({"length": 0}, b"length"), ({"ct": L - 1}, b"clean"),
                       ({"rt": 0}, b"rir"), ({"rt": -3}, b"rir"), ({"clean": None}, b"null"), ({"rir": None}, b"null"), ({"rows": None}, b"null"),
                       ({"rev": None}, b"null"), ({"early": 0}, b"early_taps"), ({"early": -2}, b"early_taps")):
        assert call(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not rev.any() and not direct.any()                            # nothing ran
    assert call(direct=None, early=0) == 0 and rev.any() and not direct.any()          # early_taps is only looked at with direct
    assert call() == 0 and direct.any()
    gains, src = torch.ones(B, 2), torch.ones(B, 1, L)
    for args, word in (((None, gains.data_ptr(), B, L, src.data_ptr()), b"null"), ((src.data_ptr(), None, B, L, src.data_ptr()), b"null"),
                       ((src.data_ptr(), gains.data_ptr(), B, L, None), b"null"), ((src.data_ptr(), gains.data_ptr(), 0, L, src.data_ptr()), b"batch"),
                       ((src.data_ptr(), gains.data_ptr(), B, 0, src.data_ptr()), b"length")):
        assert lib.wunet_apply_level(*args, None) == -1 and word in lib.wunet_last_error(), (args, lib.wunet_last_error())
    # the Python face
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.reverb_windows(cf, rf, rows.int(), rev, direct)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.reverb_windows(cf.double(), rf, rows, rev, direct)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.reverb_windows(cf, rf, rows[:4], rev, direct)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.reverb_windows(cf, rf, rows, rev, direct[:, :, :32].contiguous())
    with pytest.raises(RuntimeError, match="early_taps"):
        emu_engine.reverb_windows(cf, rf, rows, rev, direct, early_taps=0)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.apply_level(src.double(), gains)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.apply_level(src, gains[:4])
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.apply_level(src, gains, torch.ones(B, 1, L + 1))


def test_the_new_symbols_are_exported():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_reverb_windows", "wunet_apply_level"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)


def test_mix_loader_with_an_rir_shard_end_to_end(emu_engine, wd, tmp_path):
    cp, npfx, rp = V.check_loader(wd, tmp_path, emu_engine, CPU)
    kw = dict(batch_size=2, sample_length=256, engine=emu_engine, rir_prefix=rp)
    with pytest.raises(ValueError, match="target"):
        wd.MixLoader(cp, npfx, target="wet", **kw)
    with pytest.raises(ValueError, match="early_ms"):
        wd.MixLoader(cp, npfx, target="early", early_ms=0.01, **kw)
    with pytest.raises(ValueError, match="p_reverb"):
        wd.MixLoader(cp, npfx, p_reverb=1.5, **kw)
    wd.MixLoader(cp, npfx, target="reverberant", early_ms=0.0, **kw)     # (early_ms belongs to the early target alone)


def test_rir_shard_errors(emu_engine, wd, tmp_path):
    cl_list, no_list, _, _ = C.corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    rng = np.random.default_rng(1)
    C._write_pcm16(tmp_path / "r16.wav", V._rir(rng, 30) * 0.5)
    C._write_pcm16(tmp_path / "r8.wav", V._rir(rng, 30) * 0.5, rate=8000)
    with wave.open(str(tmp_path / "zero.wav"), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(bytes(40))
    lst = tmp_path / "rirs.txt"
    lst.write_text(f"{tmp_path / 'r16.wav'}\n{tmp_path / 'r8.wav'}\n{tmp_path / 'zero.wav'}\n")
    with pytest.raises(ValueError, match="sample rates"):
        wd.pack_rir_shard(str(lst), str(tmp_path / "bad"))
    with pytest.raises(ValueError, match="zero.wav"):
        wd.pack_rir_shard(str(lst), str(tmp_path / "bad"), offset=2)
    for taps in (0, 16385):
        with pytest.raises(ValueError, match="max_taps"):
            wd.pack_rir_shard(str(lst), str(tmp_path / "bad"), max_taps=taps)
    # limit / offset are pack_mono_shard's; a shard at another rate than the corpus is refused by the loader
    assert wd.pack_rir_shard(str(lst), str(tmp_path / "r8"), limit=1, offset=1, max_taps=16384) == 1
    assert wd.pack_rir_shard(str(lst), str(tmp_path / "r16"), limit=1) == 1
    with pytest.raises(ValueError, match="sample rates"):
        wd.MixLoader(cp, npfx, batch_size=2, sample_length=256, engine=emu_engine, rir_prefix=str(tmp_path / "r8"))
    wd.MixLoader(cp, npfx, batch_size=2, sample_length=256, engine=emu_engine, rir_prefix=str(tmp_path / "r16"))
