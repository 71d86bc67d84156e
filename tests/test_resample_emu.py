"""-m "not gpu": sample-rate conversion (resample_rows_kernel, csrc/wunet_resample.h behind wunet_resample_rows) on the CPU emulator,
through Engine.resample_rows, resample.resample / resample_many, inference.enhance / enhance_many, the trainer's validation and the
pack_* functions.  The yardstick is the float64 oracle of tests/resample_ref.py; the bar is derived in tests/resample_cases.py and every
case prints its figures before it asserts."""
import importlib
import json
import struct

import numpy as np
import pytest
import torch

import chunks_cases as CC
import emu_lib
import resample_cases as C
import resample_ref as R
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


def small_model(emu_engine, seed=0):
    torch.manual_seed(seed)
    m = importlib.import_module(PKG_NAME + ".model").Model(n_layers=2, channels_interval=4)
    m._engine_override = emu_engine
    return m.eval()


def test_the_oracle_and_the_filter_agree_with_scipy():
    signal = pytest.importorskip("scipy.signal")
    rs = C.resample_mod()
    for rate_in, rate_out, T in ((44100, 16000, 1000), (16000, 48000, 300), (48000, 16000, 1000), (16000, 11025, 500)):
        up, down, h = rs.resample_taps(rate_in, rate_out)
        M, L = max(up, down), 10 * max(up, down)
        design = rs.design(up, down)
        want = signal.firwin(2 * L + 1, 1.0 / M, window=("kaiser", 5.0)) * up
        assert h.dtype == np.float32 and len(h) == 2 * L + 1 and np.array_equal(h, design.astype(np.float32))
        print(f"{up} / {down}: max |design - up firwin| {np.abs(design - want).max():.3g}")
        assert np.abs(design - want).max() <= 1e-15 * up
        x = np.array(C.signal(T), np.float64)
        y, _ = R.resample(x, up, down, h)
        ref = signal.resample_poly(x, up, down, window=h.astype(np.float64) / up)
        print(f"{up} / {down}: max |oracle - resample_poly| {np.abs(y - ref).max():.3g}")
        assert y.shape == ref.shape and np.abs(y - ref).max() <= 1e-14
    # the default design itself: resample_poly without a window argument
    x = np.array(C.signal(1000), np.float64)
    up, down, h = rs.resample_taps(48000, 16000)
    assert np.abs(R.resample(x, up, down, h)[0] - signal.resample_poly(x, up, down)).max() <= 2.0 ** -22


def test_the_filter_and_the_lengths():
    rs = C.resample_mod()
    for (rate_in, rate_out), (up, down, taps) in {(48000, 16000): (1, 3, 61), (16000, 48000): (3, 1, 61), (32000, 16000): (1, 2, 41),
                                                  (44100, 16000): (160, 441, 8821), (22050, 16000): (320, 441, 8821),
                                                  (11025, 16000): (640, 441, 12801), (16000, 11025): (441, 640, 12801)}.items():
        u, d, h = rs.resample_taps(rate_in, rate_out)
        assert (u, d, len(h)) == (up, down, taps) and not h.flags.writeable
        assert rs.resample_taps(rate_in, rate_out)[2] is h                                   # cached per pair
        assert abs(float(h.astype(np.float64).sum()) - up) < 1e-5 * up                       # unit gain at DC, times up
        assert np.array_equal(h, h[::-1])
    assert rs.resampled_length(1000, 48000, 16000) == 334 and rs.resampled_length(3000, 44100, 16000) == 1089
    assert rs.resampled_length(334, 16000, 48000) == 1002 and rs.resampled_length(5, 16000, 16000) == 5
    for T in (1, 2, 999, 1000, 44101):                                                       # the way back is never short
        for rate in (48000, 44100, 22050, 11025, 8000):
            assert rs.resampled_length(rs.resampled_length(T, rate, 16000), 16000, rate) >= T


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_cases_a_to_e_and_h_match_the_float64_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


@pytest.mark.parametrize("rates", C.RAGGED_RATES)
def test_case_f_a_ragged_table_in_guarded_arrays(emu_engine, rates):
    C.check_case_f(emu_engine, CPU, rates)


@pytest.mark.parametrize("rates", C.RAGGED_RATES + ((16000, 44100),))
def test_case_g_output_lengths_off_the_natural_one_and_at_the_block_size(emu_engine, rates):
    C.check_case_g(emu_engine, CPU, rates)


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    rs = C.resample_mod()
    up, down, h = rs.resample_taps(48000, 16000)
    T, To = 100, 34
    x = torch.from_numpy(np.array(C.signal(T)))
    taps = torch.from_numpy(h.copy())
    rows = torch.tensor([[0, T, 0, To]], dtype=torch.int64)
    out = torch.zeros(To)

    def call(**over):
        a = dict(x=x.data_ptr(), in_total=T, rows=rows.data_ptr(), n=1, max_out=To, up=up, down=down, taps=taps.data_ptr(), n_taps=len(h),
                 out=out.data_ptr(), out_total=To)
        a.update(over)
        return lib.wunet_resample_rows(a["x"], a["in_total"], a["rows"], a["n"], a["max_out"], a["up"], a["down"], a["taps"], a["n_taps"],
                                       a["out"], a["out_total"], None)

    for over, word in (({"x": None}, b"null"), ({"rows": None}, b"null"), ({"taps": None}, b"null"), ({"out": None}, b"null"),
                       ({"n": 0}, b"n and max_out"), ({"max_out": 0}, b"n and max_out"), ({"up": 0}, b"up and down"), ({"down": -1}, b"up and down"),
                       ({"up": 2, "down": 6}, b"coprime"), ({"up": 441, "down": 441}, b"coprime"), ({"n_taps": 60}, b"odd"), ({"n_taps": 0}, b"odd"),
                       ({"n_taps": 12803}, b"cap"), ({"up": 641, "down": 1}, b"cap"), ({"up": 1, "down": 641}, b"cap"),
                       ({"n": 2 ** 31}, b"at most"), ({"in_total": 0}, b"size"), ({"out_total": 2 ** 50}, b"size")):
        assert call(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not out.any()                                                  # nothing ran
    assert lib.wunet_resample_tile(2, 6, 61) == 0 and b"coprime" in lib.wunet_last_error()
    assert lib.wunet_resample_tile(1, 3, 12803) == 0 and lib.wunet_resample_tile(1, 3, 61) > 0
    assert call() == 0 and out.any()
    # wild rows are skipped, never addressed: the output keeps its fill value
    out.fill_(7.0)
    wild = torch.tensor([[-1, T, 0, To], [0, -1, 0, To], [0, T, -1, To], [0, T, 0, -1], [0, T, 0, 0], [1, T, 0, To], [0, T + 1, 0, To],
                         [0, T, 1, To], [0, T, 0, To + 1], [T + 1, 0, 0, To], [0, T, To + 1, 1], [2 ** 62, T, 0, To], [0, 2 ** 62, 0, To],
                         [0, T, 2 ** 62, To], [0, T, 0, 2 ** 62], [2 ** 62, 2 ** 62, 2 ** 62, 2 ** 62], [-2 ** 62, 2 ** 62, -2 ** 62, 2 ** 62]],
                        dtype=torch.int64)
    assert call(rows=wild.data_ptr(), n=wild.shape[0]) == 0 and bool((out == 7.0).all())
    # a good row among wild ones is still served
    mixed = torch.cat([wild[:3], rows, wild[3:6]])
    assert call(rows=mixed.data_ptr(), n=mixed.shape[0]) == 0
    ref, bar = C.reference(48000, 16000, T)
    C.check_against(ref, bar, out, "one good row among wild ones")
    # the Python face
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.resample_rows(x, rows.int(), out, 48000, 16000, To)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.resample_rows(x.double(), rows, out, 48000, 16000, To)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.resample_rows(x, rows, out.double(), 48000, 16000, To)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.resample_rows(x, rows[:, :3].contiguous(), out, 48000, 16000, To)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.resample_rows(x.view(1, -1), rows, out, 48000, 16000, To)
    with pytest.raises(RuntimeError, match="max_out"):
        emu_engine.resample_rows(x, rows, out, 48000, 16000, 0)
    with pytest.raises(ValueError, match="taps"):
        emu_engine.resample_rows(x, rows, out, 44100, 16001, To)


def test_the_new_symbols_are_exported():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_resample_rows", "wunet_resample_tile"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)


def test_equal_rates_return_the_input_and_bad_rates_raise(emu_engine):
    rs = C.resample_mod()
    x = torch.from_numpy(np.array(C.signal(100)))
    assert rs.resample(x, 16000, 16000, engine=emu_engine) is x and rs.resample(x, 44100, 44100) is x
    recs = [x, x.view(1, 1, -1)]
    assert all(a is b for a, b in zip(rs.resample_many(recs, 8000, 8000, engine=emu_engine), recs))
    assert rs.resample_many([], 48000, 16000, engine=emu_engine) == []
    for bad in (0, -16000, 16000.0, "16000", True, None):
        with pytest.raises(ValueError, match="positive integer"):
            rs.resample(x, bad, 16000, engine=emu_engine)
        with pytest.raises(ValueError, match="positive integer"):
            rs.resample_taps(16000, bad)
    with pytest.raises(ValueError, match="taps"):
        rs.resample(x, 44100, 16001, engine=emu_engine)
    with pytest.raises(ValueError, match="float32"):
        rs.resample(x.double(), 48000, 16000, engine=emu_engine)
    with pytest.raises(ValueError, match=r"\[1, 1, T\]"):
        rs.resample_many([torch.zeros(2, 1, 10)], 48000, 16000, engine=emu_engine)
    # [..., T]: every row of the last dimension; `length` truncates
    y = rs.resample(torch.from_numpy(np.stack([C.signal(1000), C.signal(1000, seed=1)])).view(2, 1, 1000), 3, 1, engine=emu_engine)
    assert y.shape == (2, 1, 334)
    C.check_against(*C.reference(3, 1, 1000, 1), y[1, 0], "[2, 1, T], row 1")
    z = rs.resample(x, 16000, 48000, engine=emu_engine, length=250)
    assert z.shape == (250,) and CC.bit_equal(z, rs.resample(x, 16000, 48000, engine=emu_engine)[:250])


def test_no_cpu_fallback_for_resampling(pkg):
    if torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_resample.py covers a GPU box)
        return
    rs = C.resample_mod()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.resample(torch.zeros(100), 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        rs.resample_many([torch.zeros(100)], 48000, 16000)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.inference().enhance(CC.Stub(64), torch.zeros(1, 1, 100), 64, sample_rate=48000)


# ------------------------------------------------------------------------------------------------ through the surface
@pytest.mark.parametrize("sample_rate", [48000, 44100])
def test_enhance_at_another_rate_is_down_then_up(emu_engine, sample_rate):
    out, stub = C.check_enhance_round_trip(emu_engine, CPU, sample_rate)
    Tm = C.resample_mod().resampled_length(1000, sample_rate, 16000)
    assert sum(s.shape[0] for s in stub.seen) == -(-Tm // 64)                         # the model ran on chunks at its own rate
    again, _ = C.check_enhance_round_trip(emu_engine, CPU, sample_rate)             # two runs, the same bits
    assert CC.bit_equal(out, again)


def test_enhance_without_a_rate_or_at_the_models_rate_is_the_call_of_before(emu_engine):
    inf = C.inference()
    model = small_model(emu_engine)
    x = torch.from_numpy(np.array(C.signal(150))).view(1, 1, -1)
    want = inf.enhance(model, x, 64)
    assert CC.bit_equal(inf.enhance(model, x, 64, sample_rate=None), want)
    assert CC.bit_equal(inf.enhance(model, x, 64, sample_rate=16000), want)
    assert CC.bit_equal(inf.enhance(model, x, 64, sample_rate=8000, model_rate=8000), want)
    over = inf.enhance(model, x, 64, margin=8, fade=16, engine=emu_engine)
    assert CC.bit_equal(inf.enhance(model, x, 64, margin=8, fade=16, engine=emu_engine, sample_rate=16000, model_rate=16000), over)
    many = inf.enhance_many(model, [x, x[..., :70]], 64)
    for rates in (None, 16000, [16000, 16000]):
        again = inf.enhance_many(model, [x, x[..., :70]], 64, sample_rates=rates)
        assert all(CC.bit_equal(a, b) for a, b in zip(again, many))


def test_enhance_many_over_three_rates_at_once(emu_engine):
    """Recordings at 16, 44.1 and 48 kHz (two of them at 48) in one call: each gets the bits enhance gives it alone; the model sees
    slabs that recordings of different rates share."""
    inf = C.inference()
    rates = [48000, 16000, 44100, 48000, 16000]
    xs = [torch.from_numpy(np.array(C.signal(T, seed=2))) for T in (1000, 150, 700, 333, 64)]
    recs = [x.view(1, 1, -1) if k % 2 == 0 else x for k, x in enumerate(xs)]
    stub = CC.Stub(64, identity=True)
    outs = inf.enhance_many(stub, recs, 64, max_batch=3, engine=emu_engine, sample_rates=rates)
    assert len(stub.seen) > 1 and max(s.shape[0] for s in stub.seen) <= 3
    for k, (rec, rate, out) in enumerate(zip(recs, rates, outs)):
        assert out.shape == rec.shape
        alone = inf.enhance(CC.Stub(64, identity=True), rec.view(1, 1, -1), 64, max_batch=3, engine=emu_engine, sample_rate=rate)
        assert CC.bit_equal(out.reshape(-1), alone.reshape(-1)), f"recording {k} at {rate} Hz: enhance_many differs from enhance"
    # overlapped chunks, a non-identity stub: the same
    outs = inf.enhance_many(CC.Stub(64), recs, 64, max_batch=3, margin=8, fade=16, engine=emu_engine, sample_rates=rates)
    for k, (rec, rate, out) in enumerate(zip(recs, rates, outs)):
        alone = inf.enhance(CC.Stub(64), rec.view(1, 1, -1), 64, margin=8, fade=16, engine=emu_engine, sample_rate=rate)
        assert CC.bit_equal(out.reshape(-1), alone.reshape(-1)), f"recording {k} at {rate} Hz, overlapped: enhance_many differs from enhance"


def test_value_errors_of_the_rate_keywords(emu_engine):
    inf = C.inference()
    stub = CC.Stub(64)
    x = torch.zeros(1, 1, 100)
    for kw in ({"sample_rate": 0}, {"sample_rate": -48000}, {"sample_rate": 48000.0}, {"sample_rate": 48000, "model_rate": 0},
               {"sample_rate": 44100, "model_rate": 16001}, {"sample_rate": "48000"}):
        with pytest.raises(ValueError):
            inf.enhance(stub, x, 64, engine=emu_engine, **kw)
    for kw in ({"sample_rates": 0}, {"sample_rates": [48000]}, {"sample_rates": [48000, 16000, 16000]}, {"sample_rates": [48000, -1]},
               {"sample_rates": [44100, 16000], "model_rate": 16001}, {"sample_rates": [48000, None]}, {"sample_rates": 48000, "model_rate": -5}):
        with pytest.raises(ValueError):
            inf.enhance_many(stub, [x, x], 64, engine=emu_engine, **kw)
    assert not stub.seen                                                  # nothing ran


def test_trainer_validation_at_another_rate(emu_engine, tmp_path):
    """Validation files at 48 kHz, the model at 16 kHz: the epoch runs and scores, one recording at a time and several per pass alike.
    With model_rate == sample_rate the scores are those of the trainer without the key, bit for bit; bad values raise in the constructor."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    loss_mod = importlib.import_module(PKG_NAME + ".loss")
    sl = 64
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=4, sample_length=sl, seed=1), batch_size=2, shuffle=False)
    vloader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=3, sample_length=9 * sl + 17, seed=4, mode="validation"),
                                          batch_size=1, shuffle=False)

    def trainer(name, custom, **validation):
        m = small_model(emu_engine).train()
        crit = loss_mod.si_sdr_loss()
        crit._engine_override = emu_engine
        opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3)
        opt._engine_override = emu_engine
        cfg = {"root_dir": str(tmp_path), "experiment_name": name,
               "trainer": {"epochs": 1, "validation": dict({"metric": "si_sdr", "interval": 1, "custom": dict({"sample_length": sl}, **custom)}, **validation)}}
        return trainer_mod.Trainer(cfg, False, m, crit, opt, loader, vloader)

    plain = trainer("plain", {"sample_rate": 48000})
    assert plain.validation_rates == {}
    plain.train()
    same = trainer("same", {"sample_rate": 48000, "model_rate": 48000})
    assert same.validation_rates == {}
    same.train()
    assert len(plain.validation_scores) == 1 and same.validation_scores == plain.validation_scores
    other = trainer("other", {"sample_rate": 48000, "model_rate": 16000})
    assert other.validation_rates == {"sample_rate": 48000, "model_rate": 16000}
    score = other._validation_epoch(1)
    assert np.isfinite(score) and other.validation_scores == [score] and score != plain.validation_scores[0]
    passes = trainer("passes", {"sample_rate": 48000, "model_rate": 16000, "margin": 8, "fade": 16}, recordings_per_pass=2)
    single = trainer("single", {"sample_rate": 48000, "model_rate": 16000, "margin": 8, "fade": 16})
    assert np.isfinite(passes._validation_epoch(1)) and passes.validation_scores == [single._validation_epoch(1)]
    for custom in ({"model_rate": 0}, {"model_rate": -16000}, {"model_rate": "16000"}, {"model_rate": 16000.0}, {"model_rate": True},
                   {"sample_rate": 44100, "model_rate": 16001}):
        with pytest.raises(ValueError, match="validation"):
            trainer("bad", custom)


def write_wav(path, x, rate):
    """16-bit PCM mono."""
    pcm = np.clip(np.round(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype("<i2").tobytes()
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(pcm)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16))
        f.write(b"data" + struct.pack("<I", len(pcm)) + pcm)


def test_the_pack_functions_bring_files_to_the_shards_rate(emu_engine, tmp_path):
    wd = importlib.import_module(PKG_NAME + ".waveform_dataset")
    rs = C.resample_mod()
    files = {"a16": (16000, 500), "b48": (48000, 1200), "c44": (44100, 900)}
    for name, (rate, T) in files.items():
        write_wav(str(tmp_path / (name + ".wav")), 0.5 * C.signal(T, seed=3), rate)
        write_wav(str(tmp_path / (name + "_clean.wav")), 0.25 * C.signal(T, seed=4), rate)
    mono = tmp_path / "mono.txt"
    mono.write_text("".join(f"{tmp_path / (n + '.wav')}\n" for n in files))
    pairs = tmp_path / "pairs.txt"
    pairs.write_text("".join(f"{tmp_path / (n + '.wav')} {tmp_path / (n + '_clean.wav')}\n" for n in files))

    def expect(path, rate):
        x, r = wd.read_wav(str(path))
        assert r == rate
        if rate == 16000:
            return x.astype(np.float64), np.zeros(len(x))
        up, down, h = rs.resample_taps(rate, 16000)
        y, s = R.resample(x, up, down, h)
        return y, C.bar_of(y, s, up, len(h))

    def check_shard(data, index, suffix, label):
        assert index["sample_rate"] == 16000 and index["names"] == list(files)
        assert index["lengths"] == [rs.resampled_length(T, rate, 16000) for rate, T in files.values()]
        assert index["starts"] == [0] + list(np.cumsum(index["lengths"])[:-1]) and len(data) == sum(index["lengths"])
        for name, start, n, (rate, _) in zip(index["names"], index["starts"], index["lengths"], files.values()):
            ref, bar = expect(tmp_path / (name + suffix + ".wav"), rate)
            C.check_against(ref, bar, torch.from_numpy(data[start:start + n].copy()), f"{label} {name}")

    assert wd.pack_mono_shard(str(mono), str(tmp_path / "m"), sample_rate=16000, engine=emu_engine) == 3
    check_shard(np.fromfile(str(tmp_path / "m.f32"), np.float32), json.load(open(tmp_path / "m.index.json")), "", "pack_mono_shard")
    assert wd.pack_shard(str(pairs), str(tmp_path / "p"), sample_rate=16000, engine=emu_engine) == 3
    index = json.load(open(tmp_path / "p.index.json"))
    check_shard(np.fromfile(str(tmp_path / "p.noisy.f32"), np.float32), index, "", "pack_shard noisy")
    check_shard(np.fromfile(str(tmp_path / "p.clean.f32"), np.float32), index, "_clean", "pack_shard clean")
    # a response at 48 kHz lands in a 16 kHz shard cut at its direct path, found at the shard's rate
    h48 = np.zeros(600, np.float32)
    h48[30:] = (0.9 * np.exp(-np.arange(570) / 100.0) * np.sign(C.signal(570, seed=5))).astype(np.float32)
    write_wav(str(tmp_path / "rir48.wav"), h48, 48000)
    rirs = tmp_path / "rirs.txt"
    rirs.write_text(f"{tmp_path / 'rir48.wav'}\n")
    assert wd.pack_rir_shard(str(rirs), str(tmp_path / "r"), max_taps=64, sample_rate=16000, engine=emu_engine) == 1
    ridx, rdata = json.load(open(tmp_path / "r.index.json")), np.fromfile(str(tmp_path / "r.f32"), np.float32)
    assert ridx["sample_rate"] == 16000 and ridx["lengths"] == [64] and rdata[0] == 1.0
    ref, _ = expect(tmp_path / "rir48.wav", 48000)
    p = int(np.argmax(np.abs(ref)))
    assert np.abs(rdata - ref[p:p + 64] / ref[p]).max() < 1e-5
    # without the keyword a list of mixed rates fails as before, and a list at one rate records that rate
    with pytest.raises(AssertionError, match="mixed sample rates"):
        wd.pack_mono_shard(str(mono), str(tmp_path / "m2"))
    with pytest.raises(AssertionError, match="mixed sample rates"):
        wd.pack_shard(str(pairs), str(tmp_path / "p2"))
    one = tmp_path / "one.txt"
    one.write_text(f"{tmp_path / 'b48.wav'}\n")
    assert wd.pack_mono_shard(str(one), str(tmp_path / "o")) == 1 and json.load(open(tmp_path / "o.index.json"))["sample_rate"] == 48000
    assert np.array_equal(np.fromfile(str(tmp_path / "o.f32"), np.float32), wd.read_wav(str(tmp_path / "b48.wav"))[0])
    for bad in (0, -16000, "16000"):
        with pytest.raises(ValueError):
            wd.pack_mono_shard(str(one), str(tmp_path / "bad"), sample_rate=bad, engine=emu_engine)
