"""-m "not gpu": STOI per row (stoi_tables_kernel / stoi_resample_kernel / stoi_mask_kernel / stoi_spec_kernel / stoi_segment_kernel /
stoi_final_kernel, csrc/wunet_stoi.h behind wunet_stoi_*) on the CPU emulator, through the public metrics.stoi and the trainer's
"validation.stoi" key.  The yardstick is the definition in float64 (tests/stoi_ref.py: oracle64); the bar is 4 d_ref + 2^-23 with
d_ref the distance at which two float32 computations on the CPU land from it on the same inputs, and every case prints its d and
d_ref.  Frame counts are compared exactly."""
import importlib

import pytest
import torch

import emu_lib
import stoi_cases as C
import stoi_ref as R
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("name", C.EMU_CASES)
def test_scores_and_frame_counts_match_the_float64_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


def test_two_runs_are_bit_identical_and_leading_dimensions_are_flattened(emu_engine):
    s1, f1 = C.run(emu_engine, CPU, "f")
    s2, f2 = C.run(emu_engine, CPU, "f")
    assert torch.equal(s1, s2) and torch.equal(f1, f2)
    ref = R.case_reference(*C.CASES["f"])
    c = ref["c"][:, None, :].repeat(1, 3, 1)
    e = ref["e"][:, None, :].repeat(1, 3, 1)
    s = C.metrics().stoi(c, e, sample_rate=10000, engine=emu_engine)
    assert s.shape == (6,) and torch.equal(s, s1.repeat_interleave(3))


def test_the_taps_the_engine_sends_are_the_oracles_rounded_once(emu_engine):
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    for fs in (16000, 8000):
        p, q, h = eng_mod.stoi_resampler_taps(fs)
        rp, rq, L, rh = R.taps(fs)
        assert (p, q, len(h)) == (rp, rq, 2 * L + 1) and h.dtype.name == "float32" and (h == rh.astype("float32")).all()
    assert eng_mod.stoi_resampler_taps(10000) is None
    t1 = emu_engine.stoi_tables(16000, CPU)
    assert emu_engine.stoi_tables(16000, CPU) is t1 and t1.numel() * 4 == emu_engine.lib.wunet_stoi_tables_bytes(16000)


def test_the_product_does_not_import_scipy():
    import subprocess
    import sys
    from conftest import ROOT
    code = (f"import sys, importlib; sys.path.insert(0, {ROOT!r}); e = importlib.import_module({PKG_NAME!r} + '.engine'); "
            "e.stoi_resampler_taps(16000); assert 'scipy' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300).returncode == 0


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    c, e = R.pair(2, 3000, 10000)
    tables = emu_engine.stoi_tables(10000, CPU)
    scr = torch.zeros(lib.wunet_stoi_scratch_bytes(2, 3000, 10000) // 8, dtype=torch.float64)
    out, frames = torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    args = [c.data_ptr(), e.data_ptr(), 2, 3000, 10000, tables.data_ptr(), scr.data_ptr(), out.data_ptr(), frames.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (2, 0, b"rows"),
                       (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, -16000, b"sample rate"), (4, 44100, b"taps")):
        a = list(args)
        a[k] = v
        assert lib.wunet_stoi_forward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
    assert not out.any() and not frames.any()                            # nothing ran
    assert lib.wunet_stoi_tables_bytes(0) == 0 and lib.wunet_stoi_tables_bytes(44100) == 0 and lib.wunet_stoi_scratch_bytes(0, 3000, 10000) == 0
    assert lib.wunet_stoi_tables_bytes(10000) == (256 * 2 * 224 + 256) * 4 and lib.wunet_stoi_tables_bytes(16000) == (256 * 2 * 224 + 256 + 584) * 4
    assert lib.wunet_stoi_tables_build(16000, None, 0, tables.data_ptr(), None) == -1 and b"581" in lib.wunet_last_error()
    assert lib.wunet_stoi_tables_build(10000, None, 0, None, None) == -1
    args[8] = None                                                       # frames_out is optional
    assert lib.wunet_stoi_forward(*args) == 0 and out.all() and not frames.any()
    # a row too short for one frame is not an error: 1e-5 and no frames
    for T in (1, 256, 257):
        s, f = C.metrics().stoi(c[:, :T], e[:, :T], sample_rate=10000, return_frames=True, engine=emu_engine)
        assert (s == 1e-5).all() and f.tolist() == [0, 0], (T, s, f)
    s, f = C.metrics().stoi(c[:, :300], e[:, :300], sample_rate=16000, return_frames=True, engine=emu_engine)
    assert (s == 1e-5).all() and f.tolist() == [0, 0]
    # the Python face
    with pytest.raises(RuntimeError, match="mismatch"):
        C.metrics().stoi(c, e[:1], engine=emu_engine)
    with pytest.raises(RuntimeError, match="float32"):
        C.metrics().stoi(c.double(), e.double(), engine=emu_engine)
    with pytest.raises(ValueError, match="sample rate"):
        C.metrics().stoi(c, e, sample_rate=0, engine=emu_engine)
    with pytest.raises(RuntimeError, match="taps"):
        C.metrics().stoi(c, e, sample_rate=44100, engine=emu_engine)


def test_the_new_symbols_are_exported_and_public(pkg):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_stoi_tables_bytes", "wunet_stoi_tables_build", "wunet_stoi_scratch_bytes", "wunet_stoi_forward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    assert callable(pkg.stoi)
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_stoi.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.stoi(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096))


def test_trainer_stoi_key_reports_or_scores_and_is_opt_in(emu_engine, tmp_path):
    """ "stoi": "report" leaves validation_scores bit-identical to a run without the key and fills validation_stoi with metrics.stoi
    called by hand; "stoi": "score" makes the score the mean enhanced STOI; anything else, or the key without "metric", raises."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    model_mod = importlib.import_module(PKG_NAME + ".model")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    loss_mod = importlib.import_module(PKG_NAME + ".loss")
    inference = importlib.import_module(PKG_NAME + ".inference")
    metrics = C.metrics()
    sl, fs = 64, 10000
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=4, sample_length=sl, seed=1), batch_size=2, shuffle=False)
    vloader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=2, sample_length=75 * sl + 17, seed=4, mode="validation"),
                                          batch_size=1, shuffle=False)

    def make():
        torch.manual_seed(0)
        m = model_mod.Model(n_layers=2, channels_interval=4)
        m._engine_override = emu_engine
        crit = loss_mod.si_sdr_loss()
        crit._engine_override = emu_engine
        opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3)
        opt._engine_override = emu_engine
        return m, crit, opt

    def train(name, **vkeys):
        val = {"metric": "si_sdr", "interval": 1, "custom": {"sample_length": sl, "sample_rate": fs}}
        val.update(vkeys)
        m, crit, opt = make()
        tr = trainer_mod.Trainer({"root_dir": str(tmp_path), "experiment_name": name, "trainer": {"epochs": 2, "validation": val}},
                                 False, m, crit, opt, loader, vloader)
        tr.train()
        return tr, m

    plain, _ = train("plain")
    assert plain.validation_stoi == [] and plain.validation_stoi_mode is None and len(plain.validation_scores) == 2
    rep, m = train("report", stoi="report")
    assert rep.validation_scores == plain.validation_scores and len(rep.validation_stoi) == 2
    was = m.training
    m.eval()
    with torch.no_grad():
        pairs = [(metrics.stoi(cl, mix, sample_rate=fs, engine=emu_engine), metrics.stoi(cl, inference.enhance(m, mix, sl), sample_rate=fs, engine=emu_engine))
                 for mix, cl, _ in vloader]
    m.train(was)
    noisy = torch.cat([a for a, _ in pairs]).double().mean().item()
    enh = torch.cat([b for _, b in pairs]).double().mean().item()
    assert rep.validation_stoi[-1] == (noisy, enh)                      # (the model after epoch 2 is the one the last epoch scored)
    assert 1e-5 < noisy < 1.0 and 1e-5 < enh < 1.0                      # (real scores: the recordings are long enough for segments)
    sc, _ = train("score", stoi="score")
    assert sc.validation_stoi == rep.validation_stoi and sc.validation_scores == [b for _, b in rep.validation_stoi]
    assert sc.best_score == max(sc.validation_scores) and (sc.checkpoints_dir / "best_model.tar").exists()
    m0, crit0, opt0 = make()
    for bad in ({"metric": "si_sdr", "stoi": "yes"}, {"metric": "si_sdr", "stoi": True}, {"stoi": "report"}):
        with pytest.raises(ValueError, match="validation.stoi"):
            trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": bad}}, False, m0, crit0, opt0, loader, vloader)
    with pytest.raises(ValueError, match="si_sdr"):
        trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": {"metric": "stoi"}}}, False, m0, crit0, opt0, loader, vloader)
