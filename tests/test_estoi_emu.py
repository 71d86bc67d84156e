"""-m "not gpu": ESTOI per row (estoi_segment_kernel of csrc/wunet_estoi.h in stoi_segment_kernel's place, behind wunet_estoi_forward) on
the CPU emulator, through the public metrics.stoi(extended=True) and the trainer's "validation.stoi_extended" key.  The yardstick is
the definition in float64 (tests/estoi_ref.py: oracle64); conditions and bars are those of tests/estoi_cases.py, and every case prints
its d beside d_ref.  Frame counts are compared exactly."""
import importlib

import pytest
import torch

import emu_lib
import estoi_cases as EC
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
    EC.check_case(name, emu_engine, CPU)


def test_two_runs_are_bit_identical_and_leading_dimensions_are_flattened(emu_engine):
    s1, f1 = EC.run(emu_engine, CPU, "f")
    s2, f2 = EC.run(emu_engine, CPU, "f")
    assert torch.equal(s1, s2) and torch.equal(f1, f2)
    ref = R.case_reference(*C.CASES["f"])
    c = ref["c"][:, None, :].repeat(1, 3, 1)
    e = ref["e"][:, None, :].repeat(1, 3, 1)
    s = C.metrics().stoi(c, e, sample_rate=10000, engine=emu_engine, extended=True)
    assert s.shape == (6,) and torch.equal(s, s1.repeat_interleave(3))


@pytest.mark.parametrize("name", ("a", "b"))
def test_inputs_with_4_byte_alignment_only(emu_engine, name):
    cv, ev = EC.offset_views(name, CPU)
    s, f = EC.check_case(name, emu_engine, CPU, c=cv, e=ev)
    sa, fa = EC.run(emu_engine, CPU, name)
    assert torch.equal(s, sa) and torch.equal(f, fa)


def test_the_keyword_off_is_the_call_without_it_and_on_is_another_score(emu_engine):
    """extended=False returns the bits of the call without the keyword, before and after an extended call on the same tables; the
    extended scores of the same case differ from the plain ones; both modes share one tables buffer."""
    ref = R.case_reference(*C.CASES["b"])
    plain = C.run(emu_engine, CPU, "b")
    tables = emu_engine.stoi_tables(16000, CPU)
    snapshot = tables.clone()
    ext = EC.run(emu_engine, CPU, "b")
    off = C.metrics().stoi(ref["c"], ref["e"], sample_rate=16000, return_frames=True, engine=emu_engine, extended=False)
    again = C.run(emu_engine, CPU, "b")
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1]) and torch.equal(again[0], plain[0])
    assert torch.equal(ext[1], plain[1]) and ((ext[0] - plain[0]).abs() > 0.1).all()
    assert emu_engine.stoi_tables(16000, CPU) is tables and torch.equal(tables, snapshot)
    assert emu_engine.lib.wunet_estoi_scratch_bytes(3, 9000, 16000) == emu_engine.lib.wunet_stoi_scratch_bytes(3, 9000, 16000) > 0


def test_an_all_zero_estimate_scores_exactly_zero(emu_engine):
    ref = R.case_reference(*C.CASES["a"])
    e = ref["e"].clone()
    e[0] = 0.0
    s, f = C.metrics().stoi(ref["c"], e, sample_rate=10000, return_frames=True, engine=emu_engine, extended=True)
    s_full, _ = EC.run(emu_engine, CPU, "a")
    assert s[0] == 0.0 and s[1] == s_full[1] and f.tolist() == [33, 33]
    s = C.metrics().stoi(ref["c"], torch.zeros_like(e), sample_rate=10000, engine=emu_engine, extended=True)
    assert torch.isfinite(s).all() and not s.any()


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    """wunet_estoi_forward: the cases of wunet_stoi_forward's test, with the words the STOI entry point uses."""
    lib = emu_engine.lib
    c, e = R.pair(2, 3000, 10000)
    tables = emu_engine.stoi_tables(10000, CPU)
    scr = torch.zeros(lib.wunet_estoi_scratch_bytes(2, 3000, 10000) // 8, dtype=torch.float64)
    out, frames = torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    args = [c.data_ptr(), e.data_ptr(), 2, 3000, 10000, tables.data_ptr(), scr.data_ptr(), out.data_ptr(), frames.data_ptr(), None]
    for k, v, word in ((0, None, b"null"), (1, None, b"null"), (5, None, b"null"), (6, None, b"null"), (7, None, b"null"), (2, 0, b"rows"),
                       (2, 70000, b"rows"), (4, 0, b"sample rate"), (4, -16000, b"sample rate"), (4, 44100, b"taps")):
        a = list(args)
        a[k] = v
        assert lib.wunet_estoi_forward(*a) == -1 and word in lib.wunet_last_error(), (k, v, lib.wunet_last_error())
        want = lib.wunet_last_error()
        assert lib.wunet_stoi_forward(*a) == -1 and lib.wunet_last_error() == want
    assert not out.any() and not frames.any()                            # nothing ran
    assert lib.wunet_estoi_scratch_bytes(0, 3000, 10000) == 0 and lib.wunet_estoi_scratch_bytes(2, 3000, 44100) == 0
    args[8] = None                                                       # frames_out is optional
    assert lib.wunet_estoi_forward(*args) == 0 and out.all() and not frames.any()
    # a row too short for one frame is not an error: 1e-5 and no frames
    for T in (1, 256, 257):
        s, f = C.metrics().stoi(c[:, :T], e[:, :T], sample_rate=10000, return_frames=True, engine=emu_engine, extended=True)
        assert (s == 1e-5).all() and f.tolist() == [0, 0], (T, s, f)
    # the Python face
    with pytest.raises(RuntimeError, match="mismatch"):
        C.metrics().stoi(c, e[:1], engine=emu_engine, extended=True)
    with pytest.raises(ValueError, match="sample rate"):
        C.metrics().stoi(c, e, sample_rate=0, engine=emu_engine, extended=True)
    with pytest.raises(RuntimeError, match="taps"):
        C.metrics().stoi(c, e, sample_rate=44100, engine=emu_engine, extended=True)


def test_the_new_symbols_are_exported_and_the_product_does_not_import_scipy(pkg):
    import subprocess
    import sys
    from conftest import ROOT
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_estoi_scratch_bytes", "wunet_estoi_forward", "wunet_estoi_loss_scratch_bytes", "wunet_estoi_loss_saved_bytes",
                 "wunet_estoi_loss_forward", "wunet_estoi_loss_backward"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    if not torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_estoi.py covers a GPU box)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            pkg.stoi(torch.zeros(1, 1, 4096), torch.zeros(1, 1, 4096), extended=True)
    code = (f"import sys, importlib; sys.path.insert(0, {ROOT!r}); m = importlib.import_module({PKG_NAME!r} + '.metrics'); "
            f"l = importlib.import_module({PKG_NAME!r} + '.loss'); l.stoi_loss(sample_rate=16000, extended=True); "
            "assert callable(m.stoi) and 'scipy' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=300).returncode == 0


def test_trainer_stoi_extended_key_switches_both_calls_and_is_opt_in(emu_engine, tmp_path):
    """ "stoi_extended": true with "stoi": "report" fills validation_stoi with metrics.stoi(extended=True) called by hand and leaves
    validation_scores as without it; with "score" the score is the mean ESTOI of the enhanced recordings; the key without "stoi", or with
    a value that is no bool, raises."""
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
    assert plain.validation_stoi == [] and plain.validation_stoi_extended is False
    rep, m = train("report", stoi="report", stoi_extended=True)
    assert rep.validation_stoi_extended is True and rep.validation_scores == plain.validation_scores and len(rep.validation_stoi) == 2
    was = m.training
    m.eval()
    with torch.no_grad():
        pairs = [(metrics.stoi(cl, mix, sample_rate=fs, engine=emu_engine, extended=True),
                  metrics.stoi(cl, inference.enhance(m, mix, sl), sample_rate=fs, engine=emu_engine, extended=True),
                  metrics.stoi(cl, mix, sample_rate=fs, engine=emu_engine)) for mix, cl, _ in vloader]
    m.train(was)
    noisy = torch.cat([a for a, _, _ in pairs]).double().mean().item()
    enh = torch.cat([b for _, b, _ in pairs]).double().mean().item()
    plain_noisy = torch.cat([p for _, _, p in pairs]).double().mean().item()
    assert rep.validation_stoi[-1] == (noisy, enh)                      # (the model after epoch 2 is the one the last epoch scored)
    assert 1e-5 < noisy < 1.0 and noisy != plain_noisy                  # (real scores, and not the plain ones)
    sc, _ = train("score", stoi="score", stoi_extended=True)
    assert sc.validation_stoi == rep.validation_stoi and sc.validation_scores == [b for _, b in rep.validation_stoi]
    m0, crit0, opt0 = make()
    off = trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": {"metric": "si_sdr", "stoi": "report", "stoi_extended": False}}}, False,
                              m0, crit0, opt0, loader, vloader)
    assert off.validation_stoi_extended is False and off.validation_stoi_mode == "report"
    for bad in ({"metric": "si_sdr", "stoi_extended": True}, {"metric": "si_sdr", "stoi": "report", "stoi_extended": "yes"},
                {"metric": "si_sdr", "stoi": "score", "stoi_extended": 1}):
        with pytest.raises(ValueError, match="validation.stoi_extended"):
            trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": bad}}, False, m0, crit0, opt0, loader, vloader)
    for bad in ({"metric": "si_sdr", "stoi": "yes", "stoi_extended": True}, {"metric": "si_sdr", "stoi": True}):
        with pytest.raises(ValueError, match="validation.stoi"):
            trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": bad}}, False, m0, crit0, opt0, loader, vloader)
