"""-m "not gpu": chunked enhancement with overlap (chunk_gather_kernel / chunk_overlap_add_kernel, csrc/wunet_chunks.h behind
wunet_chunk_gather / wunet_chunk_overlap_add) on the CPU emulator, through Engine.chunk_gather / Engine.chunk_overlap_add,
inference.enhance / enhance_many and the trainer's validation.  The yardstick is the float64 oracle of tests/chunks_ref.py; the bar is
derived in tests/chunks_cases.py and every case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import chunks_cases as C
import chunks_ref as R
import emu_lib
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


def test_case_a_the_tables_at_margin_and_fade_zero_give_the_bits_of_before(emu_engine):
    """L = 64, m = f = 0, T = 150 with the real small model: the table-driven pass (enhance_many) equals enhance() at its defaults - the
    code path of before - bit for bit; so do the two entries driven by hand."""
    inf = C.inference()
    model = small_model(emu_engine)
    x = torch.from_numpy(np.array(C.recording(150))).view(1, 1, -1)
    want = inf.enhance(model, x, 64)
    assert want.shape == (1, 1, 150)
    assert C.bit_equal(inf.enhance(model, x, 64, margin=0, fade=0, window="linear", engine=emu_engine), want)
    (many,) = inf.enhance_many(model, [x], 64)
    assert C.bit_equal(many, want)
    rows, recs, total = inf.chunk_tables([150], 64)
    assert total == 152 and rows.tolist() == [[0, 150, 0], [0, 150, 64], [0, 150, 128]] and recs.tolist() == [[0, 150, 0, 3]]
    chunks = torch.full((3, 1, 64), float("nan"))
    emu_engine.chunk_gather(x.view(-1), torch.from_numpy(rows), chunks)
    padded = torch.cat([x.view(-1), torch.zeros(42)]).view(3, 1, 64)                  # the reference's padding and splitting
    assert C.bit_equal(chunks, padded)
    out = torch.full((150,), float("nan"))
    emu_engine.chunk_overlap_add(model(chunks), torch.from_numpy(recs), out, 0, 0, None, 150)
    assert C.bit_equal(out.view(1, 1, -1), want)


@pytest.mark.parametrize("window", C.WINDOWS)
@pytest.mark.parametrize("name", ["b", "c", "d", "e"])
def test_overlapped_chunks_match_the_float64_oracle(emu_engine, name, window):
    C.check_stub_case(name, emu_engine, CPU, window)


def test_case_e_unaligned_guarded_arrays(emu_engine):
    C.check_case_e_guards(emu_engine, CPU)


@pytest.mark.parametrize("window", C.WINDOWS)
def test_case_f_many_recordings_share_the_slabs(emu_engine, window):
    C.check_many(emu_engine, CPU, window)


@pytest.mark.parametrize("name", ["b", "c"])
def test_an_identity_model_gives_the_input_back(emu_engine, name):
    C.check_stub_case(name, emu_engine, CPU, "hann", identity=True)


def test_the_ramps_are_float64_rounded_once():
    inf = C.inference()
    for f in (1, 7, 16, 2048):
        for window in C.WINDOWS:
            r = inf.chunk_ramp(f, window).numpy()
            assert r.dtype == np.float32 and np.array_equal(r, R.ramp(f, window)) and (r > 0).all() and (r < 1).all()
    j = np.arange(16) + 0.5
    assert np.array_equal(R.ramp(16, "linear"), (j / 16).astype(np.float32))
    assert np.array_equal(R.ramp(16, "hann"), (np.sin(np.pi * j / 32) ** 2).astype(np.float32))


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    L, m, f, T = 64, 8, 16, 200
    inf = C.inference()
    rows_np, recs_np, _ = inf.chunk_tables([T], L, m, f)
    n = rows_np.shape[0]
    flat = torch.from_numpy(np.array(C.recording(T)))
    rows, recs = torch.from_numpy(rows_np), torch.from_numpy(recs_np)
    chunks, out, ramp = torch.zeros(n, 1, L), torch.zeros(T), inf.chunk_ramp(f)

    def gather(**over):
        a = dict(flat=flat.data_ptr(), total=T, rows=rows.data_ptr(), n=n, length=L, chunks=chunks.data_ptr())
        a.update(over)
        return lib.wunet_chunk_gather(a["flat"], a["total"], a["rows"], a["n"], a["length"], a["chunks"], None)

    for over, word in (({"n": 0}, b"n and length"), ({"length": 0}, b"n and length"), ({"total": 0}, b"flat array"), ({"flat": None}, b"null"),
                       ({"rows": None}, b"null"), ({"chunks": None}, b"null"), ({"n": 2 ** 31}, b"at most")):
        assert gather(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not chunks.any()                                               # nothing ran
    assert gather() == 0 and chunks.any()

    def ola(**over):
        a = dict(chunks=chunks.data_ptr(), n=n, length=L, margin=m, fade=f, ramp=ramp.data_ptr(), recs=recs.data_ptr(), n_recs=1, max_len=T,
                 out=out.data_ptr(), total=T)
        a.update(over)
        return lib.wunet_chunk_overlap_add(a["chunks"], a["n"], a["length"], a["margin"], a["fade"], a["ramp"], a["recs"], a["n_recs"], a["max_len"],
                                           a["out"], a["total"], None)

    for over, word in (({"n": 0}, b"n and length"), ({"length": 0}, b"n and length"), ({"margin": -1}, b"margin and fade"),
                       ({"fade": -1, "ramp": None}, b"margin and fade"), ({"margin": 24, "fade": 16}, b"hop"), ({"margin": 0, "fade": 33}, b"hop"),
                       ({"ramp": None}, b"ramp"), ({"fade": 0}, b"ramp"), ({"n_recs": 0}, b"n_recs"), ({"max_len": 0}, b"max_len"),
                       ({"total": 0}, b"flat output"), ({"chunks": None}, b"null"), ({"recs": None}, b"null"), ({"out": None}, b"null")):
        assert ola(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not out.any()                                                  # nothing ran
    assert ola() == 0 and out.any()
    # tables that do not match the arrays: rows outside [0, n), a recording outside the output, wild values - skipped, never addressed
    out.fill_(7.0)
    bad = torch.tensor([[0, T, n, 3], [0, T, -5, 3], [T, T, 0, n], [-T, T, 0, n], [2 ** 62, T, 0, n], [0, 2 ** 62, 2 ** 62, 2 ** 62], [0, T, 0, 0]],
                       dtype=torch.int64)
    assert ola(recs=bad.data_ptr(), n_recs=bad.shape[0]) == 0 and bool((out == 7.0).all())
    badrows = torch.tensor([[2 ** 62, T, 0], [0, T, -2 ** 62], [-2 ** 62, 2 ** 62, 2 ** 62], [T, T, 0], [0, -3, 0], [0, T, T]], dtype=torch.int64)
    six = torch.full((6, 1, L), float("nan"))
    assert gather(rows=badrows.data_ptr(), n=6, chunks=six.data_ptr()) == 0 and not six.any()
    # the Python face
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.chunk_gather(flat, rows.int(), chunks)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.chunk_gather(flat.double(), rows, chunks)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.chunk_gather(flat, rows[:2], chunks)
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.chunk_overlap_add(chunks, recs.int(), out, m, f, ramp, T)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.chunk_overlap_add(chunks, recs, out, m, f, ramp[:5].contiguous(), T)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.chunk_overlap_add(chunks, recs, out, m, f, None, T)
    with pytest.raises(RuntimeError, match="hop"):
        emu_engine.chunk_overlap_add(chunks, recs, out, 24, f, ramp, T)


def test_value_errors_of_the_python_surface(emu_engine):
    inf = C.inference()
    stub = C.Stub(64)
    x = torch.zeros(1, 1, 100)
    for kw in ({"margin": 24, "fade": 17}, {"margin": 32}, {"fade": 33}, {"margin": 0, "fade": 64}, {"margin": -1}, {"fade": -1},
               {"fade": 8, "window": "hamming"}, {"window": "boxcar"}, {"margin": 1.5}):
        with pytest.raises(ValueError):
            inf.enhance(stub, x, 64, engine=emu_engine, **kw)
        with pytest.raises(ValueError):
            inf.enhance_many(stub, [x], 64, engine=emu_engine, **kw)
    assert not stub.seen                                                  # nothing ran
    # the checks of before
    with pytest.raises(ValueError, match="batch size is 1"):
        inf.enhance(stub, torch.zeros(2, 1, 100), 64, margin=8, fade=16, engine=emu_engine)
    with pytest.raises(ValueError, match=r"\[1, 1, T\]"):
        inf.enhance_many(stub, [torch.zeros(2, 1, 100)], 64, engine=emu_engine)
    stub.train()
    with pytest.raises(RuntimeError, match="eval"):
        inf.enhance(stub, x, 64, margin=8, fade=16, engine=emu_engine)
    with pytest.raises(RuntimeError, match="eval"):
        inf.enhance_many(stub, [x], 64, engine=emu_engine)
    stub.eval()
    assert inf.enhance_many(stub, [], 64, engine=emu_engine) == []
    # the largest overlap the geometry allows: 2 m + 2 f = L
    assert inf.enhance(stub, x, 64, margin=16, fade=16, engine=emu_engine).shape == (1, 1, 100)
    assert inf.chunk_hop(64, 16, 16) == 16 and inf.chunk_hop(16384, 2048, 2048) == 10240 and inf.chunk_hop(64) == 64


def test_the_new_symbols_are_exported():
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_chunk_gather", "wunet_chunk_overlap_add"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)


def test_no_cpu_fallback_for_the_overlapped_chunks(pkg):
    if torch.cuda.is_available():          # (the no-GPU behaviour; tests/test_gpu_chunks.py covers a GPU box)
        return
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        C.inference().enhance(C.Stub(64), torch.zeros(1, 1, 100), 64, margin=8, fade=16)


def test_trainer_validation_with_overlap_and_recordings_per_pass(emu_engine, tmp_path):
    """Three validation recordings, "recordings_per_pass": 2 (a pass of two, a pass of one).  With margin = fade = 0 the scores are those
    of the trainer without the new keys, bit for bit; with a real overlap the epoch runs and scores; bad values raise in the constructor."""
    trainer_mod = importlib.import_module(PKG_NAME + ".trainer")
    dataset_mod = importlib.import_module(PKG_NAME + ".dataset")
    optim_mod = importlib.import_module(PKG_NAME + ".optim")
    loss_mod = importlib.import_module(PKG_NAME + ".loss")
    sl = 64
    loader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=4, sample_length=sl, seed=1), batch_size=2, shuffle=False)
    vloader = torch.utils.data.DataLoader(dataset_mod.Dataset(n_items=3, sample_length=3 * sl + 17, seed=4, mode="validation"),
                                          batch_size=1, shuffle=False)

    def trainer(name, validation):
        m = small_model(emu_engine).train()
        crit = loss_mod.si_sdr_loss()
        crit._engine_override = emu_engine
        opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3)
        opt._engine_override = emu_engine
        cfg = {"root_dir": str(tmp_path), "experiment_name": name,
               "trainer": {"epochs": 1, "validation": dict({"metric": "si_sdr", "interval": 1}, **validation)}}
        return trainer_mod.Trainer(cfg, False, m, crit, opt, loader, vloader)

    plain = trainer("plain", {"custom": {"sample_length": sl}})
    assert plain.validation_overlap == {} and plain.validation_recordings_per_pass is None
    plain.train()
    zero = trainer("zero", {"custom": {"sample_length": sl, "margin": 0, "fade": 0, "window": "linear"}, "recordings_per_pass": 2})
    zero.train()
    assert len(plain.validation_scores) == 1 and zero.validation_scores == plain.validation_scores, (zero.validation_scores, plain.validation_scores)
    over = trainer("over", {"custom": {"sample_length": sl, "margin": 8, "fade": 16}, "recordings_per_pass": 2})
    over.model.encoder[1].main[1].eval()                                              # a frozen BatchNorm layer stays frozen
    flags = [(mod, mod.training) for mod in over.model.modules()]
    score = over._validation_epoch(1)
    assert all(mod.training == was for mod, was in flags)
    assert np.isfinite(score) and over.validation_scores == [score]
    single = trainer("single", {"custom": {"sample_length": sl, "margin": 8, "fade": 16}})
    assert single._validation_epoch(1) == score                                       # one recording at a time: the same recordings, the same bits
    for validation in ({"custom": {"sample_length": sl, "margin": 24, "fade": 17}}, {"custom": {"sample_length": sl, "fade": -1}},
                       {"custom": {"sample_length": sl, "fade": 8, "window": "hamming"}}, {"custom": {"sample_length": sl, "margin": "8"}},
                       {"recordings_per_pass": 0}, {"recordings_per_pass": 1.5}, {"recordings_per_pass": True}):
        with pytest.raises(ValueError, match="validation"):
            trainer("bad", validation)
