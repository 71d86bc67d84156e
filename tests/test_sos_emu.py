"""-m "not gpu": cascades of second-order sections (sos_windows_kernel, csrc/wunet_sos.h behind wunet_sos_windows) on the CPU emulator,
through Engine.sos_windows, filters.sosfilt / random_biquads and MixLoader(eq_speech=..., eq_noise=...).  The yardstick is the oracle of
tests/sos_ref.py (the recurrence in np.longdouble, and scipy.signal.sosfilt for the size of double arithmetic's own error); the bar is
derived in tests/sos_cases.py and every case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import scipy.signal
import torch

import emu_lib
import mix_cases as M
import sos_cases as C
import sos_ref as R
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


@pytest.fixture(scope="module")
def filters():
    return importlib.import_module(PKG_NAME + ".filters")


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_filtered_windows_match_the_long_double_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


def test_the_bar_is_a_float32_rounding_bar_and_rejects_float32_state(emu_engine):
    """The two conditions of tests/sos_cases.py, on the CPU."""
    C.require_long_double()
    t, c = C.tile(emu_engine)
    for name in sorted(C.CASES):
        ref = C.reference(name, t, c)
        live = ref["rms"] > 0.0
        ratio = ref["second"][live] / (2.0 ** -24 * ref["rms"][live])
        print(f"case {name}: second term / (2^-24 rms) per row {['%.2e' % v for v in ratio]} (at most 2^-8 = {2.0 ** -8:.2e})")
        assert (ratio <= 2.0 ** -8).all(), (name, ratio)
    d, ref = C.case("c", t, c), C.reference("c", t, c)
    single = R.sos_reference(d["flat"], d["rows"], d["coefs"], d["L"], d["lead"], state_dtype=np.float32)["out"]
    for b in range(single.shape[0]):
        with pytest.raises(AssertionError):
            C.check_against(ref, single.astype(np.float32).astype(np.float64), f"case c with float32 state, row {b}", rows=[b])


def test_the_tile_and_the_new_symbols(emu_engine):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_sos_windows", "wunet_sos_tile"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    lib = emu_engine.lib
    v = lib.wunet_sos_tile(1)
    assert v > 0 and all(lib.wunet_sos_tile(s) == v for s in range(1, 9))
    assert emu_engine.sos_tile(3) == (v >> 16, v & 0xffff)
    for s in (0, 9, -1):
        assert lib.wunet_sos_tile(s) == 0 and b"sections" in lib.wunet_last_error()
    with pytest.raises(RuntimeError, match="sections"):
        emu_engine.sos_tile(9)


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    B, L, S = 3, 40, 2
    flat = torch.linspace(-1.0, 1.0, 100)
    rows = torch.tensor([[0, 0, 0, 0], [60, 50, 0, 0], [0, 5, 17, 3]], dtype=torch.int64)
    coefs = torch.tensor([[1.0, 0.1, 0.2, -0.3, 0.1]]).repeat(B, S, 1).contiguous()
    out = torch.zeros(B, 1, L)

    def call(**over):
        a = dict(flat=flat.data_ptr(), total=flat.numel(), rows=rows.data_ptr(), coefs=coefs.data_ptr(), sections=S, lead=7, batch=B, length=L,
                 out=out.data_ptr())
        a.update(over)
        return lib.wunet_sos_windows(a["flat"], a["total"], a["rows"], a["coefs"], a["sections"], a["lead"], a["batch"], a["length"], a["out"], None)

    for over, word in (({"batch": 0}, b"batch"), ({"length": 0}, b"length"), ({"batch": 65536}, b"65535"), ({"length": (1 << 24) + 1}, b"2^24"),
                       ({"sections": 0}, b"sections"), ({"sections": 9}, b"sections"), ({"lead": -1}, b"lead"), ({"lead": 8193}, b"lead"),
                       ({"total": L - 1}, b"shorter"), ({"flat": None}, b"null"), ({"rows": None}, b"null"), ({"coefs": None}, b"null"),
                       ({"out": None}, b"null")):
        assert call(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
    assert not out.any()                                                 # nothing ran
    assert call() == 0 and out.any()
    assert call(lead=8192) == 0 and call(total=L) == 0
    # the Python face
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.sos_windows(flat, rows.int(), coefs, out)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.sos_windows(flat.double(), rows, coefs, out)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.sos_windows(flat, rows, coefs.double(), out)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.sos_windows(flat, rows[:2], coefs, out)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.sos_windows(flat, rows, coefs[:, :, :4].contiguous(), out)
    with pytest.raises(RuntimeError, match="shape"):
        emu_engine.sos_windows(flat.view(1, -1), rows, coefs, out)
    with pytest.raises(RuntimeError, match="contiguous"):
        emu_engine.sos_windows(flat, rows, coefs, torch.zeros(B, 1, 2 * L)[:, :, ::2])
    with pytest.raises(RuntimeError, match="lead"):
        emu_engine.sos_windows(flat, rows, coefs, out, lead=9000)


# ---------------------------------------------------------------------------------------------- filters.sosfilt, filters.random_biquads
def _sosfilt_case(filters, engine, x, sos, label):
    """filters.sosfilt(x, sos) against the oracle run on the table as the function must normalise it."""
    C.require_long_double()
    T = x.shape[-1]
    n = x.numel() // T
    y = filters.sosfilt(x, sos, engine=engine)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.device == x.device
    s = np.asarray(sos, np.float64)
    k = (s[..., [0, 1, 2, 4, 5]] / s[..., 3:4]).astype(np.float32)
    k = k if k.ndim == 3 else np.broadcast_to(k, (n,) + k.shape)
    flat = x.reshape(-1).cpu().numpy()
    start = np.arange(n) * T
    ref = R.sos_reference(flat, np.stack([start, start, 0 * start, 0 * start], 1), k, T, 0)
    C.check_against(ref, y.reshape(n, 1, T), label)
    # and scipy itself on the coefficients the device runs (a 80 Hz high-pass moves by 1e-6 when its table is rounded to float32: that
    # is the interface, not an error): its float64 result lies within a rounding and a bit of the device's
    want = np.stack([scipy.signal.sosfilt(R.to_sos6(k[r]), flat[r * T:(r + 1) * T].astype(np.float64)) for r in range(n)])
    got = y.reshape(n, T).double().cpu().numpy()
    assert (np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 2.0 ** -24 * np.abs(want).max()).all(), label
    return y


def test_sosfilt_is_scipys_on_shared_and_per_row_tables(emu_engine, filters):
    rng = np.random.default_rng(7)
    x = torch.from_numpy(rng.uniform(-0.5, 0.5, (2, 1, 1000)).astype(np.float32))
    shared = scipy.signal.butter(4, 80.0, "highpass", fs=16000.0, output="sos")
    y = _sosfilt_case(filters, emu_engine, x, shared, "shared [S, 6]")
    per_row = np.stack([scipy.signal.butter(4, 3400.0, "lowpass", fs=16000.0, output="sos"), scipy.signal.butter(4, 300.0, "highpass", fs=16000.0, output="sos")])
    _sosfilt_case(filters, emu_engine, x, per_row, "per-row [rows, S, 6]")
    scaled = shared * np.array([2.0, -0.5])[:, None]                     # a0 = 2 and -0.5: the same filter
    assert M.bit_equal(_sosfilt_case(filters, emu_engine, x, scaled, "a0 != 1"), y)
    assert M.bit_equal(filters.sosfilt(x, torch.from_numpy(shared), engine=emu_engine), y)          # a tensor table
    assert M.bit_equal(filters.sosfilt(x[0, 0], shared, engine=emu_engine), y[0, 0])                # one row, [T]


def test_sosfilt_refuses_what_it_cannot_run(emu_engine, filters):
    x = torch.zeros(2, 1, 64)
    ok = np.array([[1.0, 0.0, 0.0, 1.0, -0.5, 0.25]])
    filters.sosfilt(x, ok, engine=emu_engine)
    for bad, word in ((np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 1.0]]), "unstable"),           # |a2| = 1
                      (np.array([[1.0, 0.0, 0.0, 1.0, 1.6, 0.5]]), "unstable"),           # |a1| > 1 + a2
                      (np.array([[1.0, 0.0, 0.0, 0.0, 0.1, 0.1]]), "a0"),
                      (np.array([[1.0, np.nan, 0.0, 1.0, 0.1, 0.1]]), "finite"),
                      (np.array([[1.0, 0.0, 0.0, np.inf, 0.1, 0.1]]), "finite"),
                      (np.tile(ok, (9, 1)), "sections"),
                      (np.tile(ok, (3, 1, 1)), "rows"),
                      (np.zeros((1, 5)), "shape")):
        with pytest.raises(ValueError, match=word):
            filters.sosfilt(x, bad, engine=emu_engine)
    with pytest.raises(ValueError, match="float32"):
        filters.sosfilt(x.double(), ok, engine=emu_engine)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback(filters):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        filters.sosfilt(torch.zeros(1, 64), np.array([[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]))


def test_random_biquads(filters):
    g = lambda seed: torch.Generator().manual_seed(seed)                  # noqa: E731
    t = filters.random_biquads(50, sections=3, spread=0.375, p=0.5, generator=g(4))
    assert t.shape == (50, 3, 6) and t.dtype == torch.float32
    assert torch.equal(t, filters.random_biquads(50, sections=3, spread=0.375, p=0.5, generator=g(4)))
    assert not torch.equal(t, filters.random_biquads(50, sections=3, spread=0.375, p=0.5, generator=g(5)))
    a1, a2 = t[..., 4].double(), t[..., 5].double()
    assert bool(((a2.abs() < 1.0) & (a1.abs() < 1.0 + a2)).all()) and bool((t[..., 0] == 1.0).all()) and bool((t[..., 3] == 1.0).all())
    assert float(t[..., [1, 2, 4, 5]].abs().max()) <= 0.375
    # the documented draw order, by hand: the rows' pass / identity draws first, then the coefficients, row-major
    gen = g(4)
    on = torch.rand(50, generator=gen, dtype=torch.float64) < 0.5
    v = (2.0 * torch.rand(50, 3, 4, generator=gen, dtype=torch.float64) - 1.0) * 0.375
    want = torch.zeros(50, 3, 6, dtype=torch.float64)
    want[..., 0] = want[..., 3] = 1.0
    want[..., 1], want[..., 2], want[..., 4], want[..., 5] = v[..., 0], v[..., 1], v[..., 2], v[..., 3]
    identity = torch.tensor([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], dtype=torch.float64)
    want[~on] = identity
    assert 0 < int(on.sum()) < 50 and torch.equal(t, want.float())
    assert bool((filters.random_biquads(7, p=0.0, generator=g(1)) == identity.float()).all())
    assert filters.random_biquads(7, generator=g(1)).shape == (7, 2, 6)
    # the extreme draws of the largest spread allowed are inside the triangle
    edge = filters.random_biquads(2000, sections=8, spread=0.4999, generator=g(2))
    assert bool((edge[..., 4].double().abs() < 1.0 + edge[..., 5].double()).all())
    for kw in ({"spread": 0.5}, {"spread": -0.1}, {"sections": 9}, {"sections": 0}, {"p": 1.5}):
        with pytest.raises(ValueError):
            filters.random_biquads(4, **kw)
    with pytest.raises(ValueError):
        filters.random_biquads(0)


# ---------------------------------------------------------------------------------------------- MixLoader with the equalisers
def test_mix_loader_with_equalisers_end_to_end(emu_engine, wd, tmp_path):
    C.check_loader(wd, tmp_path, emu_engine, CPU)


def test_mix_loader_with_equalisers_and_an_rir_shard(emu_engine, wd, tmp_path):
    C.check_rir_loader(wd, tmp_path, emu_engine, CPU)


def test_mix_loader_refuses_bad_equaliser_options(emu_engine, wd, tmp_path):
    cl_list, no_list, _, _ = M.corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    kw = dict(batch_size=2, sample_length=256, engine=emu_engine)
    for bad in ({"eq_speech": {"spread": 0.6}}, {"eq_noise": {"sections": 9}}, {"eq_speech": {"order": 2}}, {"eq_noise": {}, "eq_lead": 9000},
                {"eq_speech": {}, "eq_lead": -1}):
        with pytest.raises(ValueError):
            wd.MixLoader(cp, npfx, **kw, **bad)
    wd.pack_mono_shard(str(no_list), npfx + "_short", limit=2)             # 20 + 150 samples of noise: less than one window
    wd.MixLoader(cp, npfx + "_short", eq_speech={}, **kw)
    with pytest.raises(ValueError, match="noise shard"):
        wd.MixLoader(cp, npfx + "_short", eq_noise={}, **kw)
