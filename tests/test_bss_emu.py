"""-m "not gpu": BSS Eval SDR (bss_corr_kernel / bss_solve_kernel, csrc/wunet_bss.h behind wunet_bss_sdr_forward) on the CPU emulator,
through Engine.bss_sdr and metrics.sdr / sdr_improvement, and the Trainer's "validation.sdr" key.  The yardstick is the oracle of
tests/bss_ref.py (everything in np.longdouble; np.correlate + scipy.linalg.solve_toeplitz in float64 for the size of double arithmetic's
own error); the bar is derived in tests/bss_cases.py and every case prints its figures before it asserts."""
import importlib

import numpy as np
import pytest
import torch

import bss_cases as C
import bss_ref as R
import emu_lib
import mix_cases as M
from conftest import PKG_NAME

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu_engine():
    eng_mod = importlib.import_module(PKG_NAME + ".engine")
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    return eng_mod.Engine(lib=lib_mod.declare(emu_lib.lib()), host_memory=True)


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_sdr_matches_the_long_double_oracle(emu_engine, name):
    C.check_case(name, emu_engine, CPU)


def test_the_bar_is_a_float32_rounding_bar_and_rejects_float32_accumulators(emu_engine):
    """The two conditions of tests/bss_cases.py, on the CPU."""
    C.require_long_double()
    t = C.tile(emu_engine)
    for name in sorted(C.CASES):
        ref = C.reference(name, t)
        scored = np.isfinite(ref["bar"])
        ratio = ref["second"][scored] / ref["first"][scored]
        print(f"case {name}: second term / first term per scored row {['%.2e' % v for v in ratio]} (at most 2^-8 = {2.0 ** -8:.2e})")
        assert scored.any() and (ratio <= 2.0 ** -8).all(), (name, ratio)
    d, ref = C.case("c", t), C.reference("c", t)
    for i in range(d["clean"].shape[0]):
        single = np.full(d["clean"].shape[0], np.nan)
        single[i] = R.reference_row(d["clean"][i], d["est"][i], d["n"], accumulate=np.float32)
        with pytest.raises(AssertionError):
            C.check_against(ref, single.astype(np.float32).astype(np.float64), f"case c with float32 accumulators, row {i}", rows=[i])


def test_where_the_kernel_model_lands(emu_engine):
    """The figures of tests/bss_cases.py's docstring: the float64 numpy model of the kernel's scheme and the float64 reference against
    the arbiter, in units of 2^-53 (10 / ln 10) E / R (one rounding of the residual energy), beside what 2^-8 of the float32 rounding
    is in those units.  The model's score, rounded to float32 as the kernel's is, is held to the kernel's bar."""
    C.require_long_double()
    t = C.tile(emu_engine)
    for name in sorted(C.CASES):
        d, ref = C.case(name, t), C.reference(name, t)
        rows = np.nonzero(np.isfinite(ref["bar"]))[0]
        model = np.full(d["clean"].shape[0], np.nan)
        for i in rows:
            L = d["clean"].shape[1] if d["lengths"] is None else int(d["lengths"][i])
            model[i] = R.kernel_model_row(d["clean"][i, :L], d["est"][i, :L], d["n"], t)
            unit = 2.0 ** -53 * R.K10 * ref["ratio"][i]
            print(f"case {name} row {i}: model {abs(float(np.longdouble(model[i]) - ref['arb'][i])) / unit:.1f} units, reference "
                  f"{ref['e_ref'][i] / unit:.1f} units, 2^-8 of the float32 rounding {ref['first'][i] / 256.0 / unit:.3g} units (E / R {ref['ratio'][i]:.3g})")
        C.check_against(ref, model.astype(np.float32).astype(np.float64), f"case {name}, the float64 model rounded to float32", rows=rows)


def test_the_tile_and_the_new_symbols(emu_engine):
    lib_mod = importlib.import_module(PKG_NAME + "._lib")
    for name in ("wunet_bss_sdr_scratch_bytes", "wunet_bss_sdr_forward", "wunet_bss_sdr_tile"):
        assert name in lib_mod.EXPORTS and hasattr(emu_lib.lib(), name)
    lib = emu_engine.lib
    t = lib.wunet_bss_sdr_tile(512)
    assert t >= 512 and all(lib.wunet_bss_sdr_tile(n) == t for n in (1, 5, 511))
    assert emu_engine.bss_sdr_tile() == t
    for n in (0, 513, -1):
        assert lib.wunet_bss_sdr_tile(n) == 0 and b"filter_length" in lib.wunet_last_error()
    with pytest.raises(RuntimeError, match="filter_length"):
        emu_engine.bss_sdr_tile(513)
    # one partial of r, b and E per row and segment
    assert lib.wunet_bss_sdr_scratch_bytes(3, 2 * t + 1, 512) == 3 * 3 * 1025 * 8
    assert lib.wunet_bss_sdr_scratch_bytes(1, 1, 1) == 3 * 8


def test_argument_errors_come_back_as_codes_and_messages(emu_engine):
    lib = emu_engine.lib
    rows, T = 2, 100
    rng = np.random.default_rng(3)
    clean = torch.from_numpy(rng.standard_normal((rows, T)).astype(np.float32))
    est = clean + 0.1 * torch.from_numpy(rng.standard_normal((rows, T)).astype(np.float32))
    scratch = torch.zeros(lib.wunet_bss_sdr_scratch_bytes(rows, T, 512) // 8, dtype=torch.float64)
    out = torch.zeros(rows)

    def call(**over):
        a = dict(clean=clean.data_ptr(), est=est.data_ptr(), rows=rows, T=T, lengths=None, n=512, scratch=scratch.data_ptr(), out=out.data_ptr())
        a.update(over)
        return lib.wunet_bss_sdr_forward(a["clean"], a["est"], a["rows"], a["T"], a["lengths"], a["n"], a["scratch"], a["out"], None)

    for over, word in (({"n": 0}, b"filter_length"), ({"n": 513}, b"filter_length"), ({"n": -3}, b"filter_length"), ({"rows": 65536}, b"65535"),
                       ({"rows": 0}, b"rows"), ({"T": 0}, b"row_len"), ({"T": 1 << 31}, b"2^31"), ({"clean": None}, b"null"), ({"est": None}, b"null"),
                       ({"scratch": None}, b"null"), ({"out": None}, b"null")):
        assert call(**over) == -1 and word in lib.wunet_last_error(), (over, lib.wunet_last_error())
        a = dict(rows=rows, T=T, n=512)
        a.update({k: v for k, v in over.items() if k in a})
        if set(over) & set(a):
            assert lib.wunet_bss_sdr_scratch_bytes(a["rows"], a["T"], a["n"]) == 0
    assert not out.any()                                                 # nothing ran
    assert call() == 0 and out.all()
    assert call(n=1) == 0 and call(rows=1) == 0
    # the Python face
    lengths = torch.tensor([T, T - 1], dtype=torch.int64)
    assert torch.isfinite(emu_engine.bss_sdr(clean, est, 512, lengths=lengths)).all()
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.bss_sdr(clean, est, 512, lengths=lengths.int())
    with pytest.raises(RuntimeError, match="int64"):
        emu_engine.bss_sdr(clean, est, 512, lengths=[T, T])
    with pytest.raises(RuntimeError, match="one entry per row"):
        emu_engine.bss_sdr(clean, est, 512, lengths=lengths[:1])
    with pytest.raises(RuntimeError, match="filter_length"):
        emu_engine.bss_sdr(clean, est, 513)
    with pytest.raises(RuntimeError, match="float32"):
        emu_engine.bss_sdr(clean.double(), est.double())
    with pytest.raises(RuntimeError, match="mismatch"):
        emu_engine.bss_sdr(clean, est[:, :50].contiguous())
    with pytest.raises(RuntimeError, match="out must be"):
        emu_engine.bss_sdr(clean, est, out=torch.zeros(3))
    if torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="lives on"):
            M.engine_or_default(None).bss_sdr(clean.cuda(), est.cuda(), lengths=lengths)


def test_lengths_are_clamped_on_the_device(emu_engine):
    """A length below 0 counts as 0 (NaN), one above the row as the row; a shorter length scores the truncated pair."""
    rng = np.random.default_rng(9)
    clean = torch.from_numpy(rng.standard_normal((4, 300)).astype(np.float32))
    est = clean + 0.2 * torch.from_numpy(rng.standard_normal((4, 300)).astype(np.float32))
    full = emu_engine.bss_sdr(clean, est, 32)
    got = emu_engine.bss_sdr(clean, est, 32, lengths=torch.tensor([-5, 2 ** 40, 300, 123], dtype=torch.int64))
    assert torch.isnan(got[0]) and M.bit_equal(got[1:3], full[1:3])
    assert M.bit_equal(got[3:], emu_engine.bss_sdr(clean[3:, :123].contiguous(), est[3:, :123].contiguous(), 32))


def test_metrics_sdr_and_improvement(emu_engine):
    metrics = M.metrics()
    rng = np.random.default_rng(4)
    clean = torch.from_numpy(rng.standard_normal((2, 3, 400)).astype(np.float32))
    noisy = clean + 0.5 * torch.from_numpy(rng.standard_normal((2, 3, 400)).astype(np.float32))
    better = clean + 0.1 * torch.from_numpy(rng.standard_normal((2, 3, 400)).astype(np.float32))
    v = metrics.sdr(clean, better, engine=emu_engine)
    assert v.shape == (6,) and v.dtype == torch.float32
    assert M.bit_equal(v, emu_engine.bss_sdr(clean, better, 512))
    gain = metrics.sdr_improvement(clean, noisy, better, engine=emu_engine)
    assert M.bit_equal(gain, v - metrics.sdr(clean, noisy, engine=emu_engine)) and bool((gain > 5.0).all())
    # the score forgives a filter within its taps that SI-SDR punishes: a delay of 3 samples
    delayed = torch.zeros_like(clean)
    delayed[..., 3:] = clean[..., :-3]
    assert bool((metrics.sdr(clean, delayed, filter_length=8, engine=emu_engine) > 15.0).all())
    assert bool((metrics.si_sdr(clean, delayed, engine=emu_engine) < 0.0).all())
    lengths = torch.tensor([400, 399, 1, 0, 200, 400], dtype=torch.int64)
    part = metrics.sdr(clean, better, filter_length=16, lengths=lengths, engine=emu_engine)
    assert torch.isnan(part[3]) and bool(torch.isfinite(part[[0, 1, 4, 5]]).all())
    pkg = importlib.import_module(PKG_NAME)
    assert pkg.sdr is metrics.sdr and pkg.sdr_improvement is metrics.sdr_improvement


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        M.metrics().sdr(torch.ones(1, 64), torch.ones(1, 64))


def test_trainer_validation_reports_and_scores_sdr(emu_engine, tmp_path):
    """"validation.sdr": "report" appends (mean noisy SDR, mean enhanced SDR) and leaves the score alone; "score" makes the enhanced mean
    the score, with "recordings_per_pass" through one ragged call per pass; the flags are restored; bad values raise."""
    C.check_trainer(emu_engine, CPU, tmp_path)
