"""The case table of sample-rate conversion on the device (resample_rows_kernel behind wunet_resample_rows, Engine.resample_rows,
resample.resample / resample_many, inference.enhance(sample_rate=)), shared by tests/test_resample_emu.py (CPU emulator) and
tests/test_gpu_resample.py (MI355X): what runs, on which tensors, and the checks against the float64 oracle of tests/resample_ref.py.
`engine` None = the product's default engine.

The bar (derived, not measured).  The kernel's result is fl32(S_d): S_d the sum, in double and in increasing j, of the K terms
h'[phase + up j] x[i_hi - j], each product of two float32 values exact in double.  With s = sum |h'| |x| over those terms and the exact
sum S:  |S_d - S| <= (K - 1) 2^-53 s to first order, and the oracle, a double sum of the same products in another order, is as far from
S, so |S_d - ref| <= K 2^-52 s =: d.  The one rounding to float32 adds 2^-24 |S_d| <= 2^-24 (|ref| + d) in the normal range and at most
2^-150, half a subnormal step, below it (no case here gets there; the term costs nothing):
    |dev - ref| <= 2^-24 |ref| + (1 + 2^-24) K 2^-52 s + 2^-150,     K = (n_taps - 1) / up + 1, the most taps any phase has.

Two stages (enhance at another rate with an identity model: down to the model's rate with filter 1, back with filter 2, the oracle
running both in float64 without the rounding between them).  The device's stage-1 output is y1 = ref1 + e1 with |e1| <= bar1, the bar
above, sample by sample.  Stage 2 is linear: on y1 it gives, exactly, ref + sum h2 e1, and |sum h2 e1| <= sum |h2| bar1 =: c, the
oracle's own |h| |x| sum with bar1 as the signal.  The device's stage 2 is then within the one-stage bar of that, taken for its input y1:
    |dev - ref| <= c + 2^-24 (|ref| + c) + (1 + 2^-24) K2 2^-52 sum |h2| (|ref1| + bar1) + 2^-150.
Every check prints the worst ratio |dev - ref| / bar before it asserts."""
import functools
import importlib

import numpy as np
import torch

import resample_ref as R
from chunks_cases import Stub, bit_equal
from conftest import PKG_NAME

# name: (rate_in, rate_out, T_in) - up / down = rate_out / rate_in in lowest terms
CASES = {
    "a": (3, 1, 1000),            # 1 / 3: one phase, every tap for every output
    "b": (1, 3, 333),             # 3 / 1: upsampling, 21 taps per output
    "c": (44100, 16000, 3000),    # 160 / 441: all 160 phases, the 8 821-tap table, 3000 -> 1089
    "d": (16000, 44100, 1089),    # 441 / 160: the way back, more phases than a block has threads
    "e": (11025, 16000, 700),     # 640 / 441: the largest table, 12 801 taps
    "h": (640, 1, 6000),          # 1 / 640: 12 801 taps per output and 640 inputs per output - the tile shrinks to 4 outputs, the block
                                  # asks for 110 KiB of LDS, above the 64 KiB a kernel gets without the launcher's opt-in
}
RAGGED = (1, 2, 7, 255, 256, 257, 1000)      # case f: rows shorter than the half filter among them
RAGGED_RATES = ((3, 1), (44100, 16000))      # 1 / 3 and 160 / 441


def resample_mod():
    return importlib.import_module(PKG_NAME + ".resample")


def inference():
    return importlib.import_module(PKG_NAME + ".inference")


def engine_or_default(engine):
    return engine if engine is not None else importlib.import_module(PKG_NAME + ".engine").default_engine()


@functools.lru_cache(maxsize=None)
def signal(T, seed=0):
    """float32 [T] in [-1, 1) - built once, shared, never modified."""
    x = np.random.default_rng(7000 * seed + T).uniform(-1.0, 1.0, T).astype(np.float32)
    x.setflags(write=False)
    return x


def terms(up, n_taps):
    return (n_taps - 1) // up + 1


def bar_of(ref, s, up, n_taps):
    """The one-stage bar of this file's docstring."""
    d = terms(up, n_taps) * 2.0 ** -52 * s
    return 2.0 ** -24 * np.abs(ref) + (1.0 + 2.0 ** -24) * d + 2.0 ** -150


@functools.lru_cache(maxsize=None)
def reference(rate_in, rate_out, T, seed=0, T_out=None):
    """(ref, bar) of signal(T, seed) at the other rate - computed once per case, shared by the tests, never modified."""
    up, down, h = resample_mod().resample_taps(rate_in, rate_out)
    y, s = R.resample(signal(T, seed), up, down, h, T_out)
    bar = bar_of(y, s, up, len(h))
    y.setflags(write=False)
    bar.setflags(write=False)
    return y, bar


def check_against(ref, bar, out, label):
    o = out.detach().cpu().reshape(-1).double().numpy()
    assert o.shape == ref.shape, (label, o.shape, ref.shape)
    assert np.isfinite(o).all(), f"{label}: NaN / Inf (or a sample never written)"
    d = np.abs(o - ref)
    with np.errstate(divide="ignore", invalid="ignore"):          # (a bar of 0 asks for the reference's own bits: 0 / 0 counts as 0)
        worst = float(np.nan_to_num(d / bar, nan=0.0, posinf=np.inf).max()) if d.size else 0.0
    print(f"{label}: {len(o)} samples, max |ref| {np.abs(ref).max():.3g}, max |dev - ref| {d.max():.3g}, worst |dev - ref| / bar {worst:.3f}")
    assert (d <= bar).all(), (label, worst)


def check_case(name, engine, device):
    """Cases a - e and h through resample.resample on two rows [2, T]: shape, the bar on every sample, two runs bit-equal."""
    rate_in, rate_out, T = CASES[name]
    rs = resample_mod()
    up, down, h = rs.resample_taps(rate_in, rate_out)
    x = torch.from_numpy(np.stack([signal(T), signal(T, seed=1)])).to(device)
    out = rs.resample(x, rate_in, rate_out, engine=engine)
    To = rs.resampled_length(T, rate_in, rate_out)
    assert out.shape == (2, To) and out.dtype == torch.float32 and To == R.natural_length(T, up, down)
    print(f"case {name}: {up} / {down}, {len(h)} taps, at most {terms(up, len(h))} per output, T {T} -> {To}, "
          f"{rs.outputs_per_block(rate_in, rate_out, engine)} outputs per block")
    for row in range(2):
        ref, bar = reference(rate_in, rate_out, T, row)
        check_against(ref, bar, out[row], f"case {name} row {row}")
    again = rs.resample(x, rate_in, rate_out, engine=engine)
    assert bit_equal(out, again), f"case {name}: two runs differ"
    if name == "c":
        assert (up, down, len(h), To) == (160, 441, 8821, 1089)
    if name == "e":
        assert (up, down, len(h)) == (640, 441, 12801)
    if name == "h":
        assert (up, down, len(h), To) == (1, 640, 12801, 10) and rs.outputs_per_block(rate_in, rate_out, engine) == 4


def odd_layout(lengths, first=1):
    """Starts for rows of `lengths` samples in one flat array: every start odd (4-byte aligned only), at least one guard sample between
    rows.  Returns (starts, total)."""
    starts, pos = [], first
    for T in lengths:
        if pos % 2 == 0:
            pos += 1
        starts.append(pos)
        pos += T + 1
    return starts, pos + 2


def run_table(engine, device, rate_in, rate_out, rows, label):
    """rows: [(T_in, T_out)].  One launch of Engine.resample_rows over rows that start at odd offsets of NaN-filled arrays; every row
    meets the bar against the oracle, the input array and everything outside the output rows keep their bits.  Returns the output."""
    eng = engine_or_default(engine)
    up, down, h = resample_mod().resample_taps(rate_in, rate_out)
    in_starts, in_total = odd_layout([r[0] for r in rows])
    out_starts, out_total = odd_layout([r[1] for r in rows], first=3)
    src = np.full(in_total, np.nan, np.float32)
    for k, ((T, _), s) in enumerate(zip(rows, in_starts)):
        src[s:s + T] = signal(T, seed=k % 3)
    table = np.asarray([(a, T, b, To) for (T, To), a, b in zip(rows, in_starts, out_starts)], np.int64)
    flat = torch.from_numpy(src).to(device)
    before = flat.clone()
    out = torch.full((out_total,), float("nan"), dtype=torch.float32, device=device)
    eng.resample_rows(flat, torch.from_numpy(table).to(device), out, rate_in, rate_out, max(r[1] for r in rows))
    host = out.cpu()
    written = np.zeros(out_total, bool)
    for k, ((T, To), b) in enumerate(zip(rows, out_starts)):
        ref, bar = reference(rate_in, rate_out, T, k % 3, To)
        check_against(ref, bar, host[b:b + To], f"{label} row {k} (T_in {T}, T_out {To}, natural {R.natural_length(T, up, down)})")
        written[b:b + To] = True
    guards_ok = bool(torch.isnan(host[torch.from_numpy(~written)]).all()) and bit_equal(flat, before)
    print(f"{label}: {len(rows)} rows in one launch, guards untouched: {guards_ok}")
    assert guards_ok, f"{label}: a guard was touched"
    return out


def check_case_f(engine, device, rates):
    """The ragged table at one rate pair: natural output lengths."""
    rate_in, rate_out = rates
    rs = resample_mod()
    rows = [(T, rs.resampled_length(T, rate_in, rate_out)) for T in RAGGED]
    out = run_table(engine, device, rate_in, rate_out, rows, f"case f {rate_in} -> {rate_out}")
    assert bit_equal(out, run_table(engine, device, rate_in, rate_out, rows, f"case f {rate_in} -> {rate_out}, again")), "case f: two runs differ"
    # the same rows through resample_many: the bits of the table-driven launch
    recs = [torch.from_numpy(np.array(signal(T, seed=k % 3))).to(device) for k, (T, _) in enumerate(rows)]
    recs = [r.view(1, 1, -1) if k % 2 else r for k, r in enumerate(recs)]
    many = rs.resample_many(recs, rate_in, rate_out, engine=engine)
    starts, _ = odd_layout([r[1] for r in rows], first=3)
    for k, (rec, y, (_, To), b) in enumerate(zip(recs, many, rows, starts)):
        assert y.shape == rec.shape[:-1] + (To,) and bit_equal(y.reshape(-1), out[b:b + To]), f"case f: resample_many row {k}"


def natural_input(To, up, down):
    """The smallest T_in whose natural output length is at least To."""
    T = max(1, (To - 1) * down // up)
    while R.natural_length(T, up, down) < To:
        T += 1
    return T


def check_case_g(engine, device, rates):
    """T_out off the natural length, and rows at the kernel's outputs per block, one below and one above it."""
    rate_in, rate_out = rates
    rs = resample_mod()
    up, down, h = rs.resample_taps(rate_in, rate_out)
    tile = rs.outputs_per_block(rate_in, rate_out, engine)
    assert tile >= 1 and tile == int(engine_or_default(engine).lib.wunet_resample_tile(up, down, len(h)))
    rows = [(natural_input(To, up, down), To) for To in (tile - 1, tile, tile + 1)]
    T = natural_input(tile, up, down)
    nat = R.natural_length(T, up, down)
    rows += [(T, nat - 5), (T, nat + 4), (100, R.natural_length(100, up, down) + 3), (100, R.natural_length(100, up, down) - 2), (3, 9)]
    print(f"case g {rate_in} -> {rate_out}: {tile} outputs per block")
    run_table(engine, device, rate_in, rate_out, rows, f"case g {rate_in} -> {rate_out}")


@functools.lru_cache(maxsize=None)
def round_trip_reference(sample_rate, model_rate, T):
    """(ref, bar) of signal(T) taken to model_rate and back to T samples at sample_rate: the two-stage bar of this file's docstring."""
    rs = resample_mod()
    u1, d1, h1 = rs.resample_taps(sample_rate, model_rate)
    u2, d2, h2 = rs.resample_taps(model_rate, sample_rate)
    ref1, s1 = R.resample(signal(T), u1, d1, h1)
    bar1 = bar_of(ref1, s1, u1, len(h1))
    ref, _ = R.resample(ref1, u2, d2, h2, T)
    _, c = R.resample(bar1, u2, d2, h2, T)
    _, s2 = R.resample(np.abs(ref1) + bar1, u2, d2, h2, T)
    bar = c + 2.0 ** -24 * (np.abs(ref) + c) + (1.0 + 2.0 ** -24) * terms(u2, len(h2)) * 2.0 ** -52 * s2 + 2.0 ** -150
    return ref, bar


def check_enhance_round_trip(engine, device, sample_rate, T=1000, L=64, model_rate=16000, **kw):
    """enhance with the identity stub at another rate: the oracle's down-then-up, trimmed to T; the model saw chunks at model_rate."""
    inf, rs = inference(), resample_mod()
    stub = Stub(L, identity=True).to(device)
    mix = torch.from_numpy(np.array(signal(T))).to(device).view(1, 1, -1)
    out = inf.enhance(stub, mix, sample_length=L, engine=engine, sample_rate=sample_rate, model_rate=model_rate, **kw)
    assert out.shape == (1, 1, T) and out.dtype == torch.float32
    Tm = rs.resampled_length(T, sample_rate, model_rate)
    assert rs.resampled_length(Tm, model_rate, sample_rate) >= T
    ref, bar = round_trip_reference(sample_rate, model_rate, T)
    check_against(ref, bar, out, f"enhance, identity model, {sample_rate} -> {model_rate} -> {sample_rate} Hz, T {T} (T {Tm} at the model)")
    return out, stub
