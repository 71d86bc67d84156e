"""The case table of the on-device mix (mix_partial_kernel / mix_apply_kernel behind wunet_mix_windows), shared by
tests/test_mix_emu.py (CPU emulator) and tests/test_gpu_mix.py (MI355X): what runs, on which tensors, and the checks against the
float64 oracle of tests/mix_ref.py.  `engine` None = the product's default engine.

Bars (derived, not measured; the oracle's double sums differ from the kernels' by about L 2^-53 only):
  gains      |g - g_ref| <= 2^-23 |g_ref|, the same for a: a correctly rounded float32 of a double result, with a factor of two for the
             sqrt / pow of two double implementations.
  waveforms  |mixture - ref| <= 2^-21 (|a c| + |a g n|), |clean_out - ref| <= 2^-22 |a c| per element: at most five float32 roundings
             of 2^-24 each, those of g and a included.
Every flat array is a view into a NaN-filled buffer (and starts 4-byte aligned only), so a read outside it turns the row into NaN;
every output is a view into a buffer of sentinels that must survive, and is NaN before the call."""
import functools
import importlib
import wave

import numpy as np
import torch

import mix_ref as R
from conftest import PKG_NAME

PAD = 5                  # floats of NaN in front of a flat array: its base is 4-byte aligned only
GUARD = 16               # sentinel floats either side of an output (64 bytes: the output stays 16-byte aligned)
SENTINEL = 12345.0
PEAK = 0.99
EPS = 1e-8               # metrics.snr's default


def metrics():
    return importlib.import_module(PKG_NAME + ".metrics")


def _db(x):
    return np.float32(10.0 ** (x / 20.0))


def _case_a(rng):
    # scalar tail (L = 37); noise items of 13 (wraps three times), 37 (exactly L) and 500 samples; phases 0, nl - 1, mid
    clean = rng.uniform(-0.5, 0.5, 200)
    noise = rng.standard_normal(13 + 37 + 500) * 0.1
    rows = [[1, 0, 13, 0], [50, 13, 37, 36], [200 - 37, 50, 500, 250]]
    params = [[5.0, 1.0], [0.0, 1.0], [20.0, 1.0]]
    return clean, noise, rows, params, 37


def _case_b(rng):
    # float4 body, a 4-aligned length with unaligned starts; row 1's clean window ends on the last sample of the shard
    clean = rng.uniform(-0.5, 0.5, 9001)
    noise = rng.standard_normal(7010) * 0.1
    rows = [[3, 5, 1000, 999], [9001 - 4100, 1005, 6000, 123]]
    params = [[10.0, 1.0], [3.0, _db(-3.0)]]
    return clean, noise, rows, params, 4100


def _case_c(rng):
    # 16 pieces per row: the fold order of the partials matters; SNR -5 and 40 dB
    clean = rng.uniform(-0.5, 0.5, 40000)
    noise = rng.standard_normal(23001) * 0.1
    rows = [[17, 0, 20000, 7777], [20001, 20000, 3001, 3000]]
    params = [[-5.0, _db(-20.0)], [40.0, 1.0]]
    return clean, noise, rows, params, 16384


def _case_d(rng):
    # row 0 ordinary; row 1 a silent noise item (all zeros); row 2 a silent clean window; row 3 nl = 0
    clean = rng.uniform(-0.5, 0.5, 1200)
    clean[600:900] = 0.0
    noise = rng.standard_normal(900) * 0.1
    noise[300:600] = 0.0
    rows = [[7, 0, 300, 11], [301, 300, 300, 5], [622, 600, 300, 0], [11, 0, 0, 0]]
    params = [[10.0, 1.0], [10.0, 1.0], [10.0, _db(6.0)], [10.0, _db(-6.0)]]
    return clean, noise, rows, params, 256


def _case_e(rng):
    # level +12 dB on a clean window with peak 0.9: the guard fires on row 0 and not on row 1 (level -6 dB)
    clean = rng.uniform(-0.5, 0.5, 1500)
    clean[100:612] *= 0.9 / np.abs(clean[100:612]).max()
    clean[900:1412] *= 0.9 / np.abs(clean[900:1412]).max()
    noise = rng.standard_normal(2000) * 0.1
    rows = [[100, 0, 700, 33], [900, 700, 1300, 650]]
    params = [[10.0, _db(12.0)], [10.0, _db(-6.0)]]
    return clean, noise, rows, params, 512


def _case_f(rng):
    # corrupt tables: negative start, start past the end, item ranges that leave the noise array on either side, wild values
    clean = rng.uniform(-0.5, 0.5, 300)
    noise = rng.standard_normal(200) * 0.1
    rows = [[-7, 10, 50, 3], [350, -10, 30, 5], [100, 180, 100, 17], [2 ** 62, 500, 10, 0], [-2 ** 62, 3, 2 ** 62, -1]]
    params = [[10.0, 1.0]] * 5
    return clean, noise, rows, params, 64


CASES = {"a": _case_a, "b": _case_b, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f}


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case (float32 / int64 numpy arrays) - built once, shared, never modified."""
    clean, noise, rows, params, L = CASES[name](np.random.default_rng(sorted(CASES).index(name) + 100))
    d = {"clean": clean.astype(np.float32), "noise": noise.astype(np.float32), "rows": np.asarray(rows, np.int64),
         "params": np.asarray(params, np.float32), "L": L}
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, peak_limit=PEAK):
    d = case(name)
    return R.mix_reference(d["clean"], d["noise"], d["rows"], d["params"], d["L"], peak_limit)


def guarded_flat(x, device):
    """x (float32 numpy) as a view into a NaN-filled device buffer, PAD floats in: a read outside the array reads NaN."""
    buf = torch.full((len(x) + 2 * PAD,), float("nan"), dtype=torch.float32)
    buf[PAD:PAD + len(x)] = torch.from_numpy(np.array(x))
    buf = buf.to(device)
    return buf[PAD:PAD + len(x)]


def guarded_out(shape, device):
    """(NaN-filled output view of `shape`, its whole buffer): GUARD sentinels either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=device)
    view = buf[GUARD:GUARD + n].view(*shape)
    view.fill_(float("nan"))
    return view, buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def engine_or_default(engine):
    return engine if engine is not None else importlib.import_module(PKG_NAME + ".engine").default_engine()


def run(engine, device, name, peak_limit=PEAK):
    """One call on guarded tensors: (mixture [B,1,L], clean_out [B,1,L], gains [B,2]) on `device`."""
    d = case(name)
    B, L = d["rows"].shape[0], d["L"]
    cf, nf = guarded_flat(d["clean"], device), guarded_flat(d["noise"], device)
    rows, params = torch.from_numpy(np.array(d["rows"])).to(device), torch.from_numpy(np.array(d["params"])).to(device)
    (mix, mbuf), (cl, cbuf), (gains, gbuf) = guarded_out((B, 1, L), device), guarded_out((B, 1, L), device), guarded_out((B, 2), device)
    engine_or_default(engine).mix_windows(cf, nf, rows, params, mix, cl, gains, peak_limit=peak_limit)
    assert guards_intact(mbuf) and guards_intact(cbuf) and guards_intact(gbuf), f"case {name}: a guard float was overwritten"
    return mix, cl, gains


def bit_equal(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def check_against(ref, mix, cl, gains, label):
    """The bars of this file's docstring on every element of the three outputs; g == 0 rows carry mixture == clean_out bit for bit."""
    m, c, gn = mix.double().cpu().numpy()[:, 0], cl.double().cpu().numpy()[:, 0], gains.double().cpu().numpy()
    assert np.isfinite(m).all() and np.isfinite(c).all() and np.isfinite(gn).all(), f"{label}: NaN / Inf (or an element never written)"
    dg, da = np.abs(gn[:, 0] - ref["g"]), np.abs(gn[:, 1] - ref["a"])
    dm, dc = np.abs(m - ref["mixture"]), np.abs(c - ref["clean"])
    bm, bc = 2.0 ** -21 * (ref["ac"] + ref["agn"]), 2.0 ** -22 * ref["ac"]
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{label}: g {gn[:, 0]} a {gn[:, 1]}  rel dg {np.nan_to_num(dg / np.abs(ref['g'])).max():.2e} da {(da / np.abs(ref['a'])).max():.2e} "
              f"(bar {2.0 ** -23:.2e})  worst dm / bar {np.nan_to_num(dm / bm).max():.3f}  dc / bar {np.nan_to_num(dc / bc).max():.3f}")
    assert (dg <= 2.0 ** -23 * np.abs(ref["g"])).all() and (da <= 2.0 ** -23 * np.abs(ref["a"])).all(), (label, dg, da)
    assert (dm <= bm).all() and (dc <= bc).all(), (label, (dm - bm).max(), (dc - bc).max())
    for b in np.nonzero(ref["g"] == 0.0)[0]:
        assert gn[b, 0] == 0.0 and bit_equal(mix[b], cl[b]), f"{label}: row {b} has no noise and must come out unmixed"


def snr_bound_db(ref, b, snr_db):
    """How far metrics.snr(clean_out, mixture, zero_mean=False) of row b may lie from the drawn snr_db, from the bars above.
    With r = ||a c|| / ||a g n|| = 10^(snr_db / 20) (for the float32 g of the reference waveforms; the double g differs by 2^-24):
      clean_out = a c + d, |d| <= 2^-22 |a c|                                 -> sqrt(Et) within (1 +- x1) ||a c||,   x1 = 2^-22
      mixture - clean_out = a g n + e, |e| <= 2^-21 (|a c| + |a g n|) + |d|   -> sqrt(En) within (1 +- x2) ||a g n||, x2 = 2^-21 (1 + 1.5 r)
      the rounding of g to float32                                             -> x3 = 2^-24
    20 log10(1 + x) <= 8.686 x; the second-order terms of x < 1e-3 fit in a factor 1.001.  metrics.snr adds eps = 1e-8 to both energies:
    at most 4.343 eps (1 / Et + 1 / En) dB; its float32 result is rounded once: 2^-23 max(|snr_db|, 1) covers that rounding and
    the float32 -> dB conversion.  The kernels' double sums (L 2^-53) are far below all of this."""
    r = 10.0 ** (snr_db / 20.0)
    x = 2.0 ** -22 + 2.0 ** -21 * (1.0 + 1.5 * r) + 2.0 ** -24
    k = 20.0 / np.log(10.0)
    return 1.001 * k * x + 1.001 * 0.5 * k * EPS * (1.0 / ref["Et"][b] + 1.0 / ref["En"][b]) + 2.0 ** -23 * max(abs(snr_db), 1.0)


def check_snr(ref, params, mix, cl, engine, label):
    """metrics.snr reads the mixed batch back: every ordinary row (g > 0) carries the SNR that was asked for."""
    v = metrics().snr(cl, mix, zero_mean=False, engine=engine).double().cpu().numpy()
    for b in np.nonzero(ref["g"] > 0.0)[0]:
        want = float(params[b, 0])
        bound = snr_bound_db(ref, b, want)
        print(f"{label}: row {b} asked {want:.3f} dB, metrics.snr {v[b]:.6f} dB (bound {bound:.2e})")
        assert abs(v[b] - want) <= bound, (label, b, v[b], want, bound)


def check_case(name, engine, device):
    d, ref = case(name), reference(name)
    mix, cl, gains = run(engine, device, name)
    B, L = d["rows"].shape[0], d["L"]
    assert mix.shape == (B, 1, L) and cl.shape == (B, 1, L) and mix.device.type == device.type
    check_against(ref, mix, cl, gains, f"case {name}")
    check_snr(ref, d["params"], mix, cl, engine, f"case {name}")
    # peak guard: max|mixture| <= peak_limit (1 + 2^-22) on every row, fired or not (four roundings behind the guard's bound)
    peak = np.abs(mix.double().cpu().numpy()[:, 0]).max(axis=1)
    assert (peak <= float(np.float32(PEAK)) * (1.0 + 2.0 ** -22)).all(), (name, peak)
    # two calls on the same tables are bit-identical
    again = run(engine, device, name)
    assert all(bit_equal(x, y) for x, y in zip((mix, cl, gains), again)), f"case {name}: two runs differ"
    ng = ref["g"]
    if name == "d":
        assert ng[0] > 0.0 and (ng[1:] == 0.0).all()
    if name == "e":
        assert list(ref["peak_fired"]) == [True, False]
        # clean_out is scaled by the same a: a < level on the fired row, and clean_out = a c there (check_against holds it to a)
        g = gains.double().cpu().numpy()
        assert g[0, 1] < float(d["params"][0, 1]) and g[1, 1] == float(d["params"][1, 1])
        # peak_limit = 0 turns the guard off: a is the level, exactly, and row 0 leaves the limit
        off = reference(name, 0.0)
        assert not off["peak_fired"].any()
        m0, c0, g0 = run(engine, device, name, peak_limit=0.0)
        check_against(off, m0, c0, g0, "case e, peak_limit 0")
        assert torch.equal(g0[:, 1].cpu(), torch.from_numpy(np.array(d["params"][:, 1]))) and float(m0[0].abs().max()) > 2.0
    if name == "f":
        cl_rows = [R.clamp_row(r, len(d["clean"]), len(d["noise"]), L) for r in d["rows"]]
        assert cl_rows == [(0, 10, 50, 3), (236, 0, 20, 5), (100, 180, 20, 17), (236, 0, 0, 0), (0, 3, 197, 196)]
        assert list(ng > 0.0) == [True, True, True, False, True]
    return mix, cl, gains


# ---------------------------------------------------------------------------------------------- MixLoader on a tiny corpus
def _write_pcm16(path, x, rate=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes((np.clip(x, -1, 1 - 1 / 32768) * 32768).astype("<i2").tobytes())


def _quantised(x):
    return (np.clip(x, -1, 1 - 1 / 32768) * 32768).astype("<i2").astype(np.float32) / 32768.0


def corpus(tmp_path, noise_rate=16000):
    """Six clean items of 300 - 700 samples and four noise items of 20 - 900 samples as 16-bit files + their two list files.
    Returns (clean list, noise list, {clean name: samples as written}, [noise samples as written])."""
    rng = np.random.default_rng(5)
    clean_items, noise_items, cl_lines, no_lines = {}, [], [], []
    for i in range(6):
        x = (rng.random(int(rng.integers(300, 700))) * 2 - 1).astype(np.float32) * 0.6
        p = tmp_path / f"speech{i}.wav"
        _write_pcm16(p, x)
        clean_items[f"speech{i}"] = _quantised(x)
        cl_lines.append(str(p))
    for i, T in enumerate((20, 150, 400, 900)):
        x = (0.2 * rng.standard_normal(T)).astype(np.float32)
        p = tmp_path / f"noise{i}.wav"
        _write_pcm16(p, x, rate=noise_rate)
        noise_items.append(_quantised(x))
        no_lines.append(str(p))
    cl, no = tmp_path / "clean.txt", tmp_path / "noise.txt"
    cl.write_text("\n".join(cl_lines) + "\n")
    no.write_text("\n".join(no_lines) + "\n")
    return cl, no, clean_items, noise_items


def check_loader(wd, tmp_path, engine, device):
    """MixLoader end to end: every batch against the oracle applied to loader.last_draw and to the corpus as written."""
    cl_list, no_list, clean_items, noise_items = corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    assert wd.pack_mono_shard(str(cl_list), cp) == 6 and wd.pack_mono_shard(str(no_list), npfx) == 4
    clean_flat, noise_flat = np.concatenate(list(clean_items.values())), np.concatenate(noise_items)
    assert np.array_equal(np.fromfile(cp + ".f32", np.float32), clean_flat) and np.array_equal(np.fromfile(npfx + ".f32", np.float32), noise_flat)
    L, B, snr_range = 256, 4, (-5.0, 15.0)
    kw = dict(batch_size=B, sample_length=L, snr_db=snr_range, level_db=(-6.0, 6.0), p_clean=0.25, device=device, steps_per_epoch=3, engine=engine)
    loader = wd.MixLoader(cp, npfx, seed=11, **kw)
    assert len(loader) == 3 and loader.last_draw is None
    batches, clean_rows, noisy_rows = [], 0, 0
    for mixture, clean, names in loader:
        draw = loader.last_draw
        rows, params = draw["rows"].numpy(), draw["params"].numpy()
        assert mixture.shape == (B, 1, L) and clean.shape == (B, 1, L) and mixture.dtype == torch.float32 and mixture.device.type == device.type
        assert rows.shape == (B, 4) and rows.dtype == np.int64 and params.shape == (B, 2) and params.dtype == np.float32 and len(names) == B
        ref = R.mix_reference(clean_flat, noise_flat, rows, params, L, loader.peak_limit)
        check_against(ref, mixture, clean, draw["gains"], f"loader batch {len(batches)}")
        check_snr(ref, params, mixture, clean, engine, f"loader batch {len(batches)}")
        assert ((params[:, 0] >= snr_range[0]) & (params[:, 0] <= snr_range[1])).all()                       # every SNR inside snr_db
        assert ((params[:, 1] >= _db(-6.0) * (1 - 2.0 ** -23)) & (params[:, 1] <= _db(6.0) * (1 + 2.0 ** -23))).all()
        a32 = draw["gains"][:, 1].cpu().numpy()
        for b, nm in enumerate(names):                                                                       # the clean row is a window of the item it names
            src, row = clean_items[nm], clean[b, 0].cpu().numpy()
            hits = [s for s in range(len(src) - L + 1) if np.array_equal(a32[b] * src[s:s + L], row)]
            assert len(hits) == 1, (nm, hits)
            if rows[b, 2] == 0:
                assert bit_equal(mixture[b], clean[b])
                clean_rows += 1
            else:
                assert not torch.equal(mixture[b], clean[b])
                noisy_rows += 1
        batches.append((mixture.clone(), clean.clone(), list(names)))
    assert len(batches) == 3 and clean_rows > 0 and noisy_rows > 0
    # the same seed reproduces the batches bit for bit, another seed does not
    for (m1, c1, n1), (m2, c2, n2) in zip(batches, wd.MixLoader(cp, npfx, seed=11, **kw)):
        assert bit_equal(m1, m2) and bit_equal(c1, c2) and n1 == n2
    m3, _, _ = next(iter(wd.MixLoader(cp, npfx, seed=12, **kw)))
    assert not torch.equal(m3, batches[0][0])
    # p_clean = 1: the mixture is the clean batch
    kw1 = dict(kw, p_clean=1.0, steps_per_epoch=1)
    for mixture, clean, _ in wd.MixLoader(cp, npfx, seed=3, **kw1):
        assert bit_equal(mixture, clean) and float(clean.abs().max()) > 0.0
    # a pair shard of pack_shard as the clean corpus: its .clean.f32 is used
    pair = tmp_path / "pairs.txt"
    pair.write_text("".join(f"{tmp_path / f'noise{3}.wav'} {tmp_path / f'noise{3}.wav'}\n" for _ in range(2)))
    pp = str(tmp_path / "pair")
    assert wd.pack_shard(str(pair), pp) == 2
    for mixture, clean, names in wd.MixLoader(pp, npfx, seed=1, **dict(kw1, level_db=None)):
        assert names == ["noise3"] * B and bit_equal(mixture, clean)
    return cp, npfx
