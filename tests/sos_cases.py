"""The case table of the on-device biquad cascades (sos_windows_kernel behind wunet_sos_windows), shared by tests/test_sos_emu.py (CPU
emulator) and tests/test_gpu_sos.py (MI355X): what runs, on which tensors, and the checks against the oracle of tests/sos_ref.py.
`engine` None = the product's default engine.

The bar, per element (derived, not measured):   |out - arb| <= 2^-24 |arb| + max(8 e_ref, 2^-50 A)
  arb    the recurrence in np.longdouble on the float32 coefficients and float32 inputs (the arbiter)
  e_ref  the row maximum of |scipy.signal.sosfilt in float64 - arb|: what double arithmetic itself costs on that row
  A      max|x| sum|h| of the cascade's float64 impulse response: the bound of the output
The first term is the single rounding to float32.  The second lets the kernel's double arithmetic - the same recurrence, with the entry
state of every chunk of 64 samples taken from one 2S x 2S product per chunk instead of 64 more steps - be at most 8 times as far from
exact as scipy's own double recurrence; 2^-50 A is a floor of 8 units of 2^-53 A for rows on which scipy happens to be exact.  A numpy
float64 model of the chunked scheme measured, in units of 2^-53 A, 1.3 - 460 against scipy's 1.3 - 464 on the filters of case c (a
factor >= 2.7 to spare for the worst, a single resonator of pole radius 0.999); the kernel runs that scheme, so no other factor is
needed.  Two conditions keep the bar honest, asserted on the CPU (test_sos_emu.py): on every row of every case the second term is at
most 2^-8 of 2^-24 rms(arb) - a float32-rounding bar - and the oracle re-run with float32 state FAILS check_against on case c.

t is the tile (the samples a block owns per trip) and c the chunk (the consecutive samples a thread owns), both from wunet_sos_tile.
The lead-in is at most 8192 samples, half a tile of 16384: a tile boundary never falls inside it, chunk boundaries do (case b).

Every flat array is a view into a NaN-filled buffer (and starts 4-byte aligned only), so a read outside it turns the row into NaN;
every output is a view into a buffer of sentinels that must survive, and is NaN before the call."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import mix_cases as M
import sos_ref as R

FS = 16000.0


def _k5(sos6):
    """scipy's [S, 6] (float64) -> float32 [S, 5], each section divided by its a0."""
    s = np.asarray(sos6, np.float64)
    return (s[:, [0, 1, 2, 4, 5]] / s[:, 3:4]).astype(np.float32)


IDENTITY = np.array([[1.0, 0.0, 0.0, 0.0, 0.0]], np.float32)


def _random(rng, S, spread=0.375):
    k = np.zeros((S, 5), np.float32)
    k[:, 0] = 1.0
    k[:, 1:] = rng.uniform(-spread, spread, (S, 4))
    return k


def _padded(k, S):
    return np.concatenate([k] + [IDENTITY] * (S - len(k)), axis=0)


def _case_a(rng, t, c):
    # less than one chunk, scalar tail
    flat = rng.uniform(-0.5, 0.5, 200)
    rows = [[1, 1, 0, 0], [50, 50, 0, 0], [163, 100, 0, 0]]
    return flat, rows, [_random(rng, 1) for _ in rows], 37, 0


def _case_b(L, lead):
    def make(rng, t, c):
        # lengths around one chunk and one tile; the dropped head (5, c + 3) is no multiple of the chunk.  A linear row with its whole
        # lead-in inside the item, one whose item starts 2 samples in front of the window, and a circular row.
        L_ = eval(L, {"t": t, "c": c})
        ld = eval(lead, {"c": c})
        flat = rng.uniform(-0.5, 0.5, L_ + ld + 120)
        rows = [[ld + 20, 3, 0, 0], [ld + 100, ld + 98, 0, 0], [0, 7, 101, 50]]
        return flat, rows, [_random(rng, 2) for _ in rows], L_, ld
    return make


def _case_c(rng, t, c):
    # three tiles and a bit, eight sections, near-unit poles: a state dropped at a chunk or tile boundary shows at once
    L = 3 * t + 5
    flat = rng.uniform(-0.5, 0.5, L + 2) + 0.25
    r, th = 0.999, 2.0 * np.pi * 1000.0 / FS
    resonator = np.array([[1.0 - r, 0.0, 0.0, -2.0 * r * np.cos(th), r * r]], np.float32)
    lp = _k5(scipy.signal.butter(8, 3400.0, "lowpass", fs=FS, output="sos"))
    hp = np.concatenate([_k5(scipy.signal.butter(2, 20.0, "highpass", fs=FS, output="sos")),
                         _k5(scipy.signal.butter(4, 80.0, "highpass", fs=FS, output="sos")), resonator])
    rows = [[0, 0, 0, 0], [1, 1, 0, 0], [2, 2, 0, 0]]
    return flat, rows, [_padded(lp, 8), _padded(hp, 8), _random(rng, 8)], L, 0


D_LEAD = 300
D_GAPS = (0, 1, D_LEAD - 1, D_LEAD, D_LEAD + 1)


def _case_d(rng, t, c):
    # linear rows whose item starts 0, 1, lead - 1, lead, lead + 1 samples in front of the window; what lies in front of an item is
    # 1e3 (another utterance), so a leak is a wrong number; the last row's window ends on the last sample of the array
    L, parts, rows, pos = 200, [], [], 0
    for gap in D_GAPS:
        parts += [np.full(8, 1e3), rng.uniform(-0.5, 0.5, gap + L)]
        rows.append([pos + 8 + gap, pos + 8, 0, 0])
        pos += 8 + gap + L
    return np.concatenate(parts), rows, [_random(rng, 2) for _ in rows], L, D_LEAD


def _case_e(rng, t, c):
    # circular rows: items of 1, 13, L and L + lead + 7 samples from phases 0, nl - 1 and mid; the lead-in wraps backwards
    L, lead, rows, pos = 200, 50, [], 3
    for nl in (1, 13, L, L + lead + 7):
        for ph in sorted({0, nl - 1, nl // 2}):
            rows.append([12345, pos, nl, ph])
        pos += nl
    flat = rng.uniform(-0.5, 0.5, pos + 4)
    return flat, rows, [_random(rng, 2) for _ in rows], L, lead


F_CLAMPS = [("linear", 0, 0, 0), ("linear", 236, 0, 20), ("linear", 236, 236, 0), ("linear", 0, 0, 0), ("linear", 100, 90, 10),
            ("circular", 0, 20, 5, 20), ("circular", 280, 20, 17, 20), ("zeros",), ("circular", 3, 297, 296, 20), ("zeros",),
            ("zeros",)]


def _case_f(rng, t, c):
    # corrupt tables: negative starts, starts past the end, item ranges that leave the array on either side, +-2^62, nl huge
    flat = rng.uniform(-0.5, 0.5, 300)
    rows = [[-7, 10, 0, 0], [350, -10, 0, 99], [2 ** 62, 2 ** 62, -5, 0], [-2 ** 62, -2 ** 62, -2 ** 62, 2 ** 62], [100, 90, 0, 0],
            [0, -10, 30, 5], [5, 280, 100, 17], [5, 500, 10, 0], [-1, 3, 2 ** 62, -1], [0, -2 ** 62, 2 ** 62, 7],
            [2 ** 62, -2 ** 62, 2 ** 62 + 2 ** 61, -1]]
    return flat, rows, [_random(rng, 2) for _ in rows], 64, 20


def _case_g(rng, t, c):
    # identity sections only: the output is the window, as values
    L = t + 5
    flat = rng.uniform(-0.5, 0.5, L + 50)
    rows = [[30, 0, 0, 0], [0, 5, 77, 70]]
    return flat, rows, [_padded(IDENTITY, 3) for _ in rows], L, 10


B_LENGTHS = ("c - 1", "c", "c + 1", "t - 1", "t", "t + 1")
B_LEADS = ("5", "c + 3")
CASES = {"a": _case_a, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f, "g": _case_g}
for _i, _L in enumerate(B_LENGTHS):
    for _j, _ld in enumerate(B_LEADS):
        CASES[f"b{_i}{_j}"] = _case_b(_L, _ld)
F_NAN_ROW = 4                # the row of case f that gets NaN coefficients in the second half of its check


@functools.lru_cache(maxsize=None)
def case(name, t, c):
    """The inputs of one case (float32 / int64 numpy arrays) - built once, shared, never modified."""
    flat, rows, coefs, L, lead = CASES[name](np.random.default_rng(sorted(CASES).index(name) + 300), t, c)
    d = {"flat": flat.astype(np.float32), "rows": np.asarray(rows, np.int64), "coefs": np.stack(coefs).astype(np.float32), "L": L,
         "lead": lead}
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, t, c):
    d = case(name, t, c)
    return R.sos_reference(d["flat"], d["rows"], d["coefs"], d["L"], d["lead"])


def tile(engine):
    """(t, c) of the engine's library for the 8-section kernel (the geometry does not depend on the count)."""
    t, c = M.engine_or_default(engine).sos_tile(8)
    assert t % c == 0 and c >= 8 and t > c
    return t, c


def run(engine, device, d, coefs=None):
    """One call on guarded tensors: out [B, 1, L] on `device`."""
    B, L = d["rows"].shape[0], d["L"]
    flat = M.guarded_flat(d["flat"], device)
    rows = torch.from_numpy(np.array(d["rows"])).to(device)
    k = torch.from_numpy(np.array(d["coefs"] if coefs is None else coefs)).to(device)
    out, buf = M.guarded_out((B, 1, L), device)
    M.engine_or_default(engine).sos_windows(flat, rows, k, out, lead=d["lead"])
    assert M.guards_intact(buf), "a guard float was overwritten"
    return out


def check_against(ref, out, label, rows=None):
    """The bar of this file's docstring on every element (of `rows`: default all); prints the worst error / bar per row first."""
    o = np.asarray(out, np.float64) if isinstance(out, np.ndarray) else out.double().cpu().numpy()[:, 0]
    rows = range(o.shape[0]) if rows is None else rows
    worst = []
    for b in rows:
        err = np.abs(o[b].astype(np.longdouble) - ref["arb"][b]).astype(np.float64)
        worst.append(float(np.nan_to_num(err / ref["bar"][b], nan=np.inf).max()) if ref["bar"][b].max() > 0.0 else float(np.abs(o[b]).max() > 0))
    print(f"{label}: worst error / bar per row {['%.3f' % w for w in worst]}")
    for b in rows:
        assert np.isfinite(o[b]).all(), f"{label}: row {b} has NaN / Inf (or an element never written)"
    assert max(worst) <= 1.0, (label, worst)


def require_long_double():
    if not R.HAVE_LONGDOUBLE:
        pytest.skip("np.longdouble has fewer than 64 bits of mantissa here: no arbiter above float64")
    assert np.finfo(np.longdouble).nmant >= 63


def check_case(name, engine, device):
    require_long_double()
    t, c = tile(engine)
    d, ref = case(name, t, c), reference(name, t, c)
    B, L = d["rows"].shape[0], d["L"]
    out = run(engine, device, d)
    assert out.shape == (B, 1, L) and out.device.type == device.type
    check_against(ref, out, f"case {name}")
    again = run(engine, device, d)
    assert M.bit_equal(out, again), f"case {name}: two runs differ"
    if name == "d":
        assert [R.clamp_row(r, len(d["flat"]), L, d["lead"])[3] for r in d["rows"]] == [0, 1, D_LEAD - 1, D_LEAD, D_LEAD]
        assert int(d["rows"][-1, 0]) + L == len(d["flat"])
        assert float(out.abs().max()) < 100.0                           # (nothing of the 1e3 in front of an item)
    if name == "f":
        assert [R.clamp_row(r, len(d["flat"]), L, d["lead"]) for r in d["rows"]] == F_CLAMPS
        for b, cl in enumerate(F_CLAMPS):
            assert bool(out[b].any()) == (cl[0] != "zeros"), (b, cl)
        # one row with NaN coefficients among good rows: the good rows are bit-equal to the call without it
        k = np.array(d["coefs"])
        k[F_NAN_ROW, 1, 2] = np.nan
        bad = run(engine, device, d, coefs=k)
        good = [b for b in range(B) if b != F_NAN_ROW]
        assert M.bit_equal(bad[good], out[good]) and not torch.isfinite(bad[F_NAN_ROW]).all()
    if name == "g":
        assert torch.equal(out.cpu()[:, 0], torch.from_numpy(ref["x"])), "identity sections must hand the window through as values"
    return out


# ---------------------------------------------------------------------------------------------- MixLoader with the equalisers
EQ_LEAD = 64
EQ = dict(eq_speech={"sections": 3, "p": 0.75}, eq_noise={"sections": 2, "spread": 0.3}, eq_lead=EQ_LEAD)


def _k5_of(table):
    return np.ascontiguousarray(table.numpy()[..., [0, 1, 2, 4, 5]])


def staged_reference(flat, table, sos6, L, lead):
    """The oracle's staged batch: (float32 [B L] - the arbiter rounded once -, second [B]: the second term of the row's bar)."""
    ref = R.sos_reference(flat, table, _k5_of(sos6), L, lead)
    return ref["arb"].astype(np.float32).reshape(-1), ref["second"]


def check_mix_stage(mref, sc, sn, mixture, clean, gains, label):
    """mix_cases.check_against's bars on the mix stage, for a mix oracle that was fed the SOS ORACLE's staged arrays (rounded to float32)
    while the device mixed its own.  Derived, not measured: a device sample lies within its bar of the arbiter and so does the rounded
    arbiter, so the two staged arrays differ per element by at most 2^-23 |x| (1 + 2^-23) + s, s = the row's second term (sc for the
    speech, sn for the noise; <= 2^-32 rms by condition 1).  With h = 2^-23 + 2^-32 the norms of a row differ by the factor 1 +- h, so
    g = sqrt(Pc / Pn ..) by 1 +- 2 h, and a - through the peak guard's bound a (max|c| + g max|n|), continuous where it starts to fire -
    by 1 +- 4 h; second-order terms fit in the factor 1.01.  On top of mix_cases' bars that is, per element,
      g        2.02 * 2^-23 |g|          a        4.04 * 2^-23 |a|
      clean    1.01 * 2^-23 * 5 |a c| + a sc
      mixture  1.01 * 2^-23 (5 |a c| + 7 |a g n|) + a (sc + g sn)"""
    m, c, gn = mixture.double().cpu().numpy()[:, 0], clean.double().cpu().numpy()[:, 0], gains.double().cpu().numpy()
    assert np.isfinite(m).all() and np.isfinite(c).all() and np.isfinite(gn).all(), f"{label}: NaN / Inf (or an element never written)"
    u, g, a = 1.01 * 2.0 ** -23, np.abs(mref["g"])[:, None], np.abs(mref["a"])[:, None]
    dg, da = np.abs(gn[:, 0] - mref["g"]), np.abs(gn[:, 1] - mref["a"])
    bg, ba = (2.0 ** -23 + 2.0 * u) * g[:, 0], (2.0 ** -23 + 4.0 * u) * a[:, 0]
    dm, dc = np.abs(m - mref["mixture"]), np.abs(c - mref["clean"])
    bc = 2.0 ** -22 * mref["ac"] + u * 5.0 * mref["ac"] + a * sc[:, None]
    bm = 2.0 ** -21 * (mref["ac"] + mref["agn"]) + u * (5.0 * mref["ac"] + 7.0 * mref["agn"]) + a * (sc[:, None] + g * sn[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{label}: worst dg / bar {np.nan_to_num(dg / bg).max():.3f} da / bar {np.nan_to_num(da / ba).max():.3f} "
              f"dm / bar {np.nan_to_num(dm / bm).max():.3f} dc / bar {np.nan_to_num(dc / bc).max():.3f}")
    assert (dg <= bg).all() and (da <= ba).all(), (label, dg, da)
    assert (dm <= bm).all() and (dc <= bc).all(), (label, (dm - bm).max(), (dc - bc).max())
    for b in np.nonzero(mref["g"] == 0.0)[0]:
        assert gn[b, 0] == 0.0 and M.bit_equal(mixture[b], clean[b]), f"{label}: row {b} has no noise and must come out unmixed"


def _noise_table(rows):
    t = rows.copy()
    t[:, 2] = np.maximum(rows[:, 2], 1)
    return t


def _mix_rows(rows, L, speech, noise):
    B = rows.shape[0]
    r = rows.copy()
    if speech:
        r[:, 0] = np.arange(B) * L
    if noise:
        r[:, 1], r[:, 2], r[:, 3] = np.arange(B) * L, np.where(rows[:, 2] > 0, L, 0), 0
    return r


def check_loader(wd, tmp_path, engine, device):
    """MixLoader(eq_speech=..., eq_noise=...) end to end on mix_cases' tiny corpus: every batch against sos_ref applied to
    loader.last_draw's tables followed by mix_ref on the filtered arrays; the draws, the seeds, and the untouched plain loader."""
    require_long_double()
    import reverb_cases as V
    cl_list, no_list, clean_items, noise_items = M.corpus(tmp_path)
    cp, npfx = str(tmp_path / "speech"), str(tmp_path / "noise")
    assert wd.pack_mono_shard(str(cl_list), cp) == 6 and wd.pack_mono_shard(str(no_list), npfx) == 4
    clean_flat, noise_flat = np.concatenate(list(clean_items.values())), np.concatenate(noise_items)
    L, B = 256, 4
    kw = dict(batch_size=B, sample_length=L, snr_db=(-5.0, 15.0), level_db=(-6.0, 6.0), p_clean=0.25, device=device, steps_per_epoch=3, engine=engine)
    plain_loader = wd.MixLoader(cp, npfx, seed=11, **kw)
    plain = []
    for m, c, n in plain_loader:
        assert set(plain_loader.last_draw) == {"rows", "params", "gains"}
        plain.append((m.clone(), c.clone(), n, plain_loader.last_draw["rows"].clone(), plain_loader.last_draw["params"].clone()))
    # with both None the batches of a seed are what a loader built without the keywords makes, bit for bit
    for (m1, c1, n1, _, _), (m2, c2, n2) in zip(plain, wd.MixLoader(cp, npfx, seed=11, eq_speech=None, eq_noise=None, eq_lead=7, **kw)):
        assert M.bit_equal(m1, m2) and M.bit_equal(c1, c2) and n1 == n2
    short = long_ = 0
    for which in ("both", "speech", "noise"):
        eq = dict(EQ, **({"eq_noise": None} if which == "speech" else {"eq_speech": None} if which == "noise" else {}))
        loader = wd.MixLoader(cp, npfx, seed=11, **kw, **eq)
        batches = []
        for k, (mixture, clean, names) in enumerate(loader):
            draw, label = loader.last_draw, f"eq {which} batch {k}"
            assert set(draw) == {"rows", "params", "gains", "eq_speech", "eq_noise"}
            rows, params = draw["rows"].numpy(), draw["params"].numpy()
            # the equalisers' draws come after the batch's other draws: the first batch of a seed has the plain loader's rows, params, items
            if k == 0:
                assert torch.equal(draw["rows"], plain[0][3]) and torch.equal(draw["params"], plain[0][4]) and names == plain[0][2]
            assert (draw["eq_speech"] is None) == (which == "noise") and (draw["eq_noise"] is None) == (which == "speech")
            cflat, nflat, sc, sn = clean_flat, noise_flat, np.zeros(B), np.zeros(B)
            if draw["eq_speech"] is not None:
                assert draw["eq_speech"].shape == (B, 3, 6) and draw["eq_speech"].dtype == torch.float32
                starts = np.array([V.idx_start(clean_items, nm) for nm in names])
                table = np.stack([rows[:, 0], starts, 0 * starts, 0 * starts], 1)
                gap = rows[:, 0] - starts
                short, long_ = short + int((gap < EQ_LEAD).sum()), long_ + int((gap >= EQ_LEAD).sum())
                cflat, sc = staged_reference(clean_flat, table, draw["eq_speech"], L, EQ_LEAD)
            if draw["eq_noise"] is not None:
                assert draw["eq_noise"].shape == (B, 2, 6) and float(draw["eq_noise"][..., [1, 2, 4, 5]].abs().max()) <= 0.3
                nflat, sn = staged_reference(noise_flat, _noise_table(rows), draw["eq_noise"], L, EQ_LEAD)
            mref = mix_ref_of(cflat, nflat, _mix_rows(rows, L, draw["eq_speech"] is not None, draw["eq_noise"] is not None), params, L, loader.peak_limit)
            check_mix_stage(mref, sc, sn, mixture, clean, draw["gains"], label)
            # the SNR and the peak guard apply to the filtered signals
            M.check_snr(mref, params, mixture, clean, engine, label)
            peak = np.abs(mixture.double().cpu().numpy()[:, 0]).max(axis=1)
            assert (peak <= float(np.float32(loader.peak_limit)) * (1.0 + 2.0 ** -22)).all(), (label, peak)
            batches.append((mixture.clone(), clean.clone(), list(names)))
        assert len(batches) == 3 and not M.bit_equal(batches[0][0], plain[0][0])
        # the same seed gives the same bits
        for (m1, c1, n1), (m2, c2, n2) in zip(batches, wd.MixLoader(cp, npfx, seed=11, **kw, **eq)):
            assert M.bit_equal(m1, m2) and M.bit_equal(c1, c2) and n1 == n2
    assert short > 0 and long_ > 0           # (windows nearer to their item's start than the lead-in, and further)
    return cp, npfx


def mix_ref_of(clean_flat, noise_flat, rows, params, L, peak_limit):
    import mix_ref
    return mix_ref.mix_reference(clean_flat, noise_flat, rows, params, L, peak_limit)


def check_rir_loader(wd, tmp_path, engine, device):
    """MixLoader(rir_prefix=..., eq_speech=..., eq_noise=...): the reverberant batch and the target carry the row's one cascade, from
    rest at the window start.  The unfiltered counterparts are what the reverb launch stages on the drawn rir_rows - held to reverb_ref
    with reverb_cases' bar first -, the oracle filters them, and mix_ref mixes the result."""
    require_long_double()
    import reverb_cases as V
    eng = M.engine_or_default(engine)
    cl_list, no_list, clean_items, noise_items = M.corpus(tmp_path)
    rir_list, _ = V.rir_corpus(tmp_path)
    cp, npfx, rp = str(tmp_path / "speech"), str(tmp_path / "noise"), str(tmp_path / "rir")
    wd.pack_mono_shard(str(cl_list), cp)
    wd.pack_mono_shard(str(no_list), npfx)
    wd.pack_rir_shard(str(rir_list), rp)
    clean_flat, noise_flat, rir_flat = np.concatenate(list(clean_items.values())), np.concatenate(noise_items), np.fromfile(rp + ".f32", np.float32)
    cf, rf = torch.from_numpy(clean_flat).to(device), torch.from_numpy(rir_flat).to(device)
    L, B = 256, 4
    kw = dict(batch_size=B, sample_length=L, snr_db=(-5.0, 15.0), level_db=(-6.0, 6.0), p_clean=0.25, device=device, steps_per_epoch=2, engine=engine,
              rir_prefix=rp, p_reverb=0.7, early_ms=2.0)
    at = np.arange(B) * L
    table = np.stack([at, at, 0 * at, 0 * at], 1)
    for target, E in (("early", 32), ("reverberant", 1)):
        plain = wd.MixLoader(cp, npfx, seed=11, target=target, **kw)
        next(iter(plain))
        loader = wd.MixLoader(cp, npfx, seed=11, target=target, **kw, **EQ)
        for k, (mixture, tgt, names) in enumerate(loader):
            draw, label = loader.last_draw, f"eq + rir {target} batch {k}"
            assert set(draw) == {"rows", "params", "gains", "rir_rows", "reverberant", "eq_speech", "eq_noise"}
            if k == 0:                       # rows, params and rir_rows of a seed are the same with and without the equalisers
                assert all(torch.equal(draw[key], plain.last_draw[key]) for key in ("rows", "params", "rir_rows"))
            rows, params, rir_rows = draw["rows"].numpy(), draw["params"].numpy(), draw["rir_rows"].numpy()
            staged, direct = torch.empty(B, 1, L, device=device), torch.empty(B, 1, L, device=device)
            eng.reverb_windows(cf, rf, draw["rir_rows"].to(device), staged, direct, early_taps=E)
            V.check_against(V.R.reverb_reference(clean_flat, rir_flat, rir_rows, L, E), clean_flat, staged, direct, label)
            # lead 0 whatever eq_lead is: the staged batch has no past
            cflat, sc = staged_reference(staged.cpu().numpy().reshape(-1), table, draw["eq_speech"], L, 0)
            assert np.array_equal(cflat, staged_reference(staged.cpu().numpy().reshape(-1), table, draw["eq_speech"], L, EQ_LEAD)[0])
            nflat, sn = staged_reference(noise_flat, _noise_table(rows), draw["eq_noise"], L, EQ_LEAD)
            mrows = rows.copy()
            mrows[:, 0] = at
            mref = mix_ref_of(cflat, nflat, _mix_rows(mrows, L, True, True), params, L, loader.peak_limit)
            check_mix_stage(mref, sc, sn, mixture, draw["reverberant"], draw["gains"], label)
            M.check_snr(mref, params, mixture, draw["reverberant"], engine, label)
            if target == "reverberant":
                assert M.bit_equal(tgt, draw["reverberant"])
            else:
                # the target: a32 * (the direct part through the same cascade), one float32 multiply behind the filter's bar
                dref = R.sos_reference(direct.cpu().numpy().reshape(-1), table, _k5_of(draw["eq_speech"]), L, 0)
                a = draw["gains"][:, 1].double().cpu().numpy()[:, None]
                t = tgt.double().cpu().numpy()[:, 0]
                err = np.abs(t - a * dref["arb"].astype(np.float64))
                bar = a * dref["bar"] * (1.0 + 2.0 ** -23) + 2.0 ** -24 * (1.0 + 2.0 ** -23) * np.abs(t) + 2.0 ** -52 * a * np.abs(dref["arb"]).astype(np.float64)
                print(f"{label}: target worst |diff| / bar {np.nan_to_num(err / bar).max():.4f}")
                assert (err <= bar).all(), label
