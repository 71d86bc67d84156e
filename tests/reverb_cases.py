"""The case table of the on-device reverb (reverb_kernel behind wunet_reverb_windows, apply_level_kernel behind wunet_apply_level),
shared by tests/test_reverb_emu.py (CPU emulator) and tests/test_gpu_reverb.py (MI355X): what runs, on which tensors, and the checks
against the float64 oracle of tests/reverb_ref.py.  `engine` None = the product's default engine.

Bar (derived, not measured).  The products h[k] x[t] of two float32 are exact inside the fused multiply-add, and an output is one chain
of at most n = K + 256 fused adds (the K taps, the 240 leading k' of the GEMM form, K rounded up to a whole group of 16 k'), in whatever
order: |out - ref| <= gamma_n S with gamma_n = n 2^-24 / (1 - n 2^-24) and S[j] = sum_k |h[k]| |x[cs + j - k]| (Higham, Accuracy and
Stability of Numerical Algorithms, section 3.1).  `direct` is the same with n = min(E, K) + 256 and its own S.  The oracle's double
arithmetic adds n 2^-53 S, far below.  A row without taps is the window's own bits.
Every flat array is a view into a NaN-filled buffer, every output a NaN-filled view between sentinels (mix_cases' helpers)."""
import functools

import numpy as np
import torch

import mix_cases as C
import mix_ref
import reverb_ref as R

bit_equal = C.bit_equal


def _rir(rng, K, decay=None):
    """A decaying random response of K taps with h[0] = 1 (the shape pack_rir_shard leaves)."""
    decay = decay if decay is not None else max(K / 4.0, 1.0)
    h = rng.standard_normal(K) * 0.3 * np.exp(-np.arange(K) / decay)
    h[0] = 1.0
    return h


def _case_a(rng):
    # scalar tail (L = 37), one partial tile.  The item [100, 300) follows one filled with 1e6: rows at the item start, mid-item, and
    # with cs - is = 2 < K - 1; row 3 takes the response that ends on the last sample of the RIR array
    clean = np.concatenate([np.full(100, 1e6), rng.uniform(-0.5, 0.5, 200)])
    rir = np.concatenate([_rir(rng, 5), _rir(rng, 5)])
    rows = [[100, 100, 0, 5], [180, 100, 0, 5], [102, 100, 0, 5], [263, 100, 5, 5]]
    return clean, rir, rows, 37, 2


def _case_b(rng):
    # L = 256 (one full tile, float4 stores), K in {1, 16, 17, 255}: tile-boundary taps and K % 4 != 0.  Per K a random response and
    # h = delta[k - (K - 1)], whose output is the window moved by K - 1, exactly; the last delta row starts 10 samples into its item
    clean = rng.uniform(-0.5, 0.5, 1000)
    parts, rows, pos = [], [], 0
    for i, K in enumerate((1, 16, 17, 255)):
        d = np.zeros(K)
        d[K - 1] = 1.0
        parts += [_rir(rng, K), d]
        rows += [[301 + 7 * i, 0, pos, K], [413 + 5 * i, 0 if K < 255 else 418, pos + K, K]]
        pos += 2 * K
    return clean, np.concatenate(parts), rows, 256, 16


def _case_c(rng):
    # K = 300 > L = 64: the history is longer than the window; row 0 has 200 samples of it inside its item, row 1 all 299
    clean = np.concatenate([np.full(500, 1e6), rng.uniform(-0.5, 0.5, 500)])
    return clean, _rir(rng, 300), [[700, 500, 0, 300], [900, 500, 0, 300]], 64, 100


def _case_d(rng):
    # L = 4100: three chunks, the last one of 4 samples; unaligned starts; row 1's window ends on the last sample of the clean array and
    # its response on the last sample of the RIR array
    clean = rng.uniform(-0.5, 0.5, 9001)
    rir = np.concatenate([rng.standard_normal(5), _rir(rng, 1000), rng.standard_normal(5), _rir(rng, 1000)])
    return clean, rir, [[3, 0, 5, 1000], [9001 - 4100, 2000, 1010, 1000]], 4100, 300


def _case_e(rng):
    # rows without taps (K = 0, K < 0): bit copies, a -0.0 sample included; row 2 an all-zero window at the start of its item; row 3
    # early_taps = 50 >= K = 20: direct is reverberant
    clean = rng.uniform(-0.5, 0.5, 400)
    clean[50] = -0.0
    clean[200:264] = 0.0
    return clean, _rir(rng, 20), [[40, 0, 0, 0], [40, 0, 0, -5], [200, 200, 0, 20], [100, 0, 0, 20]], 64, 50


def _case_f(rng):
    # corrupt tables: negative and huge cs, is > cs, RIR ranges that leave the array on either side, K = 2^62
    clean = rng.uniform(-0.5, 0.5, 300)
    rir = _rir(rng, 200, decay=50.0)
    rows = [[-7, 10, 50, 3], [350, -10, -10, 30], [100, 150, 180, 100], [2 ** 62, 500, 500, 10], [-2 ** 62, 3, 3, 2 ** 62]]
    return clean, rir, rows, 64, 8


def _case_g(rng):
    # the long chain: K = 2049 runs over two staged segments of taps, E = 800 ends inside the first
    clean = rng.uniform(-0.5, 0.5, 6000)
    rir = np.concatenate([_rir(rng, 2049), _rir(rng, 2049)])
    return clean, rir, [[2500, 100, 0, 2049], [4976, 3000, 2049, 2049]], 1024, 800


def _case_g_long(rng):
    # (GPU only) one row of L = 16384 and K = 16384: eight chunks, eight segments; the table asks for 2^40 taps of an array of 16390
    clean = rng.uniform(-0.5, 0.5, 40000)
    return clean, _rir(rng, 16390, decay=4000.0), [[20000, 100, 0, 2 ** 40]], 16384, 800


CASES = {"a": _case_a, "b": _case_b, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f, "g": _case_g}
GPU_CASES = dict(CASES, g_long=_case_g_long)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of one case (float32 / int64 numpy arrays) - built once, shared, never modified."""
    clean, rir, rows, L, E = GPU_CASES[name](np.random.default_rng(sorted(GPU_CASES).index(name) + 200))
    d = {"clean": clean.astype(np.float32), "rir": rir.astype(np.float32), "rows": np.asarray(rows, np.int64), "L": L, "E": E}
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name):
    d = case(name)
    return R.reverb_reference(d["clean"], d["rir"], d["rows"], d["L"], d["E"])


def run(engine, device, name, with_direct=True):
    """One call on guarded tensors: (reverberant [B,1,L], direct [B,1,L] or None) on `device`."""
    d = case(name)
    B, L = d["rows"].shape[0], d["L"]
    cf, rf = C.guarded_flat(d["clean"], device), C.guarded_flat(d["rir"], device)
    rows = torch.from_numpy(np.array(d["rows"])).to(device)
    rev, rbuf = C.guarded_out((B, 1, L), device)
    direct, dbuf = C.guarded_out((B, 1, L), device) if with_direct else (None, None)
    C.engine_or_default(engine).reverb_windows(cf, rf, rows, rev, direct, early_taps=d["E"])
    assert C.guards_intact(rbuf) and (dbuf is None or C.guards_intact(dbuf)), f"case {name}: a guard float was overwritten"
    return rev, direct


def check_against(ref, clean, rev, direct, label):
    """The bar of this file's docstring on every element of the two outputs; rows without taps must be the window's own bits."""
    r, dr = rev.double().cpu().numpy()[:, 0], direct.double().cpu().numpy()[:, 0]
    assert np.isfinite(r).all() and np.isfinite(dr).all(), f"{label}: NaN / Inf (or an element never written)"
    br, bd = R.gamma(ref["n"])[:, None] * ref["S"], R.gamma(ref["nd"])[:, None] * ref["Sd"]
    er, ed = np.abs(r - ref["reverberant"]), np.abs(dr - ref["direct"])
    with np.errstate(divide="ignore", invalid="ignore"):
        print(f"{label}: taps {ref['rows'][:, 3]}  worst |diff| / bar: reverberant {np.nan_to_num(er / br).max():.4f}  direct {np.nan_to_num(ed / bd).max():.4f}"
              f"  (largest bar {br.max():.2e}, largest |diff| {er.max():.2e})")
    assert (er <= br).all() and (ed <= bd).all(), (label, (er - br).max(), (ed - bd).max())
    for b in np.nonzero(ref["rows"][:, 3] == 0)[0]:
        cs = int(ref["rows"][b, 0])
        w = torch.from_numpy(np.array(clean[cs:cs + rev.shape[-1]]))
        assert bit_equal(rev[b, 0].cpu(), w) and bit_equal(direct[b, 0].cpu(), w), f"{label}: row {b} has no taps and must be the window's bits"


def check_case(name, engine, device):
    d, ref = case(name), reference(name)
    rev, direct = run(engine, device, name)
    B, L = d["rows"].shape[0], d["L"]
    assert rev.shape == (B, 1, L) and direct.shape == (B, 1, L) and rev.device.type == device.type
    check_against(ref, d["clean"], rev, direct, f"case {name}")
    # two calls on the same tables are bit-identical, and direct = None writes the same reverberant
    again = run(engine, device, name)
    assert bit_equal(rev, again[0]) and bit_equal(direct, again[1]), f"case {name}: two runs differ"
    alone, none = run(engine, device, name, with_direct=False)
    assert none is None and bit_equal(rev, alone), f"case {name}: reverberant depends on direct"
    r, dr, cl = rev.cpu().numpy()[:, 0], direct.cpu().numpy()[:, 0], d["clean"]
    if name == "a":
        assert np.abs(r).max() < 10.0                                   # nothing of the 1e6 item in front came in
    if name == "b":
        for b, K in zip((1, 3, 5, 7), (1, 16, 17, 255)):                 # the delta rows: the window moved by K - 1, exactly
            cs, it = int(d["rows"][b, 0]), int(d["rows"][b, 1])
            want = np.array([cl[t] if t >= it else 0.0 for t in range(cs - (K - 1), cs - (K - 1) + L)], np.float32)
            assert (r[b] == want).all(), f"case b: delta row K={K}"
            assert (dr[b] == (want if K <= d["E"] else 0.0)).all(), f"case b: delta row K={K}, direct"
        assert not r[7][:244].any() and r[7][244:].all()                  # (the last one reaches 244 samples in front of its item: zero-fill)
    if name == "c":
        assert np.abs(r).max() < 10.0
    if name == "e":
        assert list(ref["rows"][:, 3]) == [0, 0, 20, 20]
        assert np.signbit(r[0][10]) and r[0][10] == 0.0 and np.signbit(dr[1][10])      # -0.0 stays -0.0
        assert not r[2].any() and not dr[2].any()                        # the all-zero window at the start of its item
        assert bit_equal(rev[3], direct[3]) and r[3].any()               # early_taps >= K
    if name == "f":
        assert [tuple(v) for v in ref["rows"]] == [(0, 0, 50, 3), (236, 0, 0, 20), (100, 100, 180, 20), (236, 236, 0, 0), (0, 0, 3, 197)]
    if name == "g_long":
        assert [tuple(v) for v in ref["rows"]] == [(20000, 100, 0, R.MAX_TAPS)]
    return rev, direct


# ---------------------------------------------------------------------------------------------- wunet_apply_level
def check_apply_level(engine, device):
    """dst = gains[:, 1] * src bit for bit (one float32 multiply), out of place and in place, scalar (L = 37) and float4 (L = 4100) rows."""
    eng = C.engine_or_default(engine)
    rng = np.random.default_rng(7)
    for L in (37, 4100):
        B = 3
        src_np = rng.standard_normal((B, 1, L)).astype(np.float32)
        src_np[0, 0, 1] = -0.0
        gains_np = np.stack([rng.uniform(0.1, 2.0, B), rng.uniform(0.1, 2.0, B)], 1).astype(np.float32)
        want = torch.from_numpy(gains_np[:, 1, None, None] * src_np)
        src, sbuf = C.guarded_out((B, 1, L), device)
        src.copy_(torch.from_numpy(src_np))
        gains = torch.from_numpy(gains_np).to(device)
        dst, dbuf = C.guarded_out((B, 1, L), device)
        assert eng.apply_level(src, gains, dst) is dst
        assert bit_equal(dst.cpu(), want) and bit_equal(src.cpu(), torch.from_numpy(src_np)) and C.guards_intact(dbuf), f"apply_level L={L}"
        assert eng.apply_level(src, gains) is src
        assert bit_equal(src.cpu(), want) and C.guards_intact(sbuf), f"apply_level L={L}, in place"


# ---------------------------------------------------------------------------------------------- the four-launch batch
def four_launches(eng, clean, rir, noise, rir_rows, mix_rows, params, staged, direct, mixture, reverberant, gains, early_taps, peak_limit=C.PEAK):
    """MixLoader's chain on caller-owned tensors: reverb -> the mix's two launches on the staged batch -> the target's level."""
    eng.reverb_windows(clean, rir, rir_rows, staged, direct, early_taps=early_taps)
    eng.mix_windows(staged.view(-1), noise, mix_rows, params, mixture, reverberant, gains, peak_limit=peak_limit)
    eng.apply_level(direct, gains)


# ---------------------------------------------------------------------------------------------- MixLoader with an RIR shard
def rir_corpus(tmp_path, rate=16000):
    """Three synthetic responses of 7 / 120 / 600 taps as 16-bit files (the second with 5 quieter samples in front of its peak, and a
    negative peak) + their list file.  Returns (list file, [the responses as pack_rir_shard must store them])."""
    rng = np.random.default_rng(9)
    lines, stored = [], []
    for i, K in enumerate((7, 120, 600)):
        h = _rir(rng, K, decay=K / 5.0) * 0.7
        if i == 1:
            h = np.concatenate([rng.uniform(-0.05, 0.05, 5), -h])[:K]
        p = tmp_path / f"rir{i}.wav"
        C._write_pcm16(p, h, rate=rate)
        q = C._quantised(h)
        peak = int(np.argmax(np.abs(q)))
        assert peak == (5 if i == 1 else 0)
        stored.append((q[peak:] / q[peak]).astype(np.float32))
        lines.append(str(p))
    lst = tmp_path / "rir.txt"
    lst.write_text("\n".join(lines) + "\n")
    return lst, stored


def check_loader(wd, tmp_path, engine, device):
    """MixLoader(rir_prefix=...) end to end.  The composition of the bars: the loader's chain is repeated from loader.last_draw stage by
    stage - the reverb launch on the drawn rir_rows is held to the reverb bar against the float64 oracle; what it wrote (float32, and
    bit-identical run to run) is the clean array of the mix oracle, to which mixture, a r and the gains are held with mix_cases' bars;
    the target is gains[:, 1] * direct of that launch bit for bit."""
    eng = C.engine_or_default(engine)
    cl_list, no_list, clean_items, noise_items = C.corpus(tmp_path)
    rir_list, stored = rir_corpus(tmp_path)
    cp, npfx, rp = str(tmp_path / "speech"), str(tmp_path / "noise"), str(tmp_path / "rir")
    assert wd.pack_mono_shard(str(cl_list), cp) == 6 and wd.pack_mono_shard(str(no_list), npfx) == 4 and wd.pack_rir_shard(str(rir_list), rp) == 3
    clean_flat, noise_flat, rir_flat = np.concatenate(list(clean_items.values())), np.concatenate(noise_items), np.fromfile(rp + ".f32", np.float32)
    idx = __import__("json").load(open(rp + ".index.json"))
    assert set(idx) == {"names", "starts", "lengths", "sample_rate"} and idx["names"] == ["rir0", "rir1", "rir2"] and idx["sample_rate"] == 16000
    assert idx["lengths"] == [7, 115, 600] and idx["starts"] == [0, 7, 122]
    assert np.array_equal(rir_flat, np.concatenate(stored)) and all(rir_flat[s] == 1.0 for s in idx["starts"])      # every item starts at its peak, h[0] == 1
    assert wd.pack_rir_shard(str(rir_list), rp + "_short", max_taps=100) == 3
    assert __import__("json").load(open(rp + "_short.index.json"))["lengths"] == [7, 100, 100]

    L, B, snr_range = 256, 4, (-5.0, 15.0)
    kw = dict(batch_size=B, sample_length=L, snr_db=snr_range, level_db=(-6.0, 6.0), p_clean=0.25, device=device, steps_per_epoch=3, engine=engine)
    plain = [(m.clone(), c.clone(), n) for m, c, n in wd.MixLoader(cp, npfx, seed=11, **kw)]
    plain_draws = []
    pl = wd.MixLoader(cp, npfx, seed=11, **kw)
    for _ in pl:
        plain_draws.append((pl.last_draw["rows"].clone(), pl.last_draw["params"].clone()))
        assert set(pl.last_draw) == {"rows", "params", "gains"}           # without rir_prefix none of the new keys appear
    cf, rf = torch.from_numpy(clean_flat).to(device), torch.from_numpy(rir_flat).to(device)
    dry_rows = wet_rows = 0
    for target, E in (("early", 32), ("dry", 1), ("reverberant", 1)):
        loader = wd.MixLoader(cp, npfx, seed=11, rir_prefix=rp, p_reverb=0.7, target=target, early_ms=2.0, **kw)
        assert loader.early_taps == E and len(loader) == 3
        for k, (mixture, tgt, names) in enumerate(loader):
            draw, label = loader.last_draw, f"loader {target} batch {k}"
            rows, params, rir_rows = draw["rows"].numpy(), draw["params"].numpy(), draw["rir_rows"].numpy()
            # the RIR draws come after the batch's other draws: the same seed starts with the same rows, params and items with and without
            # rir_prefix (from the second batch on the generator has moved by those draws)
            if k == 0:
                assert torch.equal(draw["rows"], plain_draws[0][0]) and torch.equal(draw["params"], plain_draws[0][1]) and names == plain[0][2]
            assert rir_rows.shape == (B, 4) and rir_rows.dtype == np.int64 and np.array_equal(rir_rows[:, 0], rows[:, 0])
            assert all(tuple(r[2:]) in {(0, 7), (7, 115), (122, 600), (0, 0), (7, 0), (122, 0)} for r in rir_rows)
            for b, nm in enumerate(names):                                 # the item start is the start of the item the row names
                assert rir_rows[b, 1] == idx_start(clean_items, nm) and 0 <= rir_rows[b, 0] - rir_rows[b, 1] <= len(clean_items[nm]) - L
            dry_rows, wet_rows = dry_rows + int((rir_rows[:, 3] == 0).sum()), wet_rows + int((rir_rows[:, 3] > 0).sum())
            # stage 1: the reverb launch on the drawn table against the float64 oracle
            staged, direct = torch.empty(B, 1, L, device=device), torch.empty(B, 1, L, device=device)
            eng.reverb_windows(cf, rf, draw["rir_rows"].to(device), staged, direct, early_taps=E)
            ref = R.reverb_reference(clean_flat, rir_flat, rir_rows, L, E)
            check_against(ref, clean_flat, staged, direct, label)
            # stages 2-3: the mix oracle on what stage 1 wrote
            staged_np = staged.cpu().numpy().reshape(-1)
            mrows = rows.copy()
            mrows[:, 0] = np.arange(B) * L
            mref = mix_ref.mix_reference(staged_np, noise_flat, mrows, params, L, loader.peak_limit)
            assert mixture.shape == (B, 1, L) and tgt.shape == (B, 1, L) and draw["reverberant"].shape == (B, 1, L) and mixture.device.type == device.type
            C.check_against(mref, mixture, draw["reverberant"], draw["gains"], label)
            # the SNR is defined over the reverberant window
            C.check_snr(mref, params, mixture, draw["reverberant"], engine, label)
            peak = np.abs(mixture.double().cpu().numpy()[:, 0]).max(axis=1)
            assert (peak <= float(np.float32(loader.peak_limit)) * (1.0 + 2.0 ** -22)).all(), (label, peak)
            # stage 4: the target
            a32 = draw["gains"][:, 1].cpu().numpy()
            if target == "reverberant":
                assert bit_equal(tgt, draw["reverberant"])
            else:
                assert bit_equal(tgt.cpu(), torch.from_numpy(a32[:, None, None] * direct.cpu().numpy())), f"{label}: the target is not a * direct"
            if target == "dry":                                            # h[0] == 1: the dry target is a * the clean window, exactly
                for b in range(B):
                    cs = int(rows[b, 0])
                    assert np.array_equal(tgt[b, 0].cpu().numpy(), a32[b] * clean_flat[cs:cs + L]), f"{label}: row {b}"
    assert dry_rows > 0 and wet_rows > 0
    # p_reverb = 0 reproduces the plain MixLoader bit for bit (mixture and, for a dry target, the clean batch) on the batch a seed starts with
    for seed in (11, 12, 13):
        m0, c0, n0 = next(iter(wd.MixLoader(cp, npfx, seed=seed, **kw)))
        dry = wd.MixLoader(cp, npfx, seed=seed, rir_prefix=rp, p_reverb=0.0, **kw)
        m, c, n = next(iter(dry))
        assert bit_equal(m, m0) and bit_equal(c, c0) and n == n0 and not dry.last_draw["rir_rows"][:, 3].any()
    # the same seed reproduces the reverberant batches bit for bit
    kwr = dict(kw, rir_prefix=rp, target="early", early_ms=2.0)
    for (m1, c1, n1), (m2, c2, n2) in zip(wd.MixLoader(cp, npfx, seed=5, **kwr), wd.MixLoader(cp, npfx, seed=5, **kwr)):
        assert bit_equal(m1, m2) and bit_equal(c1, c2) and n1 == n2 and not torch.equal(m1, plain[0][0])
    return cp, npfx, rp


def idx_start(clean_items, name):
    """First sample of item `name` inside the packed clean shard."""
    pos = 0
    for nm, x in clean_items.items():
        if nm == name:
            return pos
        pos += len(x)
    raise KeyError(name)
