"""The case table of the on-device BSS Eval SDR (bss_corr_kernel / bss_solve_kernel behind wunet_bss_sdr_forward), shared by
tests/test_bss_emu.py (CPU emulator) and tests/test_gpu_bss.py (MI355X): what runs, on which tensors, and the checks against the oracle
of tests/bss_ref.py.  `engine` None = the product's default engine.

The bar, per row, in dB (derived, not measured):   |out - arb| <= 2^-24 |arb| + max(K e_ref, floor),  K = 1
  arb    the score with every correlation, Levinson's recursion and the three quadratic forms in np.longdouble (the arbiter)
  e_ref  |float64 reference - arb| on that row: np.correlate, scipy.linalg.solve_toeplitz and the same formulas in double - what
         double arithmetic itself costs there
  floor  8 units of 2^-53 (10 / ln 10) E / R: R = E - 2 c'b + c'G c is formed from terms of the size of E, so one rounding of them
         is 2^-53 E, that is 2^-53 (10 / ln 10) E / R in dB (the "unit" below) - a floor for rows on which the reference happens to
         land on the arbiter
The first term is the single rounding to float32.  The second grants the kernel's double arithmetic - correlation partials per segment
added in segment order, then Levinson's recursion - the host reference's own distance from exact: the kernel runs the reference's
algorithm in the reference's precision, only the order of the sums differs.  K = 1, not the 8 of sos_cases.py, because of the first of
the two conditions that keep the bar honest, asserted on the CPU (test_bss_emu.py): on every scored row of every case the second term
is at most 2^-8 of the first - a float32-rounding bar - and the reference re-run with float32 correlation accumulators FAILS
check_against on every row of case c.  On case c's 60 dB row E / R is 1e6 and 2^-8 of the float32 rounding is 28 units, while the
reference itself is 4 - 17 units from the arbiter (4.0 at this tile; 8.8 and 16.7 with tiles of 512 and 1024, that is other row
lengths): a larger K does not fit under the first condition there.

Measured on the CPU (test_bss_emu.py::test_where_the_kernel_model_lands prints them; tile 2048): the float64 numpy model of the
kernel's scheme (bss_ref.kernel_model_row) and the reference against the arbiter, in units:
  case a             model 1.0, 6.6          reference 1.2, 0.4         (2^-8 of the float32 rounding: 3e5 units)
  case c, 16-bit     model 4.8, 0.5, 8.1     reference 6.0, 1.1, 4.0    (5e5, 9e4 and 27.7 units)
  case d             model 20.9, 11.2, 23.0  reference 11.4, 1.0, 5.1   (4e5 units)
  case e             model 14 - 40           reference 1.6 - 23         (5e5 units)
  case f (n = 1)     model 2.2, 76, 30       reference 7.2, 8.9, 1.1    (8e4 - 3e5 units)
With full float32 mantissas (all cases but c) the model's sequential sums of up to 2048 products per lag are up to ten times as far
from exact as np.correlate's blocked ones - tens of units against 1e5 units of float32 rounding, at E / R below 130.  Case c's rows
are 16-bit PCM, where every sum of products is exact in double and what is left is the solver's and the quadratic forms' rounding.
Before that change the 60 dB row measured: reference 36 units, model 24 (26 of the reference's 36 from np.correlate's sums alone) -
above the 28 units of the first condition whatever K >= 1 is; a recording's samples are 16-bit, so the case now is what a user scores.
On the emulator and on the MI355X the worst error / bar over all cases is 0.992: the rounding to float32.

What is not a number: a row whose reference or estimate is silent inside its length, or whose length is 0, is NaN and leaves the other
rows' bits alone.  estimate == reference bit for bit is +inf (the kernel sums E in the order of r[0] and b[0], so R = 0 exactly).  A row
that an n-tap filter of the reference fits exactly up to rounding - a length of one sample - has no score to compare: R is the rounding
of a full cancellation, at most a few dozen units of 2^-53 E, so the kernel must answer at least PERFECT_DB = 140 dB (R <= 1e-14 E, 90
such units) or +inf.

t is the tile, the samples of a row that one block of the correlation launch owns (wunet_bss_sdr_tile).
Every input is a view into a NaN-filled buffer (and starts 4-byte aligned only), so a read outside it turns the row into NaN; every
output is a view into a buffer of sentinels that must survive, and is NaN before the call."""
import functools

import numpy as np
import pytest
import scipy.signal
import torch

import bss_ref as R
import mix_cases as M

FS = 16000.0
K = 1.0
PERFECT_DB = 140.0
BEHIND = 1e3                 # what lies behind a ragged row's end (case d): a leak is a wrong number


def _white(rng, T):
    return rng.standard_normal(T) * 0.1


def _ar2(rng, T):
    r, th = 0.98, 2.0 * np.pi * 700.0 / FS
    return scipy.signal.lfilter([0.02], [1.0, -2.0 * r * np.cos(th), r * r], rng.standard_normal(T + 400))[400:]


def _lowpassed(rng, T):
    sos = scipy.signal.butter(8, 3400.0, "lowpass", fs=FS, output="sos")
    return scipy.signal.sosfilt(sos, rng.standard_normal(T + 400))[400:] * 0.1


def _noisy(rng, s, snr_db, colour=None):
    """s (through `colour`, an FIR) plus white noise at snr_db below it."""
    y = s if colour is None else scipy.signal.lfilter(colour, [1.0], s)
    noise = rng.standard_normal(len(s))
    noise *= np.sqrt(np.sum(y * y) / np.sum(noise * noise)) * 10.0 ** (-snr_db / 20.0)
    return y + noise


def _pcm16(x):
    return np.round(np.asarray(x) * 32768.0) / 32768.0


def _pair_rows(rng, T, kinds):
    clean, est = [], []
    for make, snr, colour in kinds:
        s = make(rng, T)
        clean.append(s)
        est.append(_noisy(rng, s, snr, colour))
    return np.stack(clean), np.stack(est)


def _case_a(rng, t):
    # T < n: everything is halo
    clean, est = _pair_rows(rng, 37, [(_white, 5.0, None), (_ar2, 12.0, None)])
    return clean, est, 512, None


def _case_b(T, n):
    def make(rng, t):
        # tile edges against the halo: the last segment holds one sample (t + 1), or the row ends one short of / on the tile
        clean, est = _pair_rows(rng, eval(T, {"t": t}), [(_white, 4.0, None), (_ar2, 15.0, np.array([0.8, 0.3, -0.2]))])
        return clean, est, n, None
    return make


def _case_c(rng, t):
    # three tiles and a bit, 512 taps: white noise, an AR(2) resonance, and an 8th-order 3.4 kHz low-passed reference under a 40-tap
    # coloured estimate at 60 dB - ill-conditioned, high SDR: a partial dropped at a segment boundary or a float32 accumulator shows
    # (the low-passed reference ends in 64 zeros: the 40 taps' tail then lies inside the row, or what the estimate's end cuts off
    #  would cap the score near 30 dB)
    # All three rows are 16-bit PCM, as recordings are: every product is a multiple of 2^-30 and every sum of them is exact in double, so
    # what is left of double arithmetic's error - in the reference and in the kernel - is the solver's and the quadratic forms', not
    # the luck of 6000-term sums that E / R = 1e6 would magnify (the other cases keep full float32 mantissas).
    T = 3 * t + 5
    colour = np.random.default_rng(77).standard_normal(40) * np.exp(-np.arange(40) / 8.0)
    clean, est = _pair_rows(rng, T, [(_white, 3.0, None), (_ar2, 20.0, None)])
    s = _pcm16(_lowpassed(rng, T))
    s[-64:] = 0.0
    clean, est = np.concatenate([_pcm16(clean), s[None]]), np.concatenate([est, _noisy(rng, s, 60.0, colour)[None]])
    assert np.abs(est).max() < 4.0 and np.abs(clean).max() < 4.0          # (sums of T products below 2^17: 47 bits)
    return clean, _pcm16(est), 512, None


D_N = 512


def _case_d(rng, t):
    # ragged lengths 0, 1, n - 1, n, T in one slab; BEHIND lies behind every row's end in both signals
    T = t + 300
    lengths = [0, 1, D_N - 1, D_N, T]
    clean, est = _pair_rows(rng, T, [(_white, 6.0, None)] * len(lengths))
    for i, L in enumerate(lengths):
        clean[i, L:] = BEHIND
        est[i, L:] = BEHIND
    return clean, est, D_N, lengths


E_ZERO_REF, E_ZERO_EST, E_EQUAL = 1, 3, 5


def _case_e(rng, t):
    # degenerate rows between ordinary ones: a silent reference, a silent estimate, estimate == reference
    clean, est = _pair_rows(rng, 700, [(_white, 8.0, None), (_white, 8.0, None), (_ar2, 8.0, None), (_white, 8.0, None), (_white, 8.0, None),
                                       (_ar2, 8.0, None), (_white, 8.0, None)])
    clean[E_ZERO_REF] = 0.0
    est[E_ZERO_EST] = 0.0
    est[E_EQUAL] = clean[E_EQUAL]
    return clean, est, 64, None


def _case_f(rng, t):
    # one tap: SI-SDR without mean removal (rows with a mean, so that the two would differ otherwise)
    clean, est = _pair_rows(rng, t + 77, [(_white, 0.7, None), (_ar2, 25.0, None), (_lowpassed, 45.0, None)])
    return clean + 0.05, est + 0.03, 1, None


B_LENGTHS = ("t - 1", "t", "t + 1")
B_TAPS = (1, 5, 512)
CASES = {"a": _case_a, "c": _case_c, "d": _case_d, "e": _case_e, "f": _case_f}
for _i, _T in enumerate(B_LENGTHS):
    for _n in B_TAPS:
        CASES[f"b{_i}_{_n}"] = _case_b(_T, _n)


@functools.lru_cache(maxsize=None)
def case(name, t):
    """The inputs of one case (float32 numpy arrays [rows, T]) - built once, shared, never modified."""
    clean, est, n, lengths = CASES[name](np.random.default_rng(sorted(CASES).index(name) + 500), t)
    d = {"clean": clean.astype(np.float32), "est": est.astype(np.float32), "n": n,
         "lengths": None if lengths is None else np.asarray(lengths, np.int64)}
    if name == "e":
        d["est"][E_EQUAL] = d["clean"][E_EQUAL]
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name, t):
    d = case(name, t)
    return R.bss_reference(d["clean"], d["est"], d["n"], d["lengths"], K=K)


def tile(engine):
    t = M.engine_or_default(engine).bss_sdr_tile(512)
    assert t >= 512 and t == M.engine_or_default(engine).bss_sdr_tile(1)
    return t


def run(engine, device, d, rows=None):
    """One call on guarded tensors (of the rows `rows`: default all): float32 [rows] on `device`."""
    clean, est = (d["clean"], d["est"]) if rows is None else (d["clean"][rows], d["est"][rows])
    n_rows, T = clean.shape
    cl = M.guarded_flat(clean.reshape(-1), device).view(n_rows, T)
    es = M.guarded_flat(est.reshape(-1), device).view(n_rows, T)
    lengths = None
    if d["lengths"] is not None:
        lengths = torch.from_numpy(np.array(d["lengths"] if rows is None else d["lengths"][rows])).to(device)
    out, buf = M.guarded_out((n_rows,), device)
    got = M.engine_or_default(engine).bss_sdr(cl, es, d["n"], lengths=lengths, out=out)
    assert got is out and M.guards_intact(buf), "a guard float was overwritten"
    return out


def perfect(ref, i):
    """Row i is fitted exactly up to rounding: no score to compare (this file's docstring)."""
    return not np.isnan(ref["ratio"][i]) and abs(ref["ratio"][i]) > 2.0 ** 40


def check_against(ref, out, label, rows=None):
    """The bar of this file's docstring on every row (of `rows`: default all); prints the error / bar per row first."""
    o = np.asarray(out, np.float64) if isinstance(out, np.ndarray) else out.double().cpu().numpy()
    rows = list(range(len(o))) if rows is None else list(rows)
    figures = []
    for i in rows:
        if np.isnan(ref["ratio"][i]):                    # (not a live row)
            figures.append("nan" if np.isnan(o[i]) else "NOT nan")
        elif perfect(ref, i):
            figures.append("perfect" if o[i] >= PERFECT_DB else "NOT perfect")
        else:
            figures.append("%.3f" % (abs(float(np.longdouble(o[i]) - ref["arb"][i])) / ref["bar"][i]) if np.isfinite(o[i]) else "NOT finite")
    print(f"{label}: out {[float(o[i]) for i in rows]} error / bar per row {figures}")
    for f in figures:
        assert f in ("nan", "perfect") or (not f.startswith("NOT") and float(f) <= 1.0), (label, figures)


def require_long_double():
    if not R.HAVE_LONGDOUBLE:
        pytest.skip("np.longdouble has fewer than 64 bits of mantissa here: no arbiter above float64")
    assert np.finfo(np.longdouble).nmant >= 63


def check_case(name, engine, device):
    require_long_double()
    t = tile(engine)
    d, ref = case(name, t), reference(name, t)
    rows = d["clean"].shape[0]
    out = run(engine, device, d)
    assert out.shape == (rows,) and out.dtype == torch.float32 and out.device.type == device.type
    check_against(ref, out, f"case {name}")
    again = run(engine, device, d)
    assert M.bit_equal(out, again), f"case {name}: two runs differ"
    o = out.cpu().numpy()
    if name == "a":
        assert d["clean"].shape[1] < d["n"]
    if name == "d":
        assert list(d["lengths"]) == [0, 1, D_N - 1, D_N, d["clean"].shape[1]] and d["clean"].shape[1] > t
        assert np.isnan(o[0]) and perfect(ref, 1) and np.isfinite(o[2:]).all() and (np.abs(o[2:]) < 30.0).all()
    if name == "e":
        assert np.isnan(o[E_ZERO_REF]) and np.isnan(o[E_ZERO_EST]) and np.isposinf(o[E_EQUAL])
        # the ordinary rows are what they are without the degenerate rows in the call, bit for bit
        plain = [i for i in range(rows) if i not in (E_ZERO_REF, E_ZERO_EST, E_EQUAL)]
        alone = run(engine, device, d, rows=plain)
        assert np.isfinite(o[plain]).all() and M.bit_equal(out[plain], alone)
    if name == "f":
        # n = 1 is SI-SDR without mean removal and without eps: the existing kernel's score lies within the same bar of the arbiter, so
        # the two lie within both bars of each other
        cl, es = torch.from_numpy(np.array(d["clean"])).to(device), torch.from_numpy(np.array(d["est"])).to(device)
        si = M.metrics().si_sdr(cl, es, zero_mean=False, eps=0.0, engine=engine)
        check_against(ref, si, "case f, metrics.si_sdr(zero_mean=False, eps=0)")
        diff = np.abs(si.double().cpu().numpy() - out.double().cpu().numpy())
        print(f"case f: |sdr(n = 1) - si_sdr| / (2 bar) per row {['%.3f' % v for v in diff / (2.0 * ref['bar'])]}")
        assert (diff <= 2.0 * ref["bar"]).all()
    return out


# ---------------------------------------------------------------------------------------------- the Trainer's "validation.sdr" key
class _HostReads:
    """Counts the device->host reads (tolist / item / cpu / numpy on a tensor of `device`) inside a with block."""

    def __init__(self, device):
        self.device, self.count, self._saved = device, 0, {}

    def __enter__(self):
        for name in ("tolist", "item", "cpu", "numpy"):
            original = getattr(torch.Tensor, name)
            self._saved[name] = original

            def counted(t, *a, _original=original, **kw):
                if t.device.type == self.device.type:
                    self.count += 1
                return _original(t, *a, **kw)
            setattr(torch.Tensor, name, counted)
        return self

    def __exit__(self, *exc):
        for name, original in self._saved.items():
            setattr(torch.Tensor, name, original)
        return False


def check_trainer(engine, device, tmp_path):
    """A three-layer Model, three validation recordings cut from mix_cases' tiny corpus (300 - 700 samples, noise added).  One validation
    epoch with "sdr": "report", one with "sdr": "score" and "recordings_per_pass": 2 (a pass of two and a pass of one: a ragged slab
    through `lengths`): the figures are metrics.sdr of the separately enhanced recordings, the training flags are restored, an epoch reads
    the device once (counted where the device is not the host), and bad values raise in the constructor."""
    import importlib

    from conftest import PKG_NAME
    trainer_mod, optim_mod = importlib.import_module(PKG_NAME + ".trainer"), importlib.import_module(PKG_NAME + ".optim")
    loss_mod, model_mod = importlib.import_module(PKG_NAME + ".loss"), importlib.import_module(PKG_NAME + ".model")
    inference, metrics = importlib.import_module(PKG_NAME + ".inference"), M.metrics()
    _, _, clean_items, noise_items = M.corpus(tmp_path)
    noise = np.concatenate(noise_items)
    recordings = []
    for name, x in list(clean_items.items())[:3]:
        mixture = (x + 0.5 * np.resize(noise, len(x))).astype(np.float32)
        recordings.append((torch.from_numpy(mixture).view(1, 1, -1), torch.from_numpy(np.array(x)).view(1, 1, -1), name))
    assert len({r[0].shape[-1] for r in recordings}) == 3                 # ragged
    sl = 64

    def trainer(name, validation):
        torch.manual_seed(0)
        m = model_mod.Model(n_layers=3, channels_interval=4).train()
        crit, opt = loss_mod.mse_loss(), None
        if engine is not None:
            m._engine_override = crit._engine_override = engine
        opt = optim_mod.FusedAdam(m.parameters(), lr=1e-3)
        if engine is not None:
            opt._engine_override = engine
        cfg = {"root_dir": str(tmp_path), "experiment_name": name,
               "trainer": {"epochs": 1, "validation": dict({"metric": "si_sdr", "interval": 1, "custom": {"sample_length": sl}}, **validation)}}
        return trainer_mod.Trainer(cfg, False, m, crit, opt, [], recordings)

    def expected(tr, n, per_pass=None):
        """(mean noisy SDR, mean enhanced SDR) with every recording scored by a call of its own, as the trainer averages them.  The
        recordings are enhanced as the trainer enhances them - one by one, or per_pass at a time in enhance_many's shared slabs (the
        network's kernels round differently at another batch size) - and then scored apart, unpadded."""
        model = tr.model.eval()
        on_device = [(mixture.to(device), clean.to(device)) for mixture, clean, _ in recordings]
        if per_pass is None:
            enhanced = [inference.enhance(model, mixture, sl) for mixture, _ in on_device]
        else:
            enhanced = []
            for k in range(0, len(on_device), per_pass):
                enhanced += inference.enhance_many(model, [mixture for mixture, _ in on_device[k:k + per_pass]], sl)
        rows = [torch.cat([metrics.sdr(clean, mixture, n, engine=engine), metrics.sdr(clean, enh, n, engine=engine)])
                for (mixture, clean), enh in zip(on_device, enhanced)]
        model.train()
        return torch.stack(rows).double().mean(dim=0).tolist()

    def close(a, b):
        return abs(a - b) <= 1e-12 * max(1.0, abs(b))

    plain = trainer("plain", {})
    assert plain.validation_sdr_mode is None and plain._validation_epoch(1) == plain.validation_scores[0] and plain.validation_sdr == []

    report = trainer("report", {"sdr": "report"})
    report.model.encoder[1].main[1].eval()                               # a frozen BatchNorm layer stays frozen
    flags = [(mod, mod.training) for mod in report.model.modules()]
    with _HostReads(device) as reads:
        score = report._validation_epoch(1)
    assert all(mod.training == was for mod, was in flags)
    assert device.type == "cpu" or reads.count == 1, reads.count
    assert score == plain.validation_scores[0] and report.validation_scores == [score]          # the score is left alone
    want = expected(report, 512)
    print(f'"sdr": "report": validation_sdr {report.validation_sdr}, the recordings one by one {want}')
    assert len(report.validation_sdr) == 1 and all(close(a, b) for a, b in zip(report.validation_sdr[0], want))
    assert all(np.isfinite(want))

    scored = trainer("scored", {"sdr": "score", "sdr_filter_length": 64, "recordings_per_pass": 2})
    flags = [(mod, mod.training) for mod in scored.model.modules()]
    with _HostReads(device) as reads:
        score = scored._validation_epoch(1)
    assert all(mod.training == was for mod, was in flags)
    assert device.type == "cpu" or reads.count == 1, reads.count
    want = expected(scored, 64, per_pass=2)
    print(f'"sdr": "score", two recordings per pass: score {score}, validation_sdr {scored.validation_sdr}, one by one {want}')
    assert close(score, want[1]) and scored.validation_scores == [score] and scored.validation_sdr[0][1] == score
    assert close(scored.validation_sdr[0][0], want[0])
    assert scored._is_best(score)

    for validation in ({"sdr": "yes"}, {"sdr": True}, {"sdr": "score", "stoi": "score"}, {"sdr": "report", "sdr_filter_length": 0},
                       {"sdr": "report", "sdr_filter_length": 513}, {"sdr": "report", "sdr_filter_length": 64.0}, {"sdr_filter_length": 64}):
        with pytest.raises(ValueError, match="validation"):
            trainer("bad", validation)
    with pytest.raises(ValueError, match="validation"):
        trainer_mod.Trainer({"trainer": {"epochs": 1, "validation": {"sdr": "report"}}}, False, model_mod.Model(n_layers=3, channels_interval=4),
                            loss_mod.mse_loss(), optim_mod.FusedAdam(model_mod.Model(n_layers=3, channels_interval=4).parameters(), lr=1e-3), [], recordings)
    trainer("both", {"sdr": "report", "stoi": "score"})                   # one of the two may be the score
