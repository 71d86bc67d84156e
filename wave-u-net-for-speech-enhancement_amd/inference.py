"""chunked inference.

The reference enhances a long recording by zero-padding it to a multiple of `sample_length`, splitting it into
chunks and running the model on every chunk SEQUENTIALLY at batch 1 with a device->host copy per chunk
(/root/reference/enhancement.py:57-69, trainer/trainer.py:66-78).  In eval mode BatchNorm uses running statistics,
so chunks are independent: they are stacked into one [n_chunks, 1, sample_length] batch, run through ONE forward
(optionally in slabs of `max_batch` chunks) and trimmed back - same numbers, one launch sequence, one copy.

Two things beyond the reference, both opt-in (include/wunet_hip.h: wunet_chunk_gather / wunet_chunk_overlap_add, csrc/wunet_chunks.h):

  * overlapped chunks, `enhance(..., margin=m, fade=f, window="hann" | "linear")`.  Every conv of the network is zero-padded, so the
    samples next to a chunk edge are computed from padding, and disjoint chunks meet without any continuity constraint.  With
    L = sample_length and the hop H = L - 2 m - f (H >= 1, f <= H, so at most two chunks cover a sample) a recording of T samples has
    n = max(1, ceil((T - f) / H)) chunks; chunk k reads samples [k H - m, k H - m + L) (zeros outside the recording) and is trusted on
    [k H, k H + H + f): m samples at either edge are dropped, and the first f trusted samples cross-fade with the last f trusted
    samples of chunk k - 1, out = ramp[j] y_k + (1 - ramp[j]) y_(k-1).  The first chunk has no up-ramp, the last no down-ramp.  The
    ramp is a float32 table made here in float64 and rounded once ("linear": (j + 0.5) / f, "hann": sin^2(pi (j + 0.5) / (2 f))), so
    the window's shape is data for the kernel.  It costs L / H times the forwards.  m = f = 0 is the reference's padding and
    splitting, and runs the code path of before.  That seams are audible with trained weights is an expectation from the literature
    (Wave-U-Net's "context", Demucs' apply_model); it has not been measured on this project.
  * `enhance_many(model, recordings, ...)`: the chunks of many recordings of any lengths share the slabs of one pass - one flat array,
    one table of chunks, one table of recordings, one gather and one overlap-add - instead of one small forward per recording.
  * recordings at another sample rate than the model's, `enhance(..., sample_rate=48000)` / `enhance_many(..., sample_rates=[...])`:
    resampled to `model_rate` on the device (resample.py, wunet_resample_rows), enhanced by the paths above, unchanged, and resampled
    back to the rate and the length they came with.  The way back is never short: ceil(ceil(T u / d) d / u) >= T.  What lay above
    model_rate / 2 in the input is removed by the first filter and is not restored.
"""
import functools

import numpy as np
import torch

WINDOWS = ("hann", "linear")
_ALIGN = 4                      # recordings start at a multiple of 4 samples of the flat array: 16-byte accesses in the two kernels


def chunk_hop(sample_length, margin=0, fade=0, window="hann"):
    """The hop H = L - 2 m - f of the geometry above; ValueError for what the geometry does not allow."""
    for name, v in (("sample_length", sample_length), ("margin", margin), ("fade", fade)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"enhance: {name} must be an integer (got {v!r})")
    if sample_length < 1 or margin < 0 or fade < 0:
        raise ValueError(f"enhance: sample_length must be >= 1, margin and fade >= 0 (got {sample_length}, {margin}, {fade})")
    if window not in WINDOWS:
        raise ValueError(f"enhance: window must be one of {WINDOWS} (got {window!r})")
    hop = int(sample_length) - 2 * int(margin) - int(fade)
    if hop < 1:
        raise ValueError(f"enhance: the hop sample_length - 2 margin - fade must be >= 1 (got {sample_length} - 2 * {margin} - {fade} = {hop})")
    if fade > hop:
        raise ValueError(f"enhance: fade must not exceed the hop, 2 margin + 2 fade <= sample_length (got fade {fade}, hop {hop})")
    return hop


@functools.lru_cache(maxsize=8)
def _ramp_host(fade, window):
    x = (np.arange(fade, dtype=np.float64) + 0.5) / fade
    return (x if window == "linear" else np.sin(0.5 * np.pi * x) ** 2).astype(np.float32)


def chunk_ramp(fade, window="hann"):
    """The up-ramp of a cross-fade of `fade` samples as float32 [fade] (host tensor): float64, rounded once."""
    if window not in WINDOWS:
        raise ValueError(f"enhance: window must be one of {WINDOWS} (got {window!r})")
    return torch.from_numpy(_ramp_host(int(fade), window).copy())


def chunk_count(T, hop, fade):
    return max(1, -((fade - T) // hop))          # max(1, ceil((T - f) / H))


def chunk_tables(lengths, sample_length, margin=0, fade=0):
    """The tables of one pass over recordings of `lengths` samples: (rows int64 [n, 3] = flat start, T, chunk start; recs int64 [R, 4] =
    flat start, T, first chunk row, chunk count; total samples of the flat array).  A recording starts at a multiple of 4 samples."""
    hop = chunk_hop(sample_length, margin, fade)
    rows, recs, start = [], [], 0
    for T in lengths:
        T = int(T)
        if T < 1:
            raise ValueError(f"enhance: a recording needs at least one sample (got {T})")
        n = chunk_count(T, hop, fade)
        recs.append((start, T, len(rows), n))
        rows.extend((start, T, k * hop - margin) for k in range(n))
        start += -(-T // _ALIGN) * _ALIGN
    return np.asarray(rows, np.int64).reshape(-1, 3), np.asarray(recs, np.int64).reshape(-1, 4), start


def _engine_of(model, engine):
    if engine is not None:
        return engine
    override = getattr(model, "_engine_override", None)
    if override is not None:
        return override
    from .engine import default_engine
    return default_engine()


def _equal_slabs(n, max_batch):
    # equal slabs (586 chunks -> 196 + 196 + 194, not 256 + 256 + 74): no small ragged forward at the end, one context size
    nslab = (n + max_batch - 1) // max_batch
    return (n + nslab - 1) // nslab


def _table_driven(model, flat, lengths, sample_length, max_batch, margin, fade, window, engine):
    """gather -> slabs of chunks through the model -> overlap-add, for the recordings that lie in `flat` as chunk_tables places them.
    Returns the flat output (the layout of `flat`) and the recordings' starts."""
    engine = _engine_of(model, engine)
    dev = flat.device
    rows, recs, total = chunk_tables(lengths, sample_length, margin, fade)
    assert total == flat.numel() or (len(lengths) == 1 and flat.numel() == lengths[0])
    n = rows.shape[0]
    chunks = torch.empty(n, 1, sample_length, dtype=torch.float32, device=dev)
    engine.chunk_gather(flat, torch.from_numpy(rows).to(dev, non_blocking=True), chunks)
    step = _equal_slabs(n, max_batch)
    outs = [model(chunks[i:i + step]) for i in range(0, n, step)]
    y = outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
    out_flat = torch.empty(flat.numel(), dtype=torch.float32, device=dev)
    ramp = chunk_ramp(fade, window).to(dev, non_blocking=True) if fade else None
    engine.chunk_overlap_add(y.contiguous(), torch.from_numpy(recs).to(dev, non_blocking=True), out_flat, margin, fade, ramp, int(max(lengths)))
    return out_flat, recs[:, 0]


def _result_to_host(out_flat):
    """One pinned copy of the whole result."""
    if not out_flat.is_cuda:
        return out_flat
    host = torch.empty(out_flat.shape, dtype=out_flat.dtype, pin_memory=True)
    host.copy_(out_flat, non_blocking=True)
    torch.cuda.current_stream(out_flat.device).synchronize()
    return host


def _other_rate(sample_rate, model_rate, what="sample_rate"):
    """None when the recording is at the model's rate (or no rate is given), else the checked pair (rate, model rate); ValueError for a
    rate that is not a positive integer and for a pair whose filter is above the resampler's cap."""
    if sample_rate is None:
        return None
    from .resample import rate_ratio
    try:
        up, down = rate_ratio(sample_rate, model_rate)
    except ValueError as e:
        raise ValueError(f"enhance: {what} / model_rate: {e}") from None
    return None if up == down else (int(sample_rate), int(model_rate))


def _check_call(model, max_batch):
    if model.training:
        raise RuntimeError("enhance() needs model.eval(): chunks are only independent with running BatchNorm statistics")
    if isinstance(max_batch, bool) or not isinstance(max_batch, (int, np.integer)) or max_batch < 1:
        raise ValueError(f"enhance: max_batch must be an integer >= 1 (got {max_batch!r})")


@torch.no_grad()
def enhance(model, mixture, sample_length=16384, max_batch=256, to_host=False, margin=0, fade=0, window="hann", engine=None,
            sample_rate=None, model_rate=16000):
    """mixture: float32 [1, 1, T] (any T, the reference's batch-1 contract, enhancement.py:50) on the model's device.
    Returns the enhanced waveform [1, 1, T] - on the model's device, or with to_host=True as a host tensor (what the reference
    hands to the file writer, enhancement.py:66-71): every slab goes into one pinned buffer with an asynchronous copy,
    one synchronisation at the end instead of one per chunk.
    margin / fade / window: the overlapped chunks of this file's header (margin = fade = 0, the default: the reference's disjoint
    chunks, by the code path of before).  engine: the engine of the chunk and resampling kernels; default the model's own.
    sample_rate: the rate of `mixture` in Hz when it is not the model's (default None: the samples are run as they are).  With a rate
    other than `model_rate` the mixture is resampled to model_rate on the device, enhanced as above (sample_length, margin and fade
    count samples at model_rate) and resampled back to its own rate and its own T.  Content above model_rate / 2 is not restored:
    the output is band-limited to the model's band.  to_host=True is then one pinned copy of the result at the input's rate."""
    if mixture.dim() != 3 or mixture.shape[0] != 1 or mixture.shape[1] != 1:
        raise ValueError("Only support batch size is 1 in enhancement stage.")       # reference wording, enhancement.py:50
    _check_call(model, max_batch)
    chunk_hop(sample_length, margin, fade, window)
    T = mixture.shape[-1]
    rates = _other_rate(sample_rate, model_rate)
    if rates is not None:
        from .resample import resample
        if T < 1:
            raise ValueError("enhance: a recording needs at least one sample (got 0)")
        eng = _engine_of(model, engine)
        at_model = resample(mixture.to(torch.float32), rates[0], rates[1], engine=eng)
        enhanced = enhance(model, at_model, sample_length, max_batch, False, margin, fade, window, engine)
        back = resample(enhanced.to(torch.float32), rates[1], rates[0], engine=eng, length=T).view(-1)
        return (_result_to_host(back) if to_host else back).view(1, 1, T)
    if margin or fade:
        if T < 1:
            raise ValueError("enhance: a recording needs at least one sample (got 0)")
        flat = mixture.to(torch.float32).contiguous().view(-1)
        out_flat, _ = _table_driven(model, flat, [T], sample_length, max_batch, margin, fade, window, engine)
        return (_result_to_host(out_flat) if to_host else out_flat).view(1, 1, T)
    pad = (-T) % sample_length                                   # enhancement.py:57-59
    if pad:
        mixture = torch.cat([mixture, torch.zeros(1, 1, pad, device=mixture.device, dtype=mixture.dtype)], dim=-1)
    chunks = mixture.reshape(-1, 1, sample_length)               # == torch.split(..., sample_length, dim=-1) stacked
    n = chunks.shape[0]
    max_batch = _equal_slabs(n, max_batch)
    if to_host and mixture.is_cuda:
        host = torch.empty(n, 1, sample_length, dtype=mixture.dtype, pin_memory=True)
        for i in range(0, n, max_batch):
            host[i:i + max_batch].copy_(model(chunks[i:i + max_batch].contiguous()), non_blocking=True)
        torch.cuda.current_stream(mixture.device).synchronize()
        return host.reshape(1, 1, -1)[:, :, :T]
    outs = [model(chunks[i:i + max_batch].contiguous()) for i in range(0, n, max_batch)]
    enhanced = torch.cat(outs, dim=0).reshape(1, 1, -1)          # enhancement.py:68
    enhanced = enhanced[:, :, :T]                                # enhancement.py:69 trims the padding
    return enhanced.cpu() if to_host else enhanced


@torch.no_grad()
def enhance_many(model, recordings, sample_length=16384, max_batch=256, to_host=False, margin=0, fade=0, window="hann", engine=None,
                 sample_rates=None, model_rate=16000):
    """recordings: a list of float32 [1, 1, T_r] (or [T_r]) tensors of any lengths on the model's device.  Returns the list of enhanced
    waveforms in the same shapes (views of one buffer; with to_host=True of one pinned host buffer).  The chunks of all recordings are
    cut by one gather, run in slabs of `max_batch` chunks that recordings share, and put back by one overlap-add.  The gather and the
    overlap-add give a recording the bits enhance() gives it alone (at margin = fade = 0 too, where enhance() itself runs the code
    path of before), so the results are equal bit for bit whenever the model gives a row the same bits in a slab of another size.  In
    eval mode no row reads another, but the network's planner picks its GEMM tiling and reduction split by batch size (csrc/wunet_plan.cpp),
    so at other slab sizes a row may differ by the rounding of those sums.
    sample_rates: None (default: the samples are run as they are), one rate in Hz for all recordings or a list with one rate per
    recording.  Recordings at another rate than `model_rate` are resampled to it - one launch per distinct rate, written straight into
    the flat array of the pass - share the slabs with all the others at model_rate, and are resampled back to their own rate and
    length, again one launch per distinct rate (what enhance(..., sample_rate=) does for one recording, bit for bit)."""
    _check_call(model, max_batch)
    chunk_hop(sample_length, margin, fade, window)
    recordings = list(recordings)
    if not recordings:
        return []
    dev = recordings[0].device
    for x in recordings:
        if not (x.dim() == 1 or (x.dim() == 3 and x.shape[0] == 1 and x.shape[1] == 1)):
            raise ValueError("enhance_many: every recording must be [1, 1, T] or [T] (the reference's batch-1 contract, enhancement.py:50)")
        if x.dtype != torch.float32 or x.device != dev:
            raise ValueError("enhance_many: float32 recordings on one device expected")
        if x.shape[-1] < 1:
            raise ValueError("enhance: a recording needs at least one sample (got 0)")
    lengths = [int(x.shape[-1]) for x in recordings]
    if sample_rates is not None:
        if isinstance(sample_rates, (list, tuple)):
            if len(sample_rates) != len(recordings):
                raise ValueError(f"enhance_many: sample_rates needs one rate per recording (got {len(sample_rates)} for {len(recordings)})")
            pairs = [_other_rate(r, model_rate, "sample_rates") for r in sample_rates]
            if any(r is None for r in sample_rates):
                raise ValueError("enhance_many: sample_rates must not contain None")
        else:
            pairs = [_other_rate(sample_rates, model_rate, "sample_rates")] * len(recordings)
        if any(p is not None for p in pairs):
            return _enhance_many_rates(model, recordings, lengths, pairs, sample_length, max_batch, to_host, margin, fade, window, engine)
    _, recs, total = chunk_tables(lengths, sample_length, margin, fade)
    flat = torch.empty(total, dtype=torch.float32, device=dev)   # (the gaps between recordings are never read: the gather masks by T)
    for x, (start, T, _, _) in zip(recordings, recs.tolist()):
        flat[start:start + T].copy_(x.reshape(-1))
    out_flat, starts = _table_driven(model, flat, lengths, sample_length, max_batch, margin, fade, window, engine)
    if to_host:
        out_flat = _result_to_host(out_flat)
    return [out_flat[s:s + T].view(x.shape) for x, s, T in zip(recordings, starts.tolist(), lengths)]


def _enhance_many_rates(model, recordings, lengths, pairs, sample_length, max_batch, to_host, margin, fade, window, engine):
    """enhance_many where some recording is not at the model's rate.  pairs[r]: None or (rate, model rate) of recording r."""
    from .resample import resampled_length
    eng = _engine_of(model, engine)
    dev = recordings[0].device
    at_model = [T if p is None else resampled_length(T, p[0], p[1]) for T, p in zip(lengths, pairs)]
    _, recs, total = chunk_tables(at_model, sample_length, margin, fade)
    starts = recs[:, 0].tolist()
    groups = {}                                                   # rate -> the recordings at it, in their order
    for r, p in enumerate(pairs):
        groups.setdefault(None if p is None else p[0], []).append(r)
    model_rate = next(p[1] for p in pairs if p is not None)
    flat = torch.empty(total, dtype=torch.float32, device=dev)
    for rate, members in groups.items():
        if rate is None:
            for r in members:
                flat[starts[r]:starts[r] + lengths[r]].copy_(recordings[r].reshape(-1))
            continue
        src = torch.cat([recordings[r].reshape(-1) for r in members]) if len(members) > 1 else recordings[members[0]].contiguous().view(-1)
        offs = np.concatenate([[0], np.cumsum([lengths[r] for r in members])])
        table = np.asarray([(offs[k], lengths[r], starts[r], at_model[r]) for k, r in enumerate(members)], np.int64).reshape(-1, 4)
        eng.resample_rows(src, torch.from_numpy(table).to(dev, non_blocking=True), flat, rate, model_rate, max(at_model[r] for r in members))
    out_flat, _ = _table_driven(model, flat, at_model, sample_length, max_batch, margin, fade, window, engine)
    own = np.concatenate([[0], np.cumsum(lengths)])               # the results at their own rates, back to back
    final = torch.empty(int(own[-1]), dtype=torch.float32, device=dev)
    for rate, members in groups.items():
        if rate is None:
            for r in members:
                final[own[r]:own[r] + lengths[r]].copy_(out_flat[starts[r]:starts[r] + lengths[r]])
            continue
        table = np.asarray([(starts[r], at_model[r], own[r], lengths[r]) for r in members], np.int64).reshape(-1, 4)
        eng.resample_rows(out_flat, torch.from_numpy(table).to(dev, non_blocking=True), final, model_rate, rate, max(lengths[r] for r in members))
    if to_host:
        final = _result_to_host(final)
    return [final[int(own[r]):int(own[r]) + T].view(x.shape) for r, (x, T) in enumerate(zip(recordings, lengths))]
