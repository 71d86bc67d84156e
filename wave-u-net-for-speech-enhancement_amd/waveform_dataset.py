"""the data input path either side of the hot loop.

Two pieces, both float32 mono like the reference's items:

* `Dataset` - drop-in for the reference's dataset/waveform_dataset.py:10-67 (same constructor arguments, same list
  file format "<noisy path><space><clean path>", same item contract `(mixture[1,T], clean[1,T], filename)`, same
  aligned random crop as util/utils.py:101-113 including its use of `np.random.randint`, so a seeded run crops the
  same windows).  The reference decodes with librosa.load(sr=None); this image has no audio library, so RIFF/WAVE
  files are parsed here (PCM 8/16/24/32 bit and IEEE float 32/64, any channel count -> mono mean, no resampling -
  what librosa.load(sr=None, mono=True) returns for such files).  The three pack_* functions below take `sample_rate=` to bring
  files of other rates to the shard's rate on the device (resample.py) while they are packed.

      "train_dataset": {"module": "wave-u-net-for-speech-enhancement_amd.waveform_dataset", "main": "Dataset",
                        "args": {"dataset": "~/train.txt", "limit": null, "offset": 0, "sample_length": 16384, "mode": "train"}}

* `pack_shard` + `ShardLoader` - the MI355X-first form of the same path ("pre-decoded memory-mapped
  float32 shards + on-GPU crop").  Per-item librosa decoding in 40 worker processes cannot feed >50 k frames/s; a shard
  is the whole list decoded ONCE into two flat float32 files (noisy, clean) plus an index, memory-mapped, uploaded to HBM
  once (a 100-hour 16 kHz corpus is 46 GB of the 288 GB) and every batch is one gather on the GPU: random item, random
  aligned start, `[B,1,sample_length]` mixture and clean, no host work and no H2D copy per step.  Iterating it yields
  the DataLoader batch contract `(mixture, clean, names)` the reference trainer loop consumes (trainer/trainer.py:30).

* `pack_mono_shard` + `MixLoader` - mixtures made on the device: a clean corpus and a noise corpus, each one flat float32 shard in
  HBM, combined per row at a freshly drawn SNR and level every step (include/wunet_hip.h: wunet_mix_windows - two launches per
  batch).  The host draws integers and a few floats per batch; the same batch contract comes out.

* `pack_rir_shard` + `MixLoader(rir_prefix=...)` - reverberant speech: a third resident shard of room impulse responses, every clean
  window convolved with a drawn response on the device before the noise is added (wunet_reverb_windows, one more launch).
"""
import json
import os
import struct

import numpy as np
import torch
from torch.utils import data

from . import _lib


# ---------------------------------------------------------------------------------------------- WAV decoding
def read_wav(path):
    """float32 mono samples and the sample rate of a RIFF/WAVE file (what librosa.load(path, sr=None) returns)."""
    with open(os.path.abspath(os.path.expanduser(path)), "rb") as f:
        blob = f.read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"WAVE":
        raise ValueError(f"{path}: not a RIFF/WAVE file")
    pos, fmt, payload = 12, None, None
    while pos + 8 <= len(blob):
        tag, size = blob[pos:pos + 4], struct.unpack("<I", blob[pos + 4:pos + 8])[0]
        body = blob[pos + 8:pos + 8 + size]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
            if fmt[0] == 0xFFFE and len(body) >= 26:           # WAVE_FORMAT_EXTENSIBLE: the real tag leads the GUID
                fmt = (struct.unpack("<H", body[24:26])[0],) + fmt[1:]
        elif tag == b"data":
            payload = body
        pos += 8 + size + (size & 1)
    if fmt is None or payload is None:
        raise ValueError(f"{path}: missing fmt or data chunk")
    tag, channels, rate, _, _, bits = fmt
    if tag == 1:                                               # integer PCM
        if bits == 8:
            x = (np.frombuffer(payload, np.uint8).astype(np.float32) - 128.0) / 128.0
        elif bits == 16:
            x = np.frombuffer(payload[:len(payload) // 2 * 2], "<i2").astype(np.float32) / 32768.0
        elif bits == 24:
            b = np.frombuffer(payload[:len(payload) // 3 * 3], np.uint8).reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            x = (v - ((v & 0x800000) << 1)).astype(np.float32) / 8388608.0
        elif bits == 32:
            x = (np.frombuffer(payload[:len(payload) // 4 * 4], "<i4").astype(np.float64) / 2147483648.0).astype(np.float32)
        else:
            raise ValueError(f"{path}: unsupported PCM width {bits}")
    elif tag == 3:                                             # IEEE float
        if bits not in (32, 64):
            raise ValueError(f"{path}: unsupported float width {bits}")
        x = np.frombuffer(payload[:len(payload) // (bits // 8) * (bits // 8)], "<f4" if bits == 32 else "<f8").astype(np.float32)
    else:
        raise ValueError(f"{path}: unsupported WAVE format tag {tag}")
    if channels > 1:
        x = x[:len(x) // channels * channels].reshape(-1, channels).mean(axis=1).astype(np.float32)
    return np.ascontiguousarray(x), rate


# ---------------------------------------------------------------------------------------------- the list file and the item contract
class PairList:
    """The reference's list file - one "<noisy path><space><clean path>" per line (dataset/waveform_dataset.py:15-29), `offset` lines
    skipped, then at most `limit` kept - parsed once into records.  Both readers of the format use it: `Dataset` (decode per item,
    the reference's contract) and `pack_shard` (decode once into a shard)."""

    def __init__(self, list_file, limit=None, offset=0):
        with open(os.path.abspath(os.path.expanduser(list_file)), "r") as f:
            rows = [ln.rstrip("\n") for ln in f][offset:]
        self.rows = rows[:limit] if limit else rows

    def __len__(self):
        return len(self.rows)

    def pair(self, k):
        """(noisy path, clean path, item name = the noisy file's stem) of record k."""
        noisy, clean = self.rows[k].split(" ")
        return noisy, clean, os.path.splitext(os.path.basename(noisy))[0]

    def decode(self, k):
        """Both signals of record k as float32 mono + their sample rates + the item name."""
        noisy, clean, name = self.pair(k)
        (x, rx), (y, ry) = read_wav(noisy), read_wav(clean)
        return x, y, rx, ry, name


def aligned_window_start(n_a, n_b, sample_length):
    """First sample of the ONE random window both signals are cut at (util/utils.py:101-113).  The draw is `np.random.randint` over
    the n - L + 1 valid starts, as in the reference: a run seeded with np.random.seed crops the windows the reference would (the
    device-side form of the same draw is ShardLoader.draw).  The two assertion texts are the reference's."""
    assert n_a == n_b, "Inconsistent dataset length, unable to sampling"
    assert n_a >= sample_length, f"len(data_a) is {n_a}, sample_length is {sample_length}."
    return int(np.random.randint(n_a - sample_length + 1))


class Dataset(data.Dataset):
    """Plugin-compatible with the reference's dataset/waveform_dataset.py:10-67: constructor arguments, `mode` check, and the item
    `(mixture [1, T], clean [1, T], filename)` - a random aligned window of `sample_length` in "train" mode, the whole file in
    "validation" mode."""
    MODES = ("train", "validation")

    def __init__(self, dataset, limit=None, offset=0, sample_length=16384, mode="train"):
        super().__init__()
        assert mode in self.MODES, "Mode must be one of 'train' or 'validation'."
        self.pairs = PairList(dataset, limit, offset)
        self.sample_length, self.mode = sample_length, mode

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, item):
        mixture, clean, _, _, name = self.pairs.decode(item)
        if self.mode == "train":
            s = aligned_window_start(len(mixture), len(clean), self.sample_length)
            mixture, clean = mixture[s:s + self.sample_length], clean[s:s + self.sample_length]
        return mixture[None, :], clean[None, :], name


# ---------------------------------------------------------------------------------------------- shards
def _target_rate(sample_rate):
    if sample_rate is None:
        return None
    from .resample import rate_ratio
    rate_ratio(sample_rate, sample_rate)                       # (ValueError for what is not a positive integer)
    return int(sample_rate)


def _at_rate(x, rate, target, engine):
    """The decoded file x (float32, `rate` Hz) at `target` Hz: resampled on the device (resample.py) when the two differ."""
    if rate == target:
        return x
    from .resample import resample
    if engine is None:
        from .engine import default_engine
        engine = default_engine()
    if len(x) == 0:
        return x
    dev = torch.device("cpu") if engine.host_memory else torch.device("cuda", torch.cuda.current_device())
    return resample(torch.from_numpy(x).to(dev), rate, target, engine=engine).cpu().numpy()


def pack_shard(dataset, prefix, limit=None, offset=0, sample_rate=None, engine=None):
    """Decode every pair of the list file once into `<prefix>.noisy.f32`, `<prefix>.clean.f32` (flat float32) and
    `<prefix>.index.json` ({"names", "starts", "lengths", "sample_rate"}).  Returns the number of items.
    sample_rate: the rate of the shard in Hz.  A file at another rate is resampled to it on the device (`engine`: default the
    process's) before it is written, so a list of mixed rates is legal and the index records `sample_rate`.  Default None: every file
    must have one rate, which the index records - nothing is resampled."""
    pairs = PairList(dataset, limit, offset)
    target = _target_rate(sample_rate)
    names, starts, lengths, rate, pos = [], [], [], target, 0
    with open(prefix + ".noisy.f32", "wb") as fn, open(prefix + ".clean.f32", "wb") as fc:
        for k in range(len(pairs)):
            mixture, clean, r0, r1, name = pairs.decode(k)
            if target is not None:
                mixture, clean = _at_rate(mixture, r0, target, engine), _at_rate(clean, r1, target, engine)
                r0 = r1 = target
            assert len(mixture) == len(clean), f"Inconsistent dataset length: {pairs.pair(k)[0]}"
            assert r0 == r1 and (rate is None or rate == r0), f"mixed sample rates: {pairs.pair(k)[0]}"
            rate = r0
            fn.write(mixture.tobytes())
            fc.write(clean.tobytes())
            names.append(name)
            starts.append(pos)
            lengths.append(len(mixture))
            pos += len(mixture)
    with open(prefix + ".index.json", "w") as f:
        json.dump({"names": names, "starts": starts, "lengths": lengths, "sample_rate": rate}, f)
    return len(names)


class ShardLoader:
    """Batches of aligned random crops cut on the device from a shard that lives in device memory.

    for mixture, clean, names in ShardLoader(prefix, batch_size=64, device="cuda:0"): ...   # [B,1,L] float32 each
    Items shorter than `sample_length` are never drawn (the reference asserts on them).  Every rank of a data-parallel
    job passes its own `seed` (e.g. seed + rank) and draws independently, like shuffled per-rank loaders."""

    def __init__(self, prefix, batch_size, sample_length=16384, device="cpu", seed=0, steps_per_epoch=None, engine=None):
        idx = json.load(open(prefix + ".index.json"))
        self.names = idx["names"]
        starts = np.asarray(idx["starts"], np.int64)
        lengths = np.asarray(idx["lengths"], np.int64)
        usable = np.nonzero(lengths >= sample_length)[0]
        if len(usable) == 0:
            raise ValueError("no item is at least sample_length long")
        self.device = torch.device(device)
        total = int(starts[-1] + lengths[-1]) if len(starts) else 0
        self.noisy = self._resident(prefix + ".noisy.f32", total)                       # one upload; stays resident
        self.clean = self._resident(prefix + ".clean.f32", total)
        self.usable = torch.from_numpy(usable)
        self.starts = torch.from_numpy(starts)
        self.spare = torch.from_numpy(lengths - sample_length + 1)                      # number of valid window starts per item
        self.batch_size, self.sample_length = batch_size, sample_length
        self.steps = steps_per_epoch if steps_per_epoch is not None else max(1, len(usable) // batch_size)
        self.gen = torch.Generator().manual_seed(seed)
        self.engine = engine                     # tests inject the emulator engine; a GPU loader takes the default (HIP) engine

    UPLOAD_CHUNK = 1 << 26          # floats per staged piece (256 MB): the corpus is never copied into host RAM as a whole

    def _resident(self, path, total):
        """The flat float32 file as a tensor on self.device.  The file is memory-mapped (copy-on-write, so torch gets a writable
        view without touching the pages); a CPU loader uses the mapping itself, a GPU loader uploads it piece by piece."""
        mm = np.memmap(path, np.float32, "c", shape=(total,))
        if self.device.type == "cpu":
            return torch.from_numpy(mm)
        out = torch.empty(total, dtype=torch.float32, device=self.device)
        for a in range(0, total, self.UPLOAD_CHUNK):
            b = min(total, a + self.UPLOAD_CHUNK)
            out[a:b].copy_(torch.from_numpy(mm[a:b]))
        return out

    def __len__(self):
        return self.steps

    def draw(self):
        """(item ids, window starts inside the flat arrays) of one batch - host-side integers only."""
        pick = self.usable[torch.randint(len(self.usable), (self.batch_size,), generator=self.gen)]
        inner = (torch.rand(self.batch_size, generator=self.gen, dtype=torch.float64) * self.spare[pick].double()).long()
        inner = torch.minimum(inner, self.spare[pick] - 1)
        return pick, self.starts[pick] + inner

    def crop(self, first):
        """The batch of aligned windows that start at `first` (host int64 [B], offsets into the flat arrays): mixture and clean
        [B, 1, L].  On a GPU this is ONE launch of the HIP crop kernel behind the C ABI (wunet_crop_windows, csrc/wunet_ops.cpp);
        a host loader (device="cpu": the reference's DataLoader worker side) slices the memory map."""
        B, L = first.numel(), self.sample_length
        if self.device.type != "cuda" and self.engine is None:
            index = first[:, None] + torch.arange(L)[None, :]
            return self.noisy[index].unsqueeze(1), self.clean[index].unsqueeze(1)
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        mixture = torch.empty(B, 1, L, dtype=torch.float32, device=self.device)
        clean = torch.empty(B, 1, L, dtype=torch.float32, device=self.device)
        starts = first.to(self.device, non_blocking=True)
        self.engine.crop_windows(self.noisy, self.clean, starts, mixture, clean)
        return mixture, clean

    def __iter__(self):
        for _ in range(self.steps):
            pick, first = self.draw()
            mixture, clean = self.crop(first)
            yield mixture, clean, [self.names[i] for i in pick.tolist()]


# ---------------------------------------------------------------------------------------------- mixtures made on the device
def pack_mono_shard(list_file, prefix, limit=None, offset=0, sample_rate=None, engine=None):
    """Decode every file of the list (one path per line; `offset` lines skipped, then at most `limit` kept) once into `<prefix>.f32`
    (flat float32) and `<prefix>.index.json` (pack_shard's keys: {"names", "starts", "lengths", "sample_rate"}; an item's name is its
    file's stem).  The clean corpus and the noise corpus of a MixLoader are each one such shard.  Returns the number of items.
    sample_rate / engine: pack_shard's - with a rate, files at other rates are resampled to it on the device."""
    with open(os.path.abspath(os.path.expanduser(list_file)), "r") as f:
        paths = [ln.strip() for ln in f][offset:]
    paths = [p for p in (paths[:limit] if limit else paths) if p]
    target = _target_rate(sample_rate)
    names, starts, lengths, rate, pos = [], [], [], target, 0
    with open(prefix + ".f32", "wb") as out:
        for path in paths:
            x, r = read_wav(path)
            if target is not None:
                x, r = _at_rate(x, r, target, engine), target
            assert rate is None or rate == r, f"mixed sample rates: {path}"
            rate = r
            out.write(x.tobytes())
            names.append(os.path.splitext(os.path.basename(path))[0])
            starts.append(pos)
            lengths.append(len(x))
            pos += len(x)
    with open(prefix + ".index.json", "w") as f:
        json.dump({"names": names, "starts": starts, "lengths": lengths, "sample_rate": rate}, f)
    return len(names)


SOS_MAX_LEAD = _lib.CONSTANTS["WUNET_SOS_MAX_LEAD"]
RIR_MAX_TAPS = _lib.CONSTANTS["WUNET_REVERB_MAX_TAPS"]


def pack_rir_shard(list_file, prefix, max_taps=8192, limit=None, offset=0, sample_rate=None, engine=None):
    """Room impulse responses for MixLoader(rir_prefix=...): pack_mono_shard's list handling (one path per line) and files (`<prefix>.f32`,
    `<prefix>.index.json` with the same keys), but every response is cut to start at its direct path and scaled to it: with
    p = argmax |h| the stored item is h[p : p + max_taps] / h[p], so h[0] == 1.0.  The propagation delay is gone - a dry target stays
    time-aligned with the reverberant signal - and so is the response's own gain.  Returns the number of items.
    sample_rate / engine: pack_shard's - with a rate, a response at another rate is resampled to it on the device first, so the direct
    path is found, and max_taps counted, at the shard's rate."""
    if not 1 <= max_taps <= RIR_MAX_TAPS:
        raise ValueError(f"max_taps must be in [1, {RIR_MAX_TAPS}], got {max_taps}")
    with open(os.path.abspath(os.path.expanduser(list_file)), "r") as f:
        paths = [ln.strip() for ln in f][offset:]
    paths = [p for p in (paths[:limit] if limit else paths) if p]
    target = _target_rate(sample_rate)
    names, starts, lengths, rate, pos = [], [], [], target, 0
    with open(prefix + ".f32", "wb") as out:
        for path in paths:
            h, r = read_wav(path)
            if target is not None:
                h, r = _at_rate(h, r, target, engine), target
            if rate is not None and rate != r:
                raise ValueError(f"mixed sample rates: {path} ({r} vs {rate})")
            rate = r
            p = int(np.argmax(np.abs(h))) if len(h) else 0
            if len(h) == 0 or h[p] == 0.0:
                raise ValueError(f"{path}: an all-zero impulse response")
            h = (h[p:p + max_taps] / h[p]).astype(np.float32)
            out.write(h.tobytes())
            names.append(os.path.splitext(os.path.basename(path))[0])
            starts.append(pos)
            lengths.append(len(h))
            pos += len(h)
    with open(prefix + ".index.json", "w") as f:
        json.dump({"names": names, "starts": starts, "lengths": lengths, "sample_rate": rate}, f)
    return len(names)


class MixLoader:
    """Batches of noisy mixtures made on the device from a clean shard and a noise shard that live in device memory.

    for mixture, clean, names in MixLoader(clean_prefix, noise_prefix, batch_size=64, device="cuda:0"): ...   # [B,1,L] float32 each
    Per row: a random window of a random clean item (ShardLoader's draw), a random noise item read circularly from a random phase (so
    noise items of any length >= 1 are usable), an SNR uniform in dB over `snr_db` and a level uniform in dB over `level_db` (0 dB
    when None).  The SNR is defined over the window on raw sums (no mean removal): 10 log10(sum c^2 / sum (g n)^2).  A window whose
    clean or noise RMS is below 1e-6 comes out unmixed (g = 0); with probability `p_clean` a row is passed clean on purpose.  With
    peak_limit > 0 a row whose bound a (max|c| + g max|n|) exceeds it is scaled down as a whole - mixture and clean alike, the SNR
    stays.  `clean_prefix` is a mono shard (pack_mono_shard) or a pair shard (pack_shard: its `.clean.f32` is used).  `last_draw`
    keeps the host tables and the device gains of the last batch: {"rows": int64 [B,4], "params": float32 [B,2], "gains": [B,2]}.
    There is no host implementation of the mix: device="cpu" needs an engine (the tests inject the emulator's).  Every rank of a
    data-parallel job passes its own `seed` (e.g. seed + rank).

    Reverberant speech (`rir_prefix`, a pack_rir_shard shard at the same sample rate; without it nothing below applies and the batches
    are what they were).  Per row a response is drawn as well, from the same generator and after the batch's draws above: a seed starts
    with the same rows and params with and without it, and then moves on by two more draws per batch.  With probability `p_reverb` the
    clean window is convolved with the response on the device before the noise
    is added (wunet_reverb_windows; what precedes the window inside its item reverberates into it, what precedes the item does not).
    The mix then runs on the reverberant window r: the SNR is 10 log10(sum r^2 / sum (g n)^2), the peak guard bounds the mixture
    a (r + g n).  The second element of a batch is the target, at the mixture's level a:
      target="dry"          a c, the clean window itself (the response's first tap: h[0] = 1 in a packed shard)
      target="early"        a (h[:E] * c), the direct path and the early reflections, E = round(early_ms sample_rate / 1000) taps
      target="reverberant"  a r: denoising only
    The guard looks at r and the noise; a dry or early target is NOT guarded and can exceed peak_limit where the response attenuates
    (|r| well below |c|).  `last_draw` gains "rir_rows" (int64 [B,4]: window start, item start, RIR start, RIR taps - 0 for a dry row)
    and "reverberant" (a r, [B,1,L]).  Four launches per batch.

    Random spectral shaping (`eq_speech`, `eq_noise`: None, or a dict of filters.random_biquads' keywords sections / spread / p; with
    both None nothing below applies and the batches, the generator's consumption and the launches are what they were).  Per row a
    short cascade of random second-order sections (RNNoise's recipe) is drawn for the speech and another for the noise, from the same
    generator and after all the draws above, the response's included: a seed keeps its rows, params and rir_rows with and without the
    equalisers.  The speech first, then the noise; each by random_biquads' documented order.  Both are filtered on the device
    (wunet_sos_windows) before they are mixed, so the SNR and the peak guard apply to the filtered signals, and the target is the
    filtered speech at the mixture's level: the network is not asked to undo the colouration.
      without a response  the speech window is filtered out of the clean shard, the filter starting at rest `eq_lead` samples in
                          front of the window (fewer where the item starts later; never in front of the item), so a window from the
                          middle of a recording carries no start-up transient; the noise is filtered out of the noise shard along its
                          circular read, with `eq_lead` samples of lead-in too.  The mix then reads the two staged batches.
      with a response     the speech equaliser runs on what the reverb staged - the reverberant window and, for a dry or early target,
                          the direct part, both with the row's one cascade, so the target stays consistent.  These start from rest at
                          the window start: the staged batch has no past, so the lead-in is 0 there, whatever eq_lead is.
    eq_noise needs a noise shard of at least sample_length samples in all.  `last_draw` gains "eq_speech" and "eq_noise": the float32
    [B, S, 6] tables in scipy's layout, or None.  One more launch per filtered batch; still one linear chain."""

    TARGETS = ("dry", "early", "reverberant")

    def __init__(self, clean_prefix, noise_prefix, batch_size, sample_length=16384, snr_db=(0.0, 20.0), level_db=None, peak_limit=0.99,
                 p_clean=0.0, device="cpu", seed=0, steps_per_epoch=None, engine=None, rir_prefix=None, p_reverb=1.0, target="dry",
                 early_ms=50.0, eq_speech=None, eq_noise=None, eq_lead=256):
        self.device = torch.device(device)
        if self.device.type != "cuda" and engine is None:
            raise ValueError("MixLoader mixes on the device: device='cpu' needs an engine (there is no host implementation of the mix)")
        cidx = json.load(open(clean_prefix + ".index.json"))
        nidx = json.load(open(noise_prefix + ".index.json"))
        if cidx["sample_rate"] != nidx["sample_rate"]:
            raise ValueError(f"clean and noise sample rates differ: {cidx['sample_rate']} vs {nidx['sample_rate']}")
        self.sample_rate = cidx["sample_rate"]
        self.names = cidx["names"]
        starts, lengths = np.asarray(cidx["starts"], np.int64), np.asarray(cidx["lengths"], np.int64)
        usable = np.nonzero(lengths >= sample_length)[0]
        if len(usable) == 0:
            raise ValueError("no clean item is at least sample_length long")
        nstarts, nlengths = np.asarray(nidx["starts"], np.int64), np.asarray(nidx["lengths"], np.int64)
        nusable = np.nonzero(nlengths >= 1)[0]
        if len(nusable) == 0:
            raise ValueError("the noise shard has no item of at least one sample")
        clean_file = clean_prefix + ".f32" if os.path.exists(clean_prefix + ".f32") else clean_prefix + ".clean.f32"
        self.clean = self._resident(clean_file, int(starts[-1] + lengths[-1]))          # one upload each; they stay resident
        self.noise = self._resident(noise_prefix + ".f32", int(nstarts[-1] + nlengths[-1]))
        self.usable, self.starts = torch.from_numpy(usable), torch.from_numpy(starts)
        self.spare = torch.from_numpy(lengths - sample_length + 1)                      # number of valid window starts per item
        self.noise_usable, self.noise_starts, self.noise_lengths = torch.from_numpy(nusable), torch.from_numpy(nstarts), torch.from_numpy(nlengths)
        self.batch_size, self.sample_length = batch_size, sample_length
        self.snr_db = (float(snr_db[0]), float(snr_db[1]))
        self.level_db = None if level_db is None else (float(level_db[0]), float(level_db[1]))
        self.peak_limit, self.p_clean = float(peak_limit), float(p_clean)
        self.steps = steps_per_epoch if steps_per_epoch is not None else max(1, len(usable) // batch_size)
        self.gen = torch.Generator().manual_seed(seed)
        self.engine = engine
        self.last_draw = None
        self.rir = None
        if rir_prefix is not None:
            self._init_rir(rir_prefix, p_reverb, target, early_ms)
        self.eq_speech, self.eq_noise, self.eq_lead = self._eq_spec("eq_speech", eq_speech), self._eq_spec("eq_noise", eq_noise), int(eq_lead)
        if self.eq_speech is not None or self.eq_noise is not None:
            from .filters import random_biquads
            for spec in (self.eq_speech, self.eq_noise):
                if spec is not None:
                    random_biquads(1, generator=torch.Generator().manual_seed(0), **spec)      # (its checks, before the first batch)
            if not 0 <= self.eq_lead <= SOS_MAX_LEAD:
                raise ValueError(f"eq_lead must be in [0, {SOS_MAX_LEAD}], got {eq_lead}")
            if self.eq_noise is not None and self.noise.numel() < sample_length:
                raise ValueError("eq_noise needs a noise shard of at least sample_length samples in all")

    UPLOAD_CHUNK = ShardLoader.UPLOAD_CHUNK
    _resident = ShardLoader._resident

    def _init_rir(self, rir_prefix, p_reverb, target, early_ms):
        if target not in self.TARGETS:
            raise ValueError(f"target must be one of {self.TARGETS}, got {target!r}")
        ridx = json.load(open(rir_prefix + ".index.json"))
        if ridx["sample_rate"] != self.sample_rate:
            raise ValueError(f"clean and RIR sample rates differ: {self.sample_rate} vs {ridx['sample_rate']}")
        self.early_taps = int(round(float(early_ms) * self.sample_rate / 1000.0)) if target == "early" else 1
        if self.early_taps < 1:
            raise ValueError(f"early_ms={early_ms} is less than one tap at {self.sample_rate} Hz")
        if not 0.0 <= float(p_reverb) <= 1.0:
            raise ValueError(f"p_reverb must be in [0, 1], got {p_reverb}")
        rstarts, rlengths = np.asarray(ridx["starts"], np.int64), np.asarray(ridx["lengths"], np.int64)
        rusable = np.nonzero(rlengths >= 1)[0]
        if len(rusable) == 0:
            raise ValueError("the RIR shard has no item of at least one sample")
        self.rir = self._resident(rir_prefix + ".f32", int(rstarts[-1] + rlengths[-1]))
        self.rir_usable, self.rir_starts, self.rir_lengths = torch.from_numpy(rusable), torch.from_numpy(rstarts), torch.from_numpy(rlengths)
        self.target, self.p_reverb = target, float(p_reverb)

    def __len__(self):
        return self.steps

    def _uniform_int(self, count):
        """One integer per row, uniform over [0, count[b]) (count int64 [B], >= 1) - ShardLoader.draw's rule."""
        v = (torch.rand(self.batch_size, generator=self.gen, dtype=torch.float64) * count.double()).long()
        return torch.minimum(v, count - 1)

    def draw(self):
        """(clean item ids, rows int64 [B,4], params float32 [B,2]) of one batch - the host's whole share of it.  rows[b] = clean
        window start, noise item start, noise item length (0: the row is passed clean), noise phase; params[b] = snr_db, linear level."""
        B, gen = self.batch_size, self.gen
        pick = self.usable[torch.randint(len(self.usable), (B,), generator=gen)]
        first = self.starts[pick] + self._uniform_int(self.spare[pick])
        npick = self.noise_usable[torch.randint(len(self.noise_usable), (B,), generator=gen)]
        nlen = self.noise_lengths[npick]
        phase = self._uniform_int(nlen)
        u = torch.rand(3, B, generator=gen, dtype=torch.float64)
        snr = self.snr_db[0] + (self.snr_db[1] - self.snr_db[0]) * u[0]
        level_db = torch.zeros(B, dtype=torch.float64) if self.level_db is None else self.level_db[0] + (self.level_db[1] - self.level_db[0]) * u[1]
        nlen = torch.where(u[2] < self.p_clean, torch.zeros_like(nlen), nlen)
        rows = torch.stack([first, self.noise_starts[npick], nlen, phase], dim=1).contiguous()
        params = torch.stack([snr, 10.0 ** (level_db / 20.0)], dim=1).float().contiguous()
        return pick, rows, params

    def mix(self, rows, params):
        """The batch that the two host tables describe: mixture, clean [B, 1, L] and gains [B, 2] on the device.  One non-blocking copy
        per table, then the two launches of wunet_mix_windows (csrc/wunet_mix.h)."""
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        B, L, dev = rows.shape[0], self.sample_length, self.device
        mixture = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
        clean = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
        gains = torch.empty(B, 2, dtype=torch.float32, device=dev)
        self.engine.mix_windows(self.clean, self.noise, rows.to(dev, non_blocking=True), params.to(dev, non_blocking=True), mixture, clean,
                                gains, peak_limit=self.peak_limit)
        return mixture, clean, gains

    def draw_rir(self, pick, rows):
        """rir_rows int64 [B,4] of the batch that draw() just drew: window start, clean item start, RIR start, RIR taps (0: the row stays
        dry).  Its two draws come after all of draw()'s."""
        B, gen = self.batch_size, self.gen
        rpick = self.rir_usable[torch.randint(len(self.rir_usable), (B,), generator=gen)]
        taps = self.rir_lengths[rpick]
        u = torch.rand(B, generator=gen, dtype=torch.float64)
        taps = torch.where(u < self.p_reverb, taps, torch.zeros_like(taps))
        return torch.stack([rows[:, 0], self.starts[pick], self.rir_starts[rpick], taps], dim=1).contiguous()

    def mix_reverberant(self, rows, params, rir_rows):
        """The batch that the three host tables describe: (mixture, target, gains, a r).  One linear chain of four launches: the reverb
        into a staged batch (and, for a dry / early target, the staged direct part), the mix's two with the staged batch as their clean
        array, and the target's level."""
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        B, L, dev = rows.shape[0], self.sample_length, self.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)          # noqa: E731
        staged, mixture, reverberant, gains = new(B, 1, L), new(B, 1, L), new(B, 1, L), new(B, 2)
        direct = None if self.target == "reverberant" else new(B, 1, L)
        self.engine.reverb_windows(self.clean, self.rir, rir_rows.to(dev, non_blocking=True), staged, direct, early_taps=self.early_taps)
        staged_rows = rows.clone()
        staged_rows[:, 0] = torch.arange(B, dtype=torch.int64) * L
        self.engine.mix_windows(staged.view(-1), self.noise, staged_rows.to(dev, non_blocking=True), params.to(dev, non_blocking=True), mixture,
                                reverberant, gains, peak_limit=self.peak_limit)
        target = reverberant if direct is None else self.engine.apply_level(direct, gains)
        return mixture, target, gains, reverberant

    @staticmethod
    def _eq_spec(name, spec):
        if spec is None:
            return None
        spec = dict(spec)
        if set(spec) - {"sections", "spread", "p"}:
            raise ValueError(f"{name}: a dict of random_biquads' keywords sections, spread, p expected, got {sorted(spec)}")
        return spec

    def draw_eq(self):
        """(eq_speech, eq_noise) of the batch just drawn: float32 [B, S, 6] each, or None.  Their draws come after all the others of
        the batch, the speech's first."""
        from .filters import random_biquads
        return tuple(None if spec is None else random_biquads(self.batch_size, generator=self.gen, **spec) for spec in (self.eq_speech, self.eq_noise))

    def _filtered(self, flat, table, coefs, lead):
        """A staged [B, 1, L] batch: the windows of `flat` that the table [B, 4] names, through the cascades coefs [B, S, 5]."""
        dev = self.device
        out = torch.empty(table.shape[0], 1, self.sample_length, dtype=torch.float32, device=dev)
        return self.engine.sos_windows(flat, table.to(dev, non_blocking=True), coefs.to(dev, non_blocking=True), out, lead=lead)

    def eq_tables(self, speech_table, rows, eq_speech, eq_noise):
        """The host tables of an equalised batch, a dict: "speech" / "noise" = (rows [B, 4], coefs [B, S, 5]) of the filter launch, or
        None without that equaliser, and "rows" = the mix's table on what the filters staged.  speech_table: the speech filter's rows.
        A filtered batch is read by the mix as windows of one flat array: row b's clean window starts at b L, its noise is the item
        [b L, (b + 1) L) read from phase 0.  A row that is passed clean (noise length 0) keeps its 0 in the mix's table; its staged noise
        is filtered from one sample and never read."""
        from .filters import sos_to_coefs
        B, L = rows.shape[0], self.sample_length
        at = torch.arange(B, dtype=torch.int64) * L
        t = {"speech": None, "noise": None}
        rows = rows.clone()
        if eq_speech is not None:
            t["speech"] = (speech_table.contiguous(), sos_to_coefs(eq_speech))
            rows[:, 0] = at
        if eq_noise is not None:
            table = rows.clone()
            table[:, 2] = torch.clamp(rows[:, 2], min=1)
            t["noise"] = (table, sos_to_coefs(eq_noise))
            rows[:, 1] = at
            rows[:, 2] = torch.where(rows[:, 2] > 0, torch.full_like(at, L), torch.zeros_like(at))
            rows[:, 3] = 0
        t["rows"] = rows
        return t

    def enqueue_equalised(self, clean_src, tables, params, lead):
        """The launches of an equalised batch on tables that eq_tables made (host or device tensors): a filter launch per equaliser into
        a staged batch, then the mix's two on the staged arrays - one linear chain.  clean_src: the flat array the speech is read from.
        Returns (mixture, clean, gains)."""
        B, L, dev = tables["rows"].shape[0], self.sample_length, self.device
        if tables["speech"] is not None:
            clean_src = self._filtered(clean_src, *tables["speech"], lead).view(-1)
        noise_src = self.noise if tables["noise"] is None else self._filtered(self.noise, *tables["noise"], self.eq_lead).view(-1)
        mixture = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
        clean = torch.empty(B, 1, L, dtype=torch.float32, device=dev)
        gains = torch.empty(B, 2, dtype=torch.float32, device=dev)
        self.engine.mix_windows(clean_src, noise_src, tables["rows"].to(dev, non_blocking=True), params.to(dev, non_blocking=True), mixture, clean,
                                gains, peak_limit=self.peak_limit)
        return mixture, clean, gains

    def mix_equalised(self, pick, rows, params, eq_speech, eq_noise):
        """mix() with the equalisers: (mixture, target, gains)."""
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        zero = torch.zeros(rows.shape[0], dtype=torch.int64)
        speech_table = torch.stack([rows[:, 0], self.starts[pick], zero, zero], dim=1)
        return self.enqueue_equalised(self.clean, self.eq_tables(speech_table, rows, eq_speech, eq_noise), params, self.eq_lead)

    def mix_reverberant_equalised(self, rows, params, rir_rows, eq_speech, eq_noise):
        """mix_reverberant() with the equalisers: (mixture, target, gains, a r) with r the filtered reverberant window.  The speech
        equaliser runs on the staged reverberant batch and on the staged direct part, from rest at the window start (lead 0)."""
        if self.engine is None:
            from .engine import default_engine
            self.engine = default_engine()
        B, L, dev = rows.shape[0], self.sample_length, self.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)          # noqa: E731
        staged = new(B, 1, L)
        direct = None if self.target == "reverberant" else new(B, 1, L)
        self.engine.reverb_windows(self.clean, self.rir, rir_rows.to(dev, non_blocking=True), staged, direct, early_taps=self.early_taps)
        at = torch.arange(B, dtype=torch.int64) * L
        speech_table = torch.stack([at, at, torch.zeros_like(at), torch.zeros_like(at)], dim=1)
        staged_rows = rows.clone()
        staged_rows[:, 0] = at
        tables = self.eq_tables(speech_table, staged_rows, eq_speech, eq_noise)
        if direct is not None and eq_speech is not None:
            direct = self._filtered(direct.view(-1), *tables["speech"], 0)
        mixture, reverberant, gains = self.enqueue_equalised(staged.view(-1), tables, params, 0)
        target = reverberant if direct is None else self.engine.apply_level(direct, gains)
        return mixture, target, gains, reverberant

    def __iter__(self):
        equalised = self.eq_speech is not None or self.eq_noise is not None
        for _ in range(self.steps):
            pick, rows, params = self.draw()
            if self.rir is None:
                if equalised:
                    eq_s, eq_n = self.draw_eq()
                    mixture, clean, gains = self.mix_equalised(pick, rows, params, eq_s, eq_n)
                    self.last_draw = {"rows": rows, "params": params, "gains": gains, "eq_speech": eq_s, "eq_noise": eq_n}
                else:
                    mixture, clean, gains = self.mix(rows, params)
                    self.last_draw = {"rows": rows, "params": params, "gains": gains}
            else:
                rir_rows = self.draw_rir(pick, rows)
                if equalised:
                    eq_s, eq_n = self.draw_eq()
                    mixture, clean, gains, reverberant = self.mix_reverberant_equalised(rows, params, rir_rows, eq_s, eq_n)
                else:
                    eq_s = eq_n = None
                    mixture, clean, gains, reverberant = self.mix_reverberant(rows, params, rir_rows)
                self.last_draw = {"rows": rows, "params": params, "gains": gains, "rir_rows": rir_rows, "reverberant": reverberant}
                if equalised:
                    self.last_draw.update(eq_speech=eq_s, eq_noise=eq_n)
            yield mixture, clean, [self.names[i] for i in pick.tolist()]
