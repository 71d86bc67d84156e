"""GPU box: what reverberant batches cost.  In one process, HIP-event times, median of >= 20 samples after warm-up, at 64 x 16384 - the
product's training batch - for responses of 2048 / 8192 / 16384 taps (every row reverberant, the worst case of the loader):
  (a) Engine.reverb_windows alone on a table that is already on the device, reverberant only and with the `direct` output of an early
      target (50 ms = 800 taps); a sample is 10 back-to-back calls.  The FLOP count is the algorithm's, 2 B L K (the GEMM form's extra
      240 k' per tile and the second accumulator set are not counted), over the median: achieved TFLOP/s and the share of the
      157.3 TFLOP/s fp32 matrix peak.  Per-kernel time from the library's profiler beside it.
  (b) one MixLoader batch with rir_prefix (draws, three table copies, four launches; target "early") and one without (two launches)
      - profiles/mix_bench.txt is the earlier record of the latter
  (c) the same convolution through torch.fft on the device (gather of the windows with their history, rfft of both, product, irfft),
      as a user would write it, on the same table; its largest difference from the kernel is printed
There is no pass / fail time: the file records the measurement, whichever route is faster.
    python tools/reverb_bench.py [--out profiles/reverb_bench.txt] [--reps 30] [--commit <hash>]"""
import argparse
import ctypes
import importlib
import json
import os
import socket
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "wave-u-net-for-speech-enhancement_amd"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reverb_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
wd = importlib.import_module(PKG + ".waveform_dataset")
engine = importlib.import_module(PKG + ".engine").default_engine()
dev = torch.device("cuda:0")
B, L, PEAK, EARLY_MS, INNER = 64, 16384, 0.99, 50.0, 10
PEAK_TF = 157.3
TAPS = (2048, 8192, 16384)


def write_shard(prefix, items):
    """A synthetic mono shard written directly (no decoding): the flat float32 file + pack_mono_shard's index."""
    lengths = [len(x) for x in items]
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    np.concatenate(items).astype(np.float32).tofile(prefix + ".f32")
    with open(prefix + ".index.json", "w") as f:
        json.dump({"names": [f"item{i}" for i in range(len(items))], "starts": [int(v) for v in starts], "lengths": lengths, "sample_rate": 16000}, f)


def timed(call, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner        # ms per call


def measure(call, inner=1):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = [timed(call, inner) for _ in range(args.reps)]
    return statistics.median(t), min(t), max(t)


def fft_reverb(clean_flat, rir_flat, rir_rows, K):
    """The convolution as a user writes it with torch.fft (the zero-fill in front of an item and the clamps left out: every window of
    the bench has its K - 1 samples of history inside the array)."""
    n = 1 << (L + 2 * K - 2).bit_length()
    x = clean_flat[rir_rows[:, 0:1] - (K - 1) + torch.arange(L + K - 1, device=dev)]
    h = rir_flat[rir_rows[:, 2:3] + torch.arange(K, device=dev)]
    y = torch.fft.irfft(torch.fft.rfft(x, n) * torch.fft.rfft(h, n), n)
    return y[:, K - 1:K - 1 + L]


rng = np.random.default_rng(0)
fmt = lambda t: f"{t[0]:.4f} [min {t[1]:.4f}, max {t[2]:.4f}]"          # noqa: E731
lines = [f"Reverberant batches at {B} x {L} on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}, commit {args.commit}, torch {torch.__version__}), "
         f"median of {args.reps} samples after 3 warm-up calls, HIP events, ms per call; fp32 matrix peak {PEAK_TF} TFLOP/s"]
with tempfile.TemporaryDirectory() as tmp:
    cp, npfx = os.path.join(tmp, "clean"), os.path.join(tmp, "noise")
    write_shard(cp, [rng.standard_normal(int(n)) * 0.1 for n in rng.integers(2 * L, 6 * L, 256)])
    write_shard(npfx, [rng.standard_normal(int(n)) * 0.05 for n in rng.integers(L // 4, 8 * L, 64)])
    kw = dict(batch_size=B, sample_length=L, snr_db=(0.0, 20.0), level_db=(-10.0, 3.0), peak_limit=PEAK, device=dev, seed=0)
    plain = wd.MixLoader(cp, npfx, **kw)

    def plain_batch():
        _, rows, params = plain.draw()
        return plain.mix(rows, params)

    t_plain = measure(plain_batch)
    lines.append(f"  MixLoader batch without rir_prefix (draw + 2 table copies + 2 launches):                {fmt(t_plain)}")
    for K in TAPS:
        rp = os.path.join(tmp, f"rir{K}")
        write_shard(rp, [np.concatenate([[1.0], rng.standard_normal(K - 1) * 0.3 * np.exp(-np.arange(1, K) / (K / 6.0))]) for _ in range(16)])
        loader = wd.MixLoader(cp, npfx, rir_prefix=rp, p_reverb=1.0, target="early", early_ms=EARLY_MS, **kw)
        E = loader.early_taps

        def loader_batch():
            pick, rows, params = loader.draw()
            return loader.mix_reverberant(rows, params, loader.draw_rir(pick, rows))

        # a table whose windows all have K - 1 samples of history inside the array (what the torch.fft route assumes)
        pick, rows_h, _ = loader.draw()
        rir_rows_h = loader.draw_rir(pick, rows_h)
        rir_rows_h[:, 0] = torch.clamp(rir_rows_h[:, 0], min=K - 1)
        rir_rows_h[:, 1] = 0                                  # (and no zero-fill in front of an item)
        rir_rows = rir_rows_h.to(dev)
        rev, direct = torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev)
        alone = lambda: engine.reverb_windows(loader.clean, loader.rir, rir_rows, rev, None)                          # noqa: E731
        both = lambda: engine.reverb_windows(loader.clean, loader.rir, rir_rows, rev, direct, early_taps=E)           # noqa: E731
        fft = lambda: fft_reverb(loader.clean, loader.rir, rir_rows, K)                                               # noqa: E731
        t_alone, t_both, t_fft, t_loader = measure(alone, INNER), measure(both, INNER), measure(fft, INNER), measure(loader_batch)
        alone()
        diff = float((fft() - rev[:, 0]).abs().max())
        scale = float(rev.abs().max())
        engine.lib.wunet_profile_enable(1)
        for _ in range(5):
            alone()
        buf = ctypes.create_string_buffer(1 << 16)
        n_prof = engine.lib.wunet_profile_collect(buf, len(buf))
        engine.lib.wunet_profile_enable(0)
        flop = 2.0 * B * L * K
        tf = flop / (t_alone[0] * 1e-3) / 1e12
        lines += [f"  {K} taps ({flop / 1e9:.2f} GFLOP per batch)",
                  f"    (a) Engine.reverb_windows alone, reverberant only:                                   {fmt(t_alone)}  -> {tf:.2f} TFLOP/s, "
                  f"{100.0 * tf / PEAK_TF:.1f} % of the fp32 matrix peak (compute-bound: {flop / PEAK_TF / 1e9:.4f} ms at peak)",
                  f"        with `direct` over {E} taps:                                                       {fmt(t_both)}",
                  f"    (b) MixLoader batch with rir_prefix, target early (draws + 3 table copies + 4 launches): {fmt(t_loader)}  "
                  f"({t_loader[0] - t_plain[0]:+.4f} ms over the batch without)",
                  f"    (c) the same convolution through torch.fft (gather, 2 rfft, product, irfft):           {fmt(t_fft)}  -> (c) / (a) = {t_fft[0] / t_alone[0]:.2f} x"
                  f" ({'the kernel is SLOWER than the torch.fft route' if t_alone[0] > t_fft[0] else 'the kernel is faster'});  "
                  f"max |fft - kernel| {diff:.2e} at max |out| {scale:.2e}"]
        if n_prof > 0:
            for ln in buf.value.decode().strip().split("\n"):
                if "reverb" in ln:
                    lines.append("        profiler, 5 calls (name, launches, total ms, counted flops, counted bytes): " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
