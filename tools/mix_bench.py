"""GPU box: what a MixLoader batch costs.  In one process, HIP-event times, median of >= 20 after warm-up (eager calls, host time of the
draw, the two table copies and the launches included), at 64 x 16384 - the product's training batch:
  (a) one MixLoader batch (draw, two table copies, mix_partial_kernel + mix_apply_kernel)
  (b) one ShardLoader batch (draw, one copy, crop_windows_kernel) - the pre-mixed path a step is fed by today
  (c) the same mix written in eager torch on the same device tables - what a user would write without the kernels
  (d) Engine.mix_windows alone on tables that are already on the device: the pair of launches, with the bytes they move
      (reads 2 B L floats per launch, writes 2 B L: 24 B L bytes) and the bandwidth that is; per-kernel times from the library's profiler
The difference (a) - (b) is what on-the-fly mixing adds to a training step; it is printed beside the README's step time.  There is
no pass / fail time: the file records the measurement.
    python tools/mix_bench.py [--out profiles/mix_bench.txt] [--reps 30] [--commit <hash>]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mix_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--commit", default="unknown")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
wd = importlib.import_module(PKG + ".waveform_dataset")
engine = importlib.import_module(PKG + ".engine").default_engine()
dev = torch.device("cuda:0")
B, L, PEAK = 64, 16384, 0.99
README_STEP_MS = "4.78 - 5.07"


def write_shard(prefix, lengths, rng, scale, suffixes):
    """A synthetic shard written directly (no decoding): flat float32 file(s) + the index of pack_shard / pack_mono_shard."""
    starts = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    x = (rng.standard_normal(int(np.sum(lengths))) * scale).astype(np.float32)
    for s in suffixes:
        x.tofile(prefix + s)
    with open(prefix + ".index.json", "w") as f:
        json.dump({"names": [f"item{i}" for i in range(len(lengths))], "starts": [int(v) for v in starts], "lengths": [int(v) for v in lengths],
                   "sample_rate": 16000}, f)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                # ms


def measure(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    t = [timed(call) for _ in range(args.reps)]
    return statistics.median(t), min(t), max(t)


def eager_mix(clean_flat, noise_flat, rows, params):
    """The mix as a user writes it in torch today (float32 sums; the clamps of corrupt tables left out)."""
    j = torch.arange(L, device=rows.device)
    nl = rows[:, 2:3]
    c = clean_flat[rows[:, 0:1] + j]
    n = noise_flat[rows[:, 1:2] + (rows[:, 3:4] + j) % nl.clamp(min=1)]
    pc, pn = c.square().sum(1), n.square().sum(1)
    g = torch.sqrt(pc / (pn * 10.0 ** (params[:, 0] / 10.0)))
    g = torch.where((pc < L * 1e-12) | (pn < L * 1e-12) | (nl[:, 0] < 1), torch.zeros_like(g), g)
    a = params[:, 1]
    bound = a * (c.abs().amax(1) + g * n.abs().amax(1))
    a = torch.where(bound > PEAK, a * PEAK / bound, a)
    return a[:, None] * (c + g[:, None] * n), a[:, None] * c


rng = np.random.default_rng(0)
with tempfile.TemporaryDirectory() as tmp:
    cp, npfx, pp = os.path.join(tmp, "clean"), os.path.join(tmp, "noise"), os.path.join(tmp, "pair")
    clean_lengths = rng.integers(2 * L, 6 * L, 256)
    write_shard(cp, clean_lengths, rng, 0.1, [".f32"])
    write_shard(npfx, rng.integers(L // 4, 8 * L, 64), rng, 0.05, [".f32"])
    write_shard(pp, clean_lengths, rng, 0.1, [".noisy.f32", ".clean.f32"])
    mixer = wd.MixLoader(cp, npfx, batch_size=B, sample_length=L, snr_db=(0.0, 20.0), level_db=(-10.0, 3.0), peak_limit=PEAK, device=dev, seed=0)
    shard = wd.ShardLoader(pp, batch_size=B, sample_length=L, device=dev, seed=0)

    def mix_batch():
        _, rows, params = mixer.draw()
        return mixer.mix(rows, params)

    def shard_batch():
        _, first = shard.draw()
        return shard.crop(first)

    _, rows_h, params_h = mixer.draw()
    rows, params = rows_h.to(dev), params_h.to(dev)
    outs = [torch.empty(B, 1, L, device=dev), torch.empty(B, 1, L, device=dev), torch.empty(B, 2, device=dev)]
    kernel_pair = lambda: engine.mix_windows(mixer.clean, mixer.noise, rows, params, *outs, peak_limit=PEAK)       # noqa: E731
    eager = lambda: eager_mix(mixer.clean, mixer.noise, rows, params)                                              # noqa: E731
    t_mix, t_shard, t_eager, t_pair = measure(mix_batch), measure(shard_batch), measure(eager), measure(kernel_pair)
    kernel_pair()
    em, ec = eager()
    torch.cuda.synchronize()
    d_mix, d_clean = float((em - outs[0][:, 0]).abs().max()), float((ec - outs[1][:, 0]).abs().max())
    engine.lib.wunet_profile_enable(1)
    for _ in range(5):
        kernel_pair()
    buf = ctypes.create_string_buffer(1 << 16)
    n_prof = engine.lib.wunet_profile_collect(buf, len(buf))
    engine.lib.wunet_profile_enable(0)

moved = 24.0 * B * L
fmt = lambda t: f"{t[0]:.4f} [min {t[1]:.4f}, max {t[2]:.4f}]"          # noqa: E731
lines = [f"MixLoader at {B} x {L} on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}, commit {args.commit}, torch {torch.__version__}), "
         f"median of {args.reps} eager calls after 3 warm-up calls, HIP events, ms per batch",
         f"  (a) MixLoader batch (draw + 2 table copies + 2 launches):        {fmt(t_mix)}",
         f"  (b) ShardLoader batch (draw + 1 copy + crop_windows_kernel):      {fmt(t_shard)}",
         f"  (c) the same mix in eager torch, tables already on the device:    {fmt(t_eager)}",
         f"  (d) Engine.mix_windows alone, tables already on the device:       {fmt(t_pair)}",
         f"      bytes moved by the pair of launches: {moved / 1e6:.2f} MB (partial pass reads 2 B L floats; mix pass reads 2 B L, writes 2 B L) "
         f"-> {moved / (t_pair[0] * 1e-3) / 1e12:.3f} TB/s over the median of (d), launch gaps and host time included",
         f"  kernel path vs eager torch, same tables: (c) / (d) = {t_eager[0] / t_pair[0]:.2f} x;  max |eager - kernel| mixture {d_mix:.2e}, clean {d_clean:.2e} "
         f"(the eager sums are float32)",
         f"  added per training step over a ShardLoader-fed step: (a) - (b) = {t_mix[0] - t_shard[0]:+.4f} ms, beside the README's {README_STEP_MS} ms per step"]
if n_prof > 0:
    lines.append("  per-kernel time from the library's profiler, 5 calls of (d) (name, launches, total ms, algorithmic flops, algorithmic bytes):")
    for ln in buf.value.decode().strip().split("\n"):
        lines.append("      " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
