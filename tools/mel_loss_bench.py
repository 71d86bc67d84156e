"""GPU box: what the mel loss costs beside the multi-resolution STFT loss at the same resolutions, which runs the same DFT and adjoint
GEMMs: the difference is the price of the two projection GEMMs and of the S / dS planes going once through memory.  In one process at
64 x 16384, forward + backward as eager calls (host launch time included), HIP-event times, median / minimum / maximum of >= 20 after
warm-up, the two cases alternating:
  mel_loss at its defaults (512 / 128 / 512 with 40 mels, 1024 / 256 / 1024 with 80, 2048 / 512 / 2048 with 128),
  stft_loss at the same three (n_fft, hop, window).
Also printed: the per-kernel times of both from the library's profiler (a pass of its own, after the timing), and for the three new
kernels their time beside the bytes M (3 BP + 2 MP) 4 and the flops 2 2 M bins n_mels of a direction.
    python tools/mel_loss_bench.py [--out profiles/mel_loss_bench.txt] [--reps 30]"""
import argparse
import ctypes
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "wave-u-net-for-speech-enhancement_amd"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mel_loss_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
loss_mod = importlib.import_module(PKG + ".loss")
dev = torch.device("cuda:0")
B, T = 64, 16384
g = torch.Generator().manual_seed(1)
t = torch.arange(T, dtype=torch.float64)
clean = 0.1 * torch.randn(B, 1, T, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2.0 * torch.pi * 0.013 * t)
enh = (clean + 0.05 * torch.randn(B, 1, T, generator=g, dtype=torch.float64)).float().to(dev)
clean = clean.float().to(dev)
mel = loss_mod.mel_loss()
RES = mel.resolutions


def fwd_bwd(crit):
    def call():
        x = enh.detach().requires_grad_(True)
        loss = crit(clean, x)
        loss.backward()
        return loss.detach(), x.grad
    return call


cases = {"mel": fwd_bwd(mel),
         "stft": fwd_bwd(loss_mod.stft_loss(fft_sizes=[r[0] for r in RES], hop_sizes=[r[1] for r in RES], win_lengths=[r[2] for r in RES]))}


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                # ms


out = {}
for k, fn in cases.items():
    for _ in range(3):
        out[k] = fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(args.reps):
    for k, fn in cases.items():               # alternating: both see the same box at the same time
        times[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in times.items()}
lines = [f"mel loss beside the STFT loss at the same resolutions, forward + backward at {B} x {T}, {torch.cuda.get_device_name(0)}, "
         f"{args.reps} calls each, ms per call (eager, host launches included)",
         f"  resolutions {RES}  n_mels {mel.n_mels}"]
for k, name in (("mel", "mel_loss "), ("stft", "stft_loss")):
    lines.append(f"    {name} median {med[k]:.3f}  min {min(times[k]):.3f}  max {max(times[k]):.3f}   loss {float(out[k][0]):.7f}")
lines.append(f"    difference of the medians {med['mel'] - med['stft']:.3f} ms, ratio {med['mel'] / med['stft']:.3f}")
engine = importlib.import_module(PKG + ".engine").default_engine()
CALLS = 5
prof = {}
for k, name in (("mel", "mel_loss"), ("stft", "stft_loss")):
    engine.lib.wunet_profile_enable(1)
    for _ in range(CALLS):
        cases[k]()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    n = engine.lib.wunet_profile_collect(buf, len(buf))
    engine.lib.wunet_profile_enable(0)
    if n > 0:
        lines.append(f"  per-kernel time of {name} from the library's profiler, {CALLS} calls (name, launches, ms, flops, bytes):")
        for ln in buf.value.decode().strip().split("\n"):
            lines.append("    " + ln.replace("\t", "  "))
            f = ln.split("\t")
            if k == "mel" and len(f) >= 5:
                prof[f[0]] = (float(f[2]), float(f[3]), float(f[4]))
# the new kernels beside their bytes and flops as the profiler's records count them (per direction about M (3 BP + 2 MP) 4 bytes and
# 2 2 M bins n_mels flops, summed over the three resolutions and the CALLS calls)
new = [k for k in prof if k.startswith("mel_proj") or k.startswith("mel_spec")]
if new:
    lines.append("  the kernels with the new work (mel_spec also holds the DFT GEMM): GB/s and GFLOP/s of the records above")
    for k in new:
        ms, fl, by = prof[k]
        lines.append(f"    {k}  {by / ms * 1e-6:.0f} GB/s  {fl / ms * 1e-6:.0f} GFLOP/s")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
