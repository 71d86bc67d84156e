"""GPU box: what the multi-resolution STFT loss costs, ours against torch.stft under autograd on the same GPU.  In one process at
64 x 16384 with the default three resolutions (n_fft 1024 / 2048 / 512, hop 120 / 240 / 50, window 600 / 1200 / 240), forward +
backward, HIP-event times, median of >= 20 after warm-up, alternating:
  (a) ours  loss.stft_loss: wunet_stft_forward x 3, wunet_stft_finalize, wunet_stft_backward x 3
  (b) torch the same loss written with torch.stft (hipFFT) and elementwise ops, backward by autograd
both as eager calls (host launch time included).  Also printed: how far the two losses and gradients are apart, the peak memory of
each, and the per-kernel times of (a) from the library's profiler.
    python tools/stft_loss_bench.py [--out profiles/stft_loss_bench.txt] [--reps 30]"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "wave-u-net-for-speech-enhancement_amd"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stft_loss_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
loss_mod = importlib.import_module(PKG + ".loss")
dev = torch.device("cuda:0")
B, T = 64, 16384
RES = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
CLAMP = 1e-7
g = torch.Generator().manual_seed(1)
t = torch.arange(T, dtype=torch.float64)
clean = 0.1 * torch.randn(B, 1, T, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2.0 * torch.pi * 0.013 * t)
enh = (clean + 0.05 * torch.randn(B, 1, T, generator=g, dtype=torch.float64)).float().to(dev)
clean = clean.float().to(dev)
crit = loss_mod.stft_loss()
windows = {W: torch.hann_window(W, periodic=True, device=dev) for _, _, W in RES}


def ours():
    x = enh.detach().requires_grad_(True)
    loss = crit(clean, x)
    loss.backward()
    return loss.detach(), x.grad


def mag(x, N, H, W):
    X = torch.stft(x.reshape(-1, T), N, hop_length=H, win_length=W, window=windows[W], center=True, pad_mode="reflect", return_complex=True)
    return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=CLAMP))


def torch_way():
    x = enh.detach().requires_grad_(True)
    total = 0.0
    for N, H, W in RES:
        sc, se = mag(clean, N, H, W), mag(x, N, H, W)
        total = total + torch.sqrt(((sc - se) ** 2).sum()) / torch.sqrt((sc ** 2).sum()) + (torch.log(sc) - torch.log(se)).abs().mean()
    loss = total / len(RES)
    loss.backward()
    return loss.detach(), x.grad


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                # ms


def peak(call):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    call()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20


cases = {"ours": ours, "torch": torch_way}
out = {}
for k, fn in cases.items():
    for _ in range(3):
        out[k] = fn()
torch.cuda.synchronize()
times = {k: [] for k in cases}
for _ in range(args.reps):
    for k, fn in cases.items():               # alternating: both see the same box at the same time
        times[k].append(timed(fn))
mem = {k: peak(fn) for k, fn in cases.items()}
a, b = statistics.median(times["ours"]), statistics.median(times["torch"])
dl = abs(float(out["ours"][0]) - float(out["torch"][0])) / abs(float(out["torch"][0]))
dg = ((out["ours"][1] - out["torch"][1]).abs().max() / out["torch"][1].abs().max()).item()
lines = [f"multi-resolution STFT loss forward + backward at {B} x {T}, resolutions {RES}, {torch.cuda.get_device_name(0)}, "
         f"median of {args.reps}, ms per call (eager, host launches included)",
         f"  (a) ours {a:.3f}  (b) torch.stft under autograd {b:.3f}  ratio a / b {a / b:.3f}   "
         f"[min {min(times['ours']):.3f} / {min(times['torch']):.3f}, max {max(times['ours']):.3f} / {max(times['torch']):.3f}]",
         f"  peak device memory of one call beyond the inputs: ours {mem['ours']:.0f} MiB, torch {mem['torch']:.0f} MiB",
         f"  ours against torch (both float32): loss {float(out['ours'][0]):.7f} vs {float(out['torch'][0]):.7f} ({dl:.2e} relative), "
         f"gradient {dg:.2e} of its largest element"]
engine = importlib.import_module(PKG + ".engine").default_engine()
engine.lib.wunet_profile_enable(1)
for _ in range(5):
    ours()
import ctypes  # noqa: E402
buf = ctypes.create_string_buffer(1 << 16)
n = engine.lib.wunet_profile_collect(buf, len(buf))
engine.lib.wunet_profile_enable(0)
if n > 0:
    lines.append("  per-kernel time of (a) from the library's profiler, 5 calls:")
    for ln in buf.value.decode().strip().split("\n"):
        lines.append("    " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
