"""GPU box: what the compressed spectral loss costs beside the multi-resolution STFT loss, which runs the same two GEMMs with a cheaper
epilogue and two saved planes fewer.  In one process at 64 x 16384, forward + backward as eager calls (host launch time included),
HIP-event times, median of >= 20 after warm-up, the four cases alternating:
  compressed_spectral_loss and stft_loss at the default resolution of the former (n_fft 512, hop 128, window 512),
  compressed_spectral_loss and stft_loss at the three default resolutions of the latter (1024 / 120 / 600, 2048 / 240 / 1200, 512 / 50 / 240).
Also printed: the per-kernel times of the two compressed-loss cases from the library's profiler (a pass of its own, after the timing).
    python tools/cspec_loss_bench.py [--out profiles/cspec_loss_bench.txt] [--reps 30]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cspec_loss_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
loss_mod = importlib.import_module(PKG + ".loss")
dev = torch.device("cuda:0")
B, T = 64, 16384
ONE = ((512, 128, 512),)
THREE = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
g = torch.Generator().manual_seed(1)
t = torch.arange(T, dtype=torch.float64)
clean = 0.1 * torch.randn(B, 1, T, generator=g, dtype=torch.float64) + 0.3 * torch.sin(2.0 * torch.pi * 0.013 * t)
enh = (clean + 0.05 * torch.randn(B, 1, T, generator=g, dtype=torch.float64)).float().to(dev)
clean = clean.float().to(dev)


def res_args(res):
    return {"fft_sizes": [r[0] for r in res], "hop_sizes": [r[1] for r in res], "win_lengths": [r[2] for r in res]}


def fwd_bwd(crit):
    def call():
        x = enh.detach().requires_grad_(True)
        loss = crit(clean, x)
        loss.backward()
        return loss.detach(), x.grad
    return call


cases = {"cspec 1 res": fwd_bwd(loss_mod.compressed_spectral_loss(**res_args(ONE))),
         "stft 1 res": fwd_bwd(loss_mod.stft_loss(**res_args(ONE))),
         "cspec 3 res": fwd_bwd(loss_mod.compressed_spectral_loss(**res_args(THREE))),
         "stft 3 res": fwd_bwd(loss_mod.stft_loss(**res_args(THREE)))}


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
    for k, fn in cases.items():               # alternating: all four see the same box at the same time
        times[k].append(timed(fn))
med = {k: statistics.median(v) for k, v in times.items()}
lines = [f"compressed spectral loss beside the STFT loss, forward + backward at {B} x {T}, {torch.cuda.get_device_name(0)}, "
         f"median of {args.reps}, ms per call (eager, host launches included)"]
for tag, res in (("1 res", ONE), ("3 res", THREE)):
    a, b = med["cspec " + tag], med["stft " + tag]
    ta, tb = times["cspec " + tag], times["stft " + tag]
    lines.append(f"  resolutions {res}")
    lines.append(f"    compressed_spectral_loss {a:.3f}  stft_loss {b:.3f}  ratio {a / b:.3f}   "
                 f"[min {min(ta):.3f} / {min(tb):.3f}, max {max(ta):.3f} / {max(tb):.3f}]   losses {float(out['cspec ' + tag][0]):.7f} / "
                 f"{float(out['stft ' + tag][0]):.7f}")
engine = importlib.import_module(PKG + ".engine").default_engine()
for tag in ("1 res", "3 res"):
    engine.lib.wunet_profile_enable(1)
    for _ in range(5):
        cases["cspec " + tag]()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    n = engine.lib.wunet_profile_collect(buf, len(buf))
    engine.lib.wunet_profile_enable(0)
    if n > 0:
        lines.append(f"  per-kernel time of compressed_spectral_loss, {tag}, from the library's profiler, 5 calls "
                     "(name, launches, ms, flops, bytes):")
        for ln in buf.value.decode().strip().split("\n"):
            lines.append("    " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
