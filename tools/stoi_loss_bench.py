"""GPU box: what loss.stoi_loss costs.  In one process, HIP-event times, median of >= 20 after 3 warm-up calls (eager calls, host launch
time included), at 64 x 16384 at 16 kHz - the product's training chunk, one batch:
  the loss       forward + backward of loss.stoi_loss (and the forward alone), with the per-kernel times from the library's profiler;
  (a) the metric metrics.stoi alone on the same inputs;
  (b) torch ops  the same loss and gradient from torch ops and autograd on the device, batched over the rows (conv1d resampling, unfold /
                 fold framing, torch.fft, unfold segments) in float32: what a user can write today.  Its loss and gradient are printed
                 against the kernels' so that the two are seen to compute the same thing.
There is no pass / fail time: the file records the first measurement.  --extended measures loss.stoi_loss(extended=True) (ESTOI): the
same torch graph with the segment step replaced by the two normalisations.
    python tools/stoi_loss_bench.py [--out profiles/stoi_loss_bench.txt] [--reps 30] [--commit <hash>] [--extended]"""
import argparse
import ctypes
import importlib
import os
import socket
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "wave-u-net-for-speech-enhancement_amd"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_loss_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--extended", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
import stoi_ref as R  # noqa: E402
metrics = importlib.import_module(PKG + ".metrics")
loss_mod = importlib.import_module(PKG + ".loss")
engine = importlib.import_module(PKG + ".engine").default_engine()
dev = torch.device("cuda:0")
FS, ROWS, T = 16000, 64, 16384


class TorchStoiLoss:
    """-mean STOI of [rows, T] float32 device tensors from torch ops, batched over the rows; autograd gives the gradient."""

    def __init__(self, fs, device, extended=False):
        self.extended = extended
        p, q, L, h = R.taps(fs)
        self.p, self.q, self.L = p, q, L
        self.h = torch.from_numpy(h[::-1].copy()).float().to(device)[None, None, :]
        self.w = torch.from_numpy(R.WINDOW).float().to(device)
        bands = np.zeros((R.NFFT // 2 + 1, R.BANDS), np.float32)
        for i, (a, b) in enumerate(R.band_edges()):
            bands[a:b, i] = 1.0
        self.bands = torch.from_numpy(bands).to(device)

    def resample(self, x):
        up = torch.zeros(x.shape[0], 1, x.shape[1] * self.p, device=x.device)
        up[:, 0, ::self.p] = x
        return self.p * F.conv1d(up, self.h, stride=self.q, padding=self.L)[:, 0]

    def __call__(self, clean, est):
        x, y = self.resample(clean), self.resample(est)
        n = x.shape[1]
        F0 = len(R.frame_starts(n))
        xf, yf = x.unfold(1, R.N_FRAME, R.HOP)[:, :F0] * self.w, y.unfold(1, R.N_FRAME, R.HOP)[:, :F0] * self.w
        en = 20.0 * torch.log10(xf.detach().norm(dim=2) + R.EPS)
        keep = en > en.max(dim=1, keepdim=True).values - R.DYN_RANGE
        nk = keep.sum(dim=1)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)                     # the kept frames first, in their order
        live = (torch.arange(F0, device=x.device)[None, :] < nk[:, None])[:, :, None]
        gather = order[:, :, None].expand(-1, -1, R.N_FRAME)
        size = (1, (F0 - 1) * R.HOP + R.N_FRAME)
        spec = []
        for f in (xf, yf):
            kept = torch.gather(f, 1, gather) * live
            s = F.fold(kept.transpose(1, 2), size, (1, R.N_FRAME), stride=(1, R.HOP))[:, 0, 0]
            fr = s.unfold(1, R.N_FRAME, R.HOP)[:, :F0 - 1] * self.w
            sp = torch.fft.rfft(fr, R.NFFT, dim=2)
            spec.append(sp.real ** 2 + sp.imag ** 2)
        nfr = nk - 1
        fl = (torch.arange(F0 - 1, device=x.device)[None, :] < nfr[:, None])[:, :, None]
        X, Y = (torch.sqrt(torch.where(fl, P, torch.ones_like(P)) @ self.bands) for P in spec)   # (dead frames: 1, no sqrt(0) in the backward)
        xs, ys = X.unfold(1, R.SEG, 1), Y.unfold(1, R.SEG, 1)                                   # [rows, segments, 15, 30]
        nseg = (nfr - R.SEG + 1).clamp(min=0)
        sl = torch.arange(xs.shape[1], device=x.device)[None, :] < nseg[:, None]
        if self.extended:                                                                       # ESTOI: per band over the frames, then per frame over the bands
            def normalise(a, dim):
                a = a - a.mean(dim=dim, keepdim=True)
                return a / (a.norm(dim=dim, keepdim=True) + R.EPS)
            d = (normalise(normalise(xs, 3), 2) * normalise(normalise(ys, 3), 2)).sum(dim=(2, 3)) / R.SEG
            score = torch.where(sl, d, torch.zeros_like(d)).sum(dim=1) / nseg.clamp(min=1)
            return -torch.where(nseg > 0, score, torch.full_like(score, R.SHORT)).mean()
        alpha = xs.norm(dim=3, keepdim=True) / (ys.norm(dim=3, keepdim=True) + R.EPS)
        yp = torch.minimum(alpha * ys, R.CLIP * xs)
        xs = xs - xs.mean(dim=3, keepdim=True)
        yp = yp - yp.mean(dim=3, keepdim=True)
        d = (xs * yp).sum(dim=3) / ((xs.norm(dim=3) + R.EPS) * (yp.norm(dim=3) + R.EPS))
        d = torch.where(sl[:, :, None], d, torch.zeros_like(d))
        score = d.sum(dim=(1, 2)) / (nseg.clamp(min=1) * R.BANDS)
        return -torch.where(nseg > 0, score, torch.full_like(score, R.SHORT)).mean()


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
    return f"{statistics.median(t):.3f} [min {min(t):.3f}, max {max(t):.3f}]"


c, e = R.pair(4, T, FS)
cd, ed = c.repeat(ROWS // 4, 1).to(dev), e.repeat(ROWS // 4, 1).to(dev)      # (64 rows: the four generated ones, 16 times)
EXT = {"extended": True} if args.extended else {}
NAME = "stoi_loss(extended=True)" if args.extended else "stoi_loss"
crit = loss_mod.stoi_loss(sample_rate=FS, **EXT)
ref = TorchStoiLoss(FS, dev, args.extended)
x = ed.clone().requires_grad_(True)


def hip_step():
    x.grad = None
    loss = crit(cd, x)
    loss.backward()
    return loss


def torch_step():
    x.grad = None
    loss = ref(cd, x)
    loss.backward()
    return loss


lh = hip_step()
gh = x.grad.clone()
lt = torch_step()
gt = x.grad.clone()
torch.cuda.synchronize()
lines = [f"loss.{NAME} at {FS} Hz, {ROWS} x {T}, on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}, commit {args.commit}, torch {torch.__version__}), "
         f"median of {args.reps} eager calls after 3 warm-up calls, HIP events, ms per call",
         f"  {NAME} forward + backward (HIP kernels): {measure(hip_step)}",
         f"  {NAME} forward alone (no_grad):          {measure(lambda: engine.stoi_loss_forward(cd, ed, FS, **EXT))}",
         f"  (a) metrics.stoi alone, same mode:          {measure(lambda: metrics.stoi(cd, ed, sample_rate=FS, **EXT))}",
         f"  (b) torch ops + autograd, float32, batched: {measure(torch_step)}",
         f"  the two compute the same thing: loss {lh.item():.8f} (HIP) / {lt.item():.8f} (torch ops); max |g_hip - g_torch| / max |g_hip| "
         f"{float((gh - gt).abs().max() / gh.abs().max()):.2e}; max |g_hip| {float(gh.abs().max()):.3e}",
         "  (c) the default training step is 4.78 - 5.07 ms (README.md)"]
engine.lib.wunet_profile_enable(1)
for _ in range(5):
    hip_step()
buf = ctypes.create_string_buffer(1 << 16)
n = engine.lib.wunet_profile_collect(buf, len(buf))
engine.lib.wunet_profile_enable(0)
if n > 0:
    lines.append("    per-kernel time from the library's profiler, 5 forward + backward calls (name, launches, total ms, algorithmic flops, algorithmic bytes):")
    for ln in buf.value.decode().strip().split("\n"):
        lines.append("      " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
