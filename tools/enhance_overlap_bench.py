"""GPU box: what overlapped, cross-faded chunks and batched recordings cost and buy in inference.enhance / enhance_many.  In one
process, median of --reps timed calls after warm-up calls of the same shapes; a call is timed by HIP events around it and ends in a
device synchronise (host time of the tables, their copies and the launches included).
  (i)   the two kernels (Engine.chunk_gather + Engine.chunk_overlap_add on tables already on the device) on one recording of 10 minutes
        at 16 kHz, L = 16384, margin = fade = 2048 (hop 10240), against the same result assembled from torch ops (F.pad / unfold /
        slicing / lerp - written in this tool only), both also as algorithmic bytes moved per second
  (ii)  enhance() of that recording with the 12-level model, with and without the overlap, end to end; the overlap costs L / H times
        the forwards by construction, the measured ratio is printed beside that figure
  (iii) enhance_many() over 64 recordings of 2 - 10 s against a loop of enhance() over the same recordings, margin = fade = 0
There is no pass / fail time: the file records the measurement.  No figure on quality is produced: there are no trained weights here.
    python tools/enhance_overlap_bench.py [--out profiles/enhance_overlap_bench.txt] [--reps 20] [--commit <hash>]
    python tools/enhance_overlap_bench.py --default-only [--root <checkout>]    # only the default path (margin = fade = 0) of (ii) and
        (iii)'s loop, through enhance(model, mixture, sample_length) alone, so that it also runs on a checkout without this feature:
        run it on both checkouts, alternating, to see whether the default path moved beyond its own spread"""
import argparse
import importlib
import os
import socket
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--default-only", action="store_true")
ap.add_argument("--minutes", type=float, default=10.0)
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)
PKG = "wave-u-net-for-speech-enhancement_amd"
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 5
pkg = importlib.import_module(PKG)
inference = importlib.import_module(PKG + ".inference")
dev = torch.device("cuda:0")
RATE, L, M, FADE = 16000, 16384, 2048, 2048
H = L - 2 * M - FADE
T = int(args.minutes * 60 * RATE)


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                # ms


def measure(call, reps=None, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    t = [timed(call) for _ in range(reps or args.reps)]
    return statistics.median(t), min(t), max(t)


fmt = lambda t: f"{t[0]:.3f} [min {t[1]:.3f}, max {t[2]:.3f}]"          # noqa: E731
rng = np.random.default_rng(0)
long_rec = torch.from_numpy(rng.uniform(-0.5, 0.5, T).astype(np.float32)).to(dev).view(1, 1, T)
lengths = [int(v) for v in rng.integers(2 * RATE, 10 * RATE + 1, 64)]
recs = [torch.from_numpy(rng.uniform(-0.5, 0.5, n).astype(np.float32)).to(dev).view(1, 1, n) for n in lengths]
torch.manual_seed(0)
model = pkg.Model().to(dev).eval()
head = (f"enhance with overlapped chunks on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}, commit {args.commit}, torch {torch.__version__}), "
        f"median of {args.reps} calls after 3 warm-up calls, HIP events around a call that ends in a synchronise, ms per call")

if args.default_only:
    whole = lambda: inference.enhance(model, long_rec, L)                              # noqa: E731
    loop = lambda: [inference.enhance(model, x, L) for x in recs]                      # noqa: E731
    t_whole, t_loop = measure(whole), measure(loop)
    text = "\n".join([f"default path only (margin = fade = 0, through enhance(model, mixture, sample_length) alone), commit {args.commit}, on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}), "
                      f"median of {args.reps} calls after 3 warm-up calls, ms per call",
                      f"  enhance(), margin = fade = 0, one recording of {T} samples:                 {fmt(t_whole)}",
                      f"  loop of enhance() over 64 recordings of 2 - 10 s, margin = fade = 0:          {fmt(t_loop)}"]) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as f:
            f.write(text)
    sys.exit(0)

engine = importlib.import_module(PKG + ".engine").default_engine()

# ---- (i) the two kernels against torch ops, no model in between (the overlap-add reads the gathered chunks)
rows_np, recs_np, _ = inference.chunk_tables([T], L, M, FADE)
n = rows_np.shape[0]
rows, rtab = torch.from_numpy(rows_np).to(dev), torch.from_numpy(recs_np).to(dev)
ramp = inference.chunk_ramp(FADE, "hann").to(dev)
flat = long_rec.view(-1)
chunks, out = torch.empty(n, 1, L, device=dev), torch.empty(T, device=dev)


def kernels():
    engine.chunk_gather(flat, rows, chunks)
    engine.chunk_overlap_add(chunks, rtab, out, M, FADE, ramp, T)


def torch_ops():
    padded = F.pad(flat, (M, (n - 1) * H + L - M - T))
    y = padded.unfold(0, L, H).contiguous()                                           # the gather: [n, L]
    ups, body, downs = y[:, M:M + FADE], y[:, M + FADE:M + H], y[:, M + H:M + H + FADE]
    first = torch.cat([ups[:1], torch.lerp(downs[:-1], ups[1:], ramp)])                # [n, FADE]: no up-ramp on the first chunk
    return torch.cat([torch.cat([first, body], dim=1).reshape(-1), downs[-1]])[:T]    # no down-ramp on the last


t_k, t_t = measure(kernels), measure(torch_ops)
kernels()
d_kt = float((torch_ops() - out).abs().max())
bytes_gather = 4.0 * 2.0 * n * L
bytes_ola = 4.0 * (2.0 * T + 2.0 * (n - 1) * FADE)
moved = bytes_gather + bytes_ola

# ---- (ii) the cost of the overlap, end to end with the 12-level model
plain = lambda: inference.enhance(model, long_rec, L)                                  # noqa: E731
over = lambda: inference.enhance(model, long_rec, L, margin=M, fade=FADE)              # noqa: E731
t_plain, t_over = measure(plain, reps=max(5, args.reps // 2)), measure(over, reps=max(5, args.reps // 2))
n_plain = -(-T // L)

# ---- (iii) batching: many recordings per pass against one recording per pass, margin = fade = 0
loop = lambda: [inference.enhance(model, x, L) for x in recs]                          # noqa: E731
many = lambda: inference.enhance_many(model, recs, L)                                  # noqa: E731
t_loop, t_many = measure(loop, reps=max(5, args.reps // 2)), measure(many, reps=max(5, args.reps // 2))
a, b = loop(), many()
d_many = max(float((x - y).abs().max()) for x, y in zip(a, b))
same_bits = all(torch.equal(x, y) for x, y in zip(a, b))
n_many = sum(-(-v // L) for v in lengths)

lines = [head,
         f"(i) gather + overlap-add of one recording of {T} samples ({args.minutes:g} min at {RATE} Hz), L {L} margin {M} fade {FADE} hop {H}: {n} chunks, tables on the device",
         f"      Engine.chunk_gather + Engine.chunk_overlap_add (two launches):     {fmt(t_k)}",
         f"      the same from torch ops (F.pad, unfold, slicing, lerp, cat):       {fmt(t_t)}",
         f"      algorithmic bytes: gather {bytes_gather / 1e6:.1f} MB (reads and writes n L floats), overlap-add {bytes_ola / 1e6:.1f} MB (reads T + (n - 1) f, "
         f"writes T floats, plus the fades' second operand) = {moved / 1e6:.1f} MB",
         f"      -> kernels {moved / (t_k[0] * 1e-3) / 1e12:.3f} TB/s, torch ops {moved / (t_t[0] * 1e-3) / 1e12:.3f} TB/s of those bytes over the medians "
         f"(launch gaps and host time included; the torch ops move more than these bytes)",
         f"      (chunks {4.0 * n * L / 1e6:.0f} MB + input and output {2 * 4.0 * T / 1e6:.0f} MB: the working set fits the 256 MB Infinity Cache across the timed calls, so this is not an HBM rate)",
         f"      torch ops / kernels = {t_t[0] / t_k[0]:.2f} x;  max |torch ops - kernels| = {d_kt:.2e} (lerp is a + w (b - a), the kernel w b + (1 - w) a)",
         f"(ii) enhance() of that recording, 12-level model (default init, eval), end to end",
         f"      margin = fade = 0 ({n_plain} chunks):                               {fmt(t_plain)}",
         f"      margin {M}, fade {FADE} ({n} chunks):                          {fmt(t_over)}",
         f"      measured ratio {t_over[0] / t_plain[0]:.3f}; by construction L / H = {L / H:.3f} times the forwards ({n} / {n_plain} = {n / n_plain:.3f} chunks)",
         f"(iii) 64 recordings of 2 - 10 s ({sum(lengths)} samples, {n_many} chunks), margin = fade = 0",
         f"      loop of enhance(), one recording per pass:                          {fmt(t_loop)}",
         f"      enhance_many(), shared slabs:                                       {fmt(t_many)}",
         f"      loop / enhance_many = {t_loop[0] / t_many[0]:.2f} x;  results bit-equal: {same_bits}, max |difference| {d_many:.2e} "
         f"(the network's plan depends on the slab size)",
         "no figure on quality: that seams between disjoint chunks are audible with trained weights is an expectation from the literature, "
         "not measured here (no trained weights)"]
text = "\n".join(lines) + "\n"
print(text, end="")
out_path = args.out or os.path.join(ROOT, "profiles", "enhance_overlap_bench.txt")
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
