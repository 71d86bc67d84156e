"""GPU box: what metrics.stoi costs.  In one process, HIP-event times, median of >= 20 after warm-up (eager calls, host launch time
included), at
  (a) 64 x 16384 at 16 kHz - the product's training chunk, one batch
  (b) 1 x 960000 at 16 kHz - one 60 s recording, what a validation epoch scores
and, on the same host, the wall time of the float64 CPU yardstick (tests/stoi_ref.py: oracle64 - numpy / scipy, one row at a time,
the way the reference's validation epoch calls pystoi) on the same inputs, with the distance between the two.  Also printed: the
per-kernel times of (a) and (b) from the library's profiler.  There is no pass / fail time: the file records the first measurement.
--extended measures metrics.stoi(extended=True) (ESTOI) against tests/estoi_ref.py instead.
    python tools/stoi_bench.py [--out profiles/stoi_bench.txt] [--reps 30] [--commit <hash>] [--extended]"""
import argparse
import ctypes
import importlib
import os
import socket
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "wave-u-net-for-speech-enhancement_amd"
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench.txt"))
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--commit", default="unknown")
ap.add_argument("--extended", action="store_true")
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 20
import stoi_ref as R  # noqa: E402
import estoi_ref as E  # noqa: E402
metrics = importlib.import_module(PKG + ".metrics")
engine = importlib.import_module(PKG + ".engine").default_engine()
dev = torch.device("cuda:0")
FS = 16000
SHAPES = {"64 x 16384": (64, 16384), "1 x 960000 (60 s)": (1, 960000)}


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)                # ms


NAME = "metrics.stoi(extended=True)" if args.extended else "metrics.stoi"
lines = [f"{NAME} at {FS} Hz on {torch.cuda.get_device_name(0)} (host {socket.gethostname()}, commit {args.commit}, torch {torch.__version__}), "
         f"median of {args.reps} eager calls after 3 warm-up calls, HIP events, ms per call"]
for label, (rows, T) in SHAPES.items():
    c, e = R.pair(rows if rows < 4 else 4, T, FS)
    c, e = c.repeat(rows // c.shape[0], 1), e.repeat(rows // e.shape[0], 1)     # (64 rows: the four generated ones, 16 times)
    cd, ed = c.to(dev), e.to(dev)
    call = lambda: metrics.stoi(cd, ed, sample_rate=FS, return_frames=True, extended=args.extended)     # noqa: E731
    for _ in range(3):
        score, frames = call()
    torch.cuda.synchronize()
    times = [timed(call) for _ in range(args.reps)]
    t0 = time.perf_counter()
    s64, f64 = (E if args.extended else R).oracle64(c, e, FS)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    d = float(np.abs(score.double().cpu().numpy() - s64).max())
    same = list(frames.cpu().numpy()) == list(f64)
    lines.append(f"  {label}: device {statistics.median(times):.3f} [min {min(times):.3f}, max {max(times):.3f}]   float64 CPU yardstick on this host "
                 f"{cpu_ms:.0f} (one run, one core)   max |device - yardstick| {d:.2e}, frame counts {'equal' if same else 'DIFFER'} "
                 f"({int(f64.min())} .. {int(f64.max())} spectral frames a row)")
    engine.lib.wunet_profile_enable(1)
    for _ in range(5):
        call()
    buf = ctypes.create_string_buffer(1 << 16)
    n = engine.lib.wunet_profile_collect(buf, len(buf))
    engine.lib.wunet_profile_enable(0)
    if n > 0:
        lines.append("    per-kernel time from the library's profiler, 5 calls (name, launches, total ms, algorithmic flops, algorithmic bytes):")
        for ln in buf.value.decode().strip().split("\n"):
            lines.append("      " + ln.replace("\t", "  "))
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
