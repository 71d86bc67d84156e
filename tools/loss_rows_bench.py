"""GPU box: what the row losses cost next to the element-wise ones.  In one process at 64 x 16384 (8 MB read, 4 MB written either
way), HIP-event times, median of >= 50 after warm-up, alternating:
  (a) mse    forward + backward through wunet_loss_forward / wunet_loss_backward            (engine.loss_forward / loss_backward)
  (b) si_sdr forward + backward through wunet_loss_rows_forward / wunet_loss_rows_backward  (engine.loss_rows_forward / _backward)
each as eager calls (host launch time included) and as a captured graph of 20 pairs (kernel time and launch boundaries only).
    python tools/loss_rows_bench.py [--out profiles/loss_rows_bench.txt] [--reps 60]"""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_rows_bench.txt"))
ap.add_argument("--reps", type=int, default=60)
args = ap.parse_args()
assert torch.cuda.is_available(), "needs an MI355X"
assert args.reps >= 50
engine = importlib.import_module(PKG + ".engine").default_engine()
dev = torch.device("cuda:0")
B, T, PAIRS = 64, 16384, 20
g = torch.Generator().manual_seed(1)
clean = torch.rand(B, 1, T, generator=g) * 2 - 1
enh = (0.8 * clean + 0.1 * torch.randn(B, 1, T, generator=g)).to(dev)
clean = clean.to(dev)
one = torch.ones((), device=dev)


def mse():
    loss = engine.loss_forward("mse", clean, enh)
    return loss, engine.loss_backward("mse", clean, enh, one)


def si_sdr():
    loss, coefs, _ = engine.loss_rows_forward("si_sdr", clean, enh)
    return loss, engine.loss_rows_backward("si_sdr", clean, enh, coefs, one)


def captured(fn):
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        keep = [fn() for _ in range(PAIRS)]
    return graph, keep


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


cases = {"mse": mse, "si_sdr": si_sdr}
for fn in cases.values():
    for _ in range(10):
        fn()
torch.cuda.synchronize()
graphs = {k: captured(fn) for k, fn in cases.items()}
for gr, _ in graphs.values():
    for _ in range(5):
        gr.replay()
torch.cuda.synchronize()
eager = {k: [] for k in cases}
graph = {k: [] for k in cases}
for _ in range(args.reps):
    for k, fn in cases.items():               # alternating: both see the same box at the same time
        eager[k].append(timed(fn))
        graph[k].append(timed(graphs[k][0].replay) / PAIRS)
lines = [f"loss forward + backward at {B} x {T} (8 MB read, 4 MB written), {torch.cuda.get_device_name(0)}, median of {args.reps}, us per pair"]
for name, res in (("eager calls (host launches included)", eager), (f"captured graph of {PAIRS} pairs", graph)):
    a, b = statistics.median(res["mse"]), statistics.median(res["si_sdr"])
    lines.append(f"  {name}: (a) mse {a:.2f}  (b) si_sdr {b:.2f}  ratio b / a {b / a:.3f}   "
                 f"[min {min(res['mse']):.2f} / {min(res['si_sdr']):.2f}, max {max(res['mse']):.2f} / {max(res['si_sdr']):.2f}]")
a = statistics.median(graph["mse"])
b = statistics.median(graph["si_sdr"])
lines.append(f"  bytes over kernel time (captured): mse {12.58 / a:.2f} TB/s, si_sdr {12.58 / b:.2f} TB/s  (12.58 MB per pair)")
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
