"""The single-op cases of the fp16-split kernels (conv_h3d_kernel forward and data gradient, wgrad_h3d_kernel / wgrad_h3_kernel) and
the ragged nets of the per-layer forward check, shared by the CPU emulator tests (tests/test_emu_split_ops.py) and the MI355X tests
(tests/test_gpu_split_ops_ragged.py): which shapes, which operands, the float64 reference (oracle/wunet_oracle.c, f64 build) and how a
result is measured against it.  Plain data and helpers: what is asserted at which bar is each test module's own business."""
import ctypes
import functools

import numpy as np
import torch

from oracle import c_oracle, plan

# (B, Cin, Cout, L, K, xs, ws): xs / ws scale the activations / the weights (the kernels derive power-of-two operand scales from the
# measured maxima: magnitudes far from 1 must not cost precision)
CASES = [
    (1, 24, 40, 256, 15, 1.0, 1.0),        # one un-segmented tile
    (2, 20, 24, 512, 5, 1e-4, 3e3),        # channel counts off the 8 / 16 grid; small activations, large weights
    (3, 48, 24, 128, 5, 50.0, 1e-5),       # two-item tiles, odd batch (half-empty tile)
    (5, 16, 56, 64, 15, 1.0, 1.0),         # four-item tiles
    (9, 72, 40, 32, 5, 1e3, 1e-3),         # eight-item tiles: 2 items under one wave
    (17, 40, 72, 16, 15, 1.0, 1.0),        # sixteen-item tiles: 4 items under one wave
    # K tails of conv_h3d_kernel (channel groups left over after the last chunk of 32: one tail stage per group, taps spread over
    # the K quarters of the MFMA) - the cases above already hold 1 / 2 / 3 left-over groups with and without a full chunk; here
    # behind two full chunks, split K with splits that start inside the tail, and a 5-tap tail behind three chunks
    (2, 72, 80, 512, 15, 1.0, 1.0),        # 9 groups forward (2 chunks + 1), 10 backward (2 chunks + 2)
    (3, 104, 24, 256, 5, 1.0, 1.0),        # 13 groups forward: 3 chunks + a 5-tap tail stage of 2 steps
    # ragged on several axes at once, each at the smallest size that reaches it
    (16, 16, 16, 16, 5, 1.0, 1.0),         # the smallest shape the ops accept on every axis (L = 16, B * L = 256, Cin = 16)
    (33, 24, 24, 16, 5, 1.0, 1.0),         # sixteen-item tiles with ONE item in the last tile
    (7, 60, 20, 64, 5, 1.0, 1.0),          # four-item tiles, odd batch; Cin = 60 (7.5 groups) and Cout = 20 both off the 8-grid
    (5, 100, 60, 128, 15, 1.0, 1.0),       # two-item tiles, odd batch; 12.5 groups; the wgrad_h3d / wgrad_h3 boundary at L = 128
    (1, 20, 24, 256, 15, 1.0, 1.0),        # one item, one un-segmented tile, 2.5 groups
    (3, 20, 40, 1024, 5, 1.0, 1.0),        # several tiles per item; ragged Cin; 5 taps
    (2, 28, 36, 2048, 15, 1.0, 1.0),       # 3.5 groups in, 4.5 out; the long-level DMA-staged path
]

# the cases with left-over channel groups in the forward conv or in the data gradient: also run with the K tail switched off
KTAIL_CASES = [c for c in CASES if c[:5] in ((2, 72, 80, 512, 15), (3, 104, 24, 256, 5), (2, 28, 36, 2048, 15), (5, 100, 60, 128, 15))]


def case_id(case):
    B, Cin, Cout, L, K = case[:5]
    return f"B{B}-{Cin}x{Cout}-L{L}-k{K}"


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def operands(case):
    """x [B, Cin, L], w [Cout, Cin, K], bias [Cout], gz [B, Cout, L] of one case (float32, read-only)."""
    B, Cin, Cout, L, K, xs, ws = case
    rng = np.random.default_rng(B * 1000 + Cin)
    x = (xs * rng.standard_normal((B, Cin, L))).astype(np.float32)
    w = (ws * rng.standard_normal((Cout, Cin, K)) / np.sqrt(Cin * K)).astype(np.float32)
    b = (xs * ws * rng.standard_normal((Cout,))).astype(np.float32)
    gz = (rng.standard_normal((B, Cout, L)) / xs).astype(np.float32)
    return _frozen(x, w, b, gz)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(z, dx, dw) of one case in float64 arithmetic (read-only; computed once per process)."""
    x, w, b, gz = operands(case)
    z = c_oracle.conv1d_fwd(x, w, b)
    dx, dw, _ = c_oracle.conv1d_bwd(gz, x, w)
    return _frozen(z, dx, dw)


def errors(got, ref):
    """(tensor-relative norm of the difference, largest difference relative to the largest |ref|)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    d = got - ref
    return (float(np.linalg.norm(d.ravel()) / max(np.linalg.norm(ref.ravel()), 1e-30)),
            float(np.abs(d).max() / max(np.abs(ref).max(), 1e-30)))


def profiled(lib, fn):
    """{kernel name: launches} of the annotated kernels `fn` launched (wunet_profile_enable / _collect)."""
    lib.wunet_profile_enable(1)
    try:
        fn()
        buf = ctypes.create_string_buffer(1 << 16)
        lib.wunet_profile_collect(buf, len(buf))
    finally:
        lib.wunet_profile_enable(0)
    return {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().strip().splitlines()}


# ---------------------------------------------------------------------------------------------------------------------
# per-layer forward on ragged nets: (n, ci, B, T), weights plan.golden_state(n, ci, 0), batch plan.golden_batch(B, T, 5)
NETS = [
    (3, 20, 3, 2048),      # ragged channel groups on every layer (2.5, 5, 7.5 ... groups), odd batch
    (2, 28, 1, 1024),      # batch 1, 3.5-group channels
    (3, 16, 2, 768),       # 768 = 3 * 2^8 samples: rows of 768 / 384 / 192 / 96 padded to 1024 / 512 / 256 / 128
]


def net_id(net):
    return "n%d-ci%d-B%d-T%d" % net


@functools.lru_cache(maxsize=None)
def net_reference(net, training):
    """(noisy, network output, raw conv output of every layer) of one net in float64 arithmetic (read-only)."""
    n, ci, B, T = net
    noisy, clean = plan.golden_batch(B, T, 5)
    ref = c_oracle.step(plan.golden_state(n, ci, 0), noisy, clean, n, ci, training, "mse", want_grads=False, want_acts=True, precision="f64")
    _frozen(noisy, ref["out"], *ref["acts"])
    return noisy, ref["out"], ref["acts"]


def check_layer_forward(engine, device, net, training):
    """One forward of `net` on `engine` (tensors on `device`): every layer's raw conv output against the float64 one at
    2e-5 * max(1, max |z_ref|) (the bar of test_layer_activations_vs_oracle), the network output at 1e-5.  A length that is no power of
    two runs in rows padded to the next one: engine.layer_output returns the padded rows, their first Lt columns are compared, and the
    row padding of every conv's OPERAND must be exactly zero (the conv's zero padding at the true end of the row).  The operand itself
    is not reachable from here (only raw conv outputs are), its padding is observed through the conv that reads it: a raw output
    column K/2 or more behind the true end sees nothing but operand padding (and the zeros behind the row), so it holds exactly the
    bias - the products of exact zeros - for every item and channel, if and only if all of that padding is zero.
    Returns (worst layer error relative to its bar's scale, output error)."""
    n, ci, B, T = net
    noisy, ref_out, ref_acts = net_reference(net, training)
    sd = plan.golden_state(n, ci, 0)
    params = [torch.tensor(sd[k]).to(device) for k in plan.param_names(n, ci)]
    bnames = plan.buffer_names(n, ci)
    running = [torch.tensor(sd[k]).to(device) for k in bnames if not k.endswith("num_batches_tracked")]
    nbt = [torch.tensor(int(sd[k]), dtype=torch.int64).to(device) for k in bnames if k.endswith("num_batches_tracked")]
    out, ws = engine.forward(n, ci, torch.tensor(noisy).to(device), params, running, nbt, training, False)
    if out.is_cuda:
        torch.cuda.synchronize()
    worst = 0.0
    for i, (prefix, _, cout, K) in enumerate(plan.conv_layers(n, ci)):
        z = engine.layer_output(n, ci, B, T, ws, i).cpu().numpy()
        r = ref_acts[i]
        Lt = r.shape[-1]
        assert z.shape[:2] == r.shape[:2] and z.shape[-1] >= Lt, (prefix, z.shape, r.shape)
        assert np.isfinite(z).all(), prefix
        scale = max(1.0, float(np.abs(r).max()))
        err = float(np.abs(z[..., :Lt] - r).max()) / scale
        worst = max(worst, err)
        assert err < 2e-5, (prefix, i, err)
        if z.shape[-1] > Lt:
            assert z.shape[-1] - Lt > 2 * (K // 2)          # (every padding column is read by a raw output column checked here)
            bias = sd[prefix + ".0.bias"]
            assert np.array_equal(z[..., Lt + K // 2:], np.broadcast_to(bias[None, :, None], z[..., Lt + K // 2:].shape)), prefix
    oe = float(np.abs(out.detach().cpu().numpy() - ref_out).max())
    assert oe < 1e-5, oe
    return worst, oe
