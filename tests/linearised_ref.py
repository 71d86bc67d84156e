"""TEST INFRASTRUCTURE ONLY: the backward pass against a float64 arbiter LINEARISED AT THE DEVICE'S OWN FORWARD POINT, shared by the
emulator test (tests/test_emu_backward_linearised.py) and the hardware test (tests/test_gpu_backward_linearised.py).

Every backward kernel differentiates the network at the forward point the device saved: its own raw conv outputs z_i.  The arbiter
here restates oracle/torch_port.forward (training=True) with every conv output REPLACED by the device's z_i (the gradient passes
through unchanged), so the forward's 1e-7 .. 1e-6 of noise and the LeakyReLU slopes it flips drop out of the comparison and only the
backward's own rounding remains: ~1e-6 of a tensor instead of the 3e-4 .. 6e-2 the plain-arbiter gradient tests have to allow.

Two runs per case: float64 (the arbiter) and float32 (the reference's own ATen arithmetic at the same point: its distance to the
arbiter, d_ref, is the yardstick of the bar - measured at test time, never taken from the code under test).

Ambiguous slopes: the device forms y = a z + s in fp32, the arbiter in float64; where |y| is within fp32 rounding of 0 the two may
legitimately disagree about LeakyReLU's slope.  An element is ambiguous when |y64| <= 16 * 2^-24 * (|a z| + |s|) (a, s: the arbiter's);
with k of them the arbiter is built for all 2^k choices and the one nearest the device's gradients is accepted (k <= 4, else the case
fails)."""
import ctypes
import fnmatch
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import plan, torch_port

MAX_AMBIGUOUS = 4
AMBIGUOUS_ULPS = 16.0 * 2.0 ** -24
ABS_BAR = 1e-4                       # the absolute bar of the plain-arbiter gradient tests (tests/test_gpu_parity.py: TOL)
MARGIN = {0: 2.0, 2: 4.0}            # h3 -> margin over d_ref: fp32 MFMA (same precision, another summation order); fp16-split (22 of 24 bits)
BATCH_SEED, UPSTREAM_SEED = 0, 3

NS = {"WUNET_H3_NOSPLIT": "1"}
# (h3, n, ci, B, T, environment, frozen layers (C ABI order), kernel-name prefixes the profile must contain).  Every case stays under
# ~3 M activations: the expected number of ambiguous slopes is about 1.6e-6 per activation.
CASES = [
    # ---- fp32 MFMA path
    (0, 3, 10, 3, 128, {}, (), ("conv_mfma_kernel", "wgrad_mfma_kernel", "pass_a_kernel<UP>", "pass_a_kernel<ENC>", "pass_a_kernel<HEAD>",
                                "input_grad_kernel<GZ>")),                                         # odd batch, ragged channels
    (0, 4, 6, 2, 80, {}, (), ("conv_mfma_kernel", "pass_a_kernel<UP>", "pass_a_kernel<ENC>")),    # rows of 80 / 40 / 20 / 10 / 5, padded
    (0, 4, 4, 2, 16, {}, (), ("pass_a_scalar_kernel<UP>", "pass_a_scalar_kernel<ENC>", "gz_scalar_kernel", "tiny_wgrad_kernel")),    # a middle of 1 sample
    (0, 3, 8, 2, 16, {}, (), ("pass_a_scalar_kernel<UP>", "gz_scalar_kernel", "tiny_wgrad_kernel")),                               # ... of 2 samples
    (0, 3, 10, 3, 128, {}, (0, 2, 3, 5), ("pass_a_kernel<UP>", "pass_a_kernel<ENC>")),            # frozen: two encoder layers, the middle, a decoder layer
    # ---- fp16-split path
    (2, 2, 24, 2, 1024, {}, (), ("conv_h3d_kernel<5, *upt>", "pass_a_kernel<UPH>", "gz_split_h3_kernel", "wgrad_h3")),
    (2, 3, 16, 3, 1024, {}, (), ("conv_h3d_kernel", "pass_a_kernel<ENC>", "gz_split_h3_kernel", "wgrad_h3d_kernel", "wgrad_h3_reduce_kernel")),   # a 128-sample level, two-item tiles
    (2, 3, 20, 3, 2048, {}, (), ("conv_h3d_kernel<15", "conv_h3d_kernel<5, *upt>", "wgrad_h3d_kernel<15", "wgrad_h3d_kernel<5", "pass_a_kernel<UPH>")),    # ragged channel groups, K tails
    (2, 3, 16, 3, 768, {}, (), ("conv_h3d_kernel", "pass_a_kernel<UP>", "gz_split_h3_kernel")),      # rows of 768 / 384 / 192 / 96, padded (no UPT hand-off there)
    (2, 2, 24, 3, 1536, {}, (), ("conv_h3d_kernel", "pass_a_kernel<UP>", "gz_split_h3_kernel")),     # rows of 1536 / 768 / 384, padded
    (2, 6, 16, 17, 1024, {}, (), ("conv_h3d_kernel<15", "wgrad_h3_kernel<15", "wgrad_h3_kernel<5", "wgrad_h3d_kernel", "gz_split_h3_kernel")),      # 32- and 16-sample levels: 2 / 4 items under a wave; both weight-gradient kernels
    (2, 3, 24, 3, 2048, NS, (), ("pass_a_kernel<ENC, e0>", "pass_a_kernel<ENC>", "gz_split_h3_kernel", "input_grad_kernel<ENC>")),   # unsplit encoder levels
    (2, 2, 16, 5, 512, {**NS, "WUNET_NO_E0": "1"}, (), ("input_grad_kernel<G>", "wgrad_mfma_kernel")),   # the first layer's g stored, g_z formed by its weight gradient
    (2, 3, 16, 3, 1024, {"WUNET_REDUCE_SERIAL": "100000,0"}, (), ("wgrad_h3_reduce_serial_kernel",)),  # (a hook of the emulator build: EVERY split reduce on the serial kernel; the hardware runs it where the planner puts it)
    (2, 3, 16, 3, 768, {}, (1, 3, 4, 6), ("conv_h3d_kernel", "gz_split_h3_kernel")),                 # frozen: an encoder layer, the middle, two decoder layers
]


def case_id(case):
    h3, n, ci, B, T, env, frozen, _ = case
    tag = "".join("-" + k.replace("WUNET_", "").lower() for k in env) + ("-frozen" if frozen else "")
    return f"h3_{h3}-n{n}-ci{ci}-B{B}-T{T}{tag}"


def inputs(case):
    """(state dict, noisy, upstream gradient) of one case.  The upstream gradient is random (not a loss's) and scaled as a mean loss's
    is, 1 / (B T), so that the parameter gradients have the magnitude the absolute bar of the plain-arbiter tests was set for."""
    _, n, ci, B, T = case[:5]
    noisy, _ = plan.golden_batch(B, T, BATCH_SEED)
    gout = np.random.Generator(np.random.PCG64(UPSTREAM_SEED)).standard_normal(size=noisy.shape) / (B * T)
    return plan.golden_state(n, ci, 0), noisy, gout.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ the device's side
def device_run(engine, device, case):
    """One training forward (saving) + backward + input gradient of `case` on `engine`, tensors on `device`.  Returns
    {"z": the raw conv output of every layer at its true length, "grads": {parameter name: gradient}, "input": dL/d(noisy),
     "launched": {kernel name: launches}}.  The caller has put the case's environment in place: a context is planned on first use."""
    _, n, ci, B, T, _, frozen, _ = case
    sd, noisy, gout = inputs(case)
    names = plan.param_names(n, ci)
    bnames = plan.buffer_names(n, ci)
    params = [torch.tensor(sd[k]).to(device) for k in names]
    running = [torch.tensor(sd[k]).to(device) for k in bnames if not k.endswith("num_batches_tracked")]
    nbt = [torch.tensor(int(sd[k]), dtype=torch.int64).to(device) for k in bnames if k.endswith("num_batches_tracked")]
    nl = 2 * n + 1
    mask = [i in frozen for i in range(nl)] if frozen else None
    x = torch.tensor(noisy).to(device)
    sync = torch.cuda.synchronize if x.is_cuda else (lambda: None)
    engine.lib.wunet_profile_enable(1)
    try:
        out, ws = engine.forward(n, ci, x, params, running, nbt, True, True, frozen=mask)
        sync()
        zs = []
        for i in range(nl):
            lt = T >> min(i, 2 * n - i)
            z = engine.layer_output(n, ci, B, T, ws, i)
            assert z.shape[-1] >= lt, (i, z.shape, lt)
            zs.append(z[..., :lt].cpu().numpy().copy())             # (rows padded to a power of two: their first Lt columns)
        grads = [torch.full_like(p, float("nan")) for p in params]
        engine.backward(n, ci, x, params, out, torch.tensor(gout).to(device), ws, grads, frozen=mask)
        gx = engine.backward_input(n, ci, x, params, ws)
        sync()
    finally:
        buf = ctypes.create_string_buffer(1 << 16)
        engine.lib.wunet_profile_collect(buf, len(buf))
        engine.lib.wunet_profile_enable(0)
    launched = {ln.split("\t")[0]: int(ln.split("\t")[1]) for ln in buf.value.decode().strip().splitlines()}
    return {"z": zs, "grads": {k: g.cpu().numpy() for k, g in zip(names, grads)}, "input": gx.cpu().numpy(), "launched": launched}


# ------------------------------------------------------------------------------------------------------------------ the arbiter
class _Substitute(torch.autograd.Function):
    """forward: the given tensor, exactly; backward: the gradient, unchanged, to the value it replaces."""

    @staticmethod
    def forward(ctx, z, given):
        return given.clone()

    @staticmethod
    def backward(ctx, grad):
        return grad, None


def linearised(case, zs, dtype, masks=None):
    """oracle/torch_port.forward (training=True) of `case` with every conv output replaced by zs[i], back-propagated from the case's
    upstream gradient.  masks: per layer, the boolean LeakyReLU mask to use (slope 1 where True) or None for y > 0.
    Returns (grads: {parameter name: gradient, "input": dL/d(noisy)}, layers: per layer (y, mask, threshold of ambiguity))."""
    _, n, ci, B, T, _, frozen, _ = case
    sd_np, noisy, gout = inputs(case)
    sd = torch_port.state_to_torch(sd_np, dtype=dtype, requires_grad=True)
    x = torch.as_tensor(noisy, dtype=dtype).requires_grad_(True)
    one, slope = torch.ones((), dtype=dtype), torch.tensor(torch_port.SLOPE, dtype=dtype)
    layers = []

    def conv_bn_act(h, i, prefix, taps):
        z = F.conv1d(h, sd[f"{prefix}.0.weight"], sd[f"{prefix}.0.bias"], padding=taps // 2)
        zd = torch.as_tensor(zs[i], dtype=dtype)
        assert zd.shape == z.shape, (prefix, zd.shape, z.shape)
        z = _Substitute.apply(z, zd)
        gamma, beta = sd[f"{prefix}.1.weight"], sd[f"{prefix}.1.bias"]
        if i in frozen:                                    # wunet_set_bn_frozen: the running statistics of the checkpoint
            mean, var = sd[f"{prefix}.1.running_mean"], sd[f"{prefix}.1.running_var"]
            y = F.batch_norm(z, mean, var, gamma, beta, False, torch_port.BN_MOMENTUM, torch_port.BN_EPS)
        else:
            y = F.batch_norm(z, None, None, gamma, beta, True, torch_port.BN_MOMENTUM, torch_port.BN_EPS)
            mean, var = zd.mean(dim=(0, 2)), zd.var(dim=(0, 2), unbiased=False)
        a = (gamma.detach() / torch.sqrt(var + torch_port.BN_EPS))[None, :, None]
        s = beta.detach()[None, :, None] - mean[None, :, None] * a
        mask = (y.detach() > 0) if masks is None or masks[i] is None else masks[i]
        layers.append((y.detach(), mask, AMBIGUOUS_ULPS * ((a * zd).abs() + s.abs())))
        return y * torch.where(mask, one, slope)

    convs = plan.conv_layers(n, ci)
    skips = []
    h = x
    for i in range(n):
        h = conv_bn_act(h, i, convs[i][0], convs[i][3])
        skips.append(h)
        h = h[:, :, ::2]
    h = conv_bn_act(h, n, convs[n][0], convs[n][3])
    for j in range(n):
        h = torch_port.upsample_fp32_coords(h) if dtype == torch.float64 else F.interpolate(h, scale_factor=2, mode="linear", align_corners=True)
        h = torch.cat([h, skips[n - 1 - j]], dim=1)
        h = conv_bn_act(h, n + 1 + j, convs[n + 1 + j][0], convs[n + 1 + j][3])
    h = torch.cat([h, x], dim=1)
    out = torch.tanh(F.conv1d(h, sd["out.0.weight"], sd["out.0.bias"]))
    out.backward(torch.as_tensor(gout, dtype=dtype))
    grads = {k: sd[k].grad.numpy() for k in plan.param_names(n, ci)}
    grads["input"] = x.grad.numpy()
    return grads, layers


def rel(got, want):
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-300))


def compared(case):
    """The tensors that are compared: every parameter gradient except the conv biases in front of a batch-statistics BatchNorm (their
    gradient is exactly 0 on the device: asserted apart), and the input gradient."""
    _, n, ci, _, _, _, frozen, _ = case
    keep = []
    for i, (prefix, _, _, _) in enumerate(plan.conv_layers(n, ci)):
        keep += [f"{prefix}.0.weight"] + ([f"{prefix}.0.bias"] if i in frozen else []) + [f"{prefix}.1.weight", f"{prefix}.1.bias"]
    return keep + ["out.0.weight", "out.0.bias", "input"]


def ambiguous_elements(layers):
    """[(layer, flat index)] of the activations whose slope fp32 and float64 may legitimately see differently."""
    found = []
    for i, (y, _, thr) in enumerate(layers):
        found += [(i, int(j)) for j in torch.nonzero((y.abs() <= thr).flatten()).flatten()]
    return found


def flipped(layers, elements):
    """The masks of `layers` with the slope of each (layer, flat index) of `elements` chosen the other way."""
    masks = [m for _, m, _ in layers]
    for i, j in elements:
        if masks[i] is layers[i][1]:
            masks[i] = masks[i].clone()
        masks[i].view(-1)[j] = ~masks[i].view(-1)[j]
    return masks


def arbiter(case, dev):
    """The float64 arbiter of `case` at the device's forward point dev["z"], its ambiguous slopes chosen as the device's gradients say.
    Returns (grads64, masks accepted, k, the elements flipped)."""
    got = dict(dev["grads"], input=dev["input"])
    keys = compared(case)
    g64, layers = linearised(case, dev["z"], torch.float64)
    amb = ambiguous_elements(layers)
    k = len(amb)
    assert k <= MAX_AMBIGUOUS, f"{case_id(case)}: {k} ambiguous LeakyReLU slopes (the rule allows {MAX_AMBIGUOUS}): {amb}"
    best = (sum(rel(got[t], g64[t]) ** 2 for t in keys), g64, [m for _, m, _ in layers], ())
    for r in range(1, k + 1):
        for choice in itertools.combinations(amb, r):
            masks = flipped(layers, choice)
            g, _ = linearised(case, dev["z"], torch.float64, masks)
            d = sum(rel(got[t], g[t]) ** 2 for t in keys)
            if d < best[0]:
                best = (d, g, masks, choice)
    return best[1], best[2], k, best[3]


def measure(case, dev):
    """Everything the assertions need: {"k", "choice", "d_ref", "rel": {tensor: device distance}, "abs": {tensor: largest difference},
    "worst": (tensor, distance)} - and the arbiter's gradients and masks, for the harness's self-check."""
    g64, masks, k, choice = arbiter(case, dev)
    g32, _ = linearised(case, dev["z"], torch.float32, masks)              # (the d_ref run uses the accepted mask)
    got = dict(dev["grads"], input=dev["input"])
    keys = compared(case)
    rels = {t: rel(got[t], g64[t]) for t in keys}
    worst = max(keys, key=lambda t: rels[t])
    return {"k": k, "choice": choice, "d_ref": max(rel(g32[t], g64[t]) for t in keys), "rel": rels,
            "abs": {t: float(np.abs(got[t].astype(np.float64) - g64[t]).max()) for t in keys}, "worst": (worst, rels[worst]),
            "g64": g64, "masks": masks}


def row(case, m, where):
    return (f"{where:8s} {case_id(case):44s} k={m['k']} flipped={list(m['choice'])} d_ref={m['d_ref']:.2e} "
            f"worst={m['worst'][1]:.2e} ({m['worst'][1] / m['d_ref']:.2f} x d_ref) {m['worst'][0]}")


def check(case, dev, where):
    """The assertions of one case (the same on the emulator and on the hardware).  Returns measure()'s record."""
    h3, n, ci, _, _, _, frozen, must_launch = case
    for prefix in must_launch:
        assert any(fnmatch.fnmatchcase(name, prefix + "*") for name in dev["launched"]), (prefix, sorted(dev["launched"]))
    assert sum(v for name, v in dev["launched"].items() if name.startswith("input_grad_kernel")) == 1, dev["launched"]
    for i, (prefix, _, _, _) in enumerate(plan.conv_layers(n, ci)):
        if i not in frozen:                              # exact zero in front of a batch-statistics BatchNorm
            assert np.all(dev["grads"][f"{prefix}.0.bias"] == 0.0), prefix
    for t, g in dict(dev["grads"], input=dev["input"]).items():
        assert np.isfinite(g).all(), t
    m = measure(case, dev)
    print(row(case, m, where))
    bar = MARGIN[h3] * m["d_ref"]
    for t in compared(case):
        print(f"    {t:28s} rel={m['rel'][t]:.2e} ({m['rel'][t] / m['d_ref']:.2f} x d_ref) abs={m['abs'][t]:.2e}")
    for t in compared(case):
        assert m["rel"][t] <= bar, (t, m["rel"][t], m["d_ref"], m["rel"][t] / m["d_ref"])
        assert m["abs"][t] < ABS_BAR, (t, m["abs"][t])
    return m
