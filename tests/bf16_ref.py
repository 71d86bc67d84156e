"""The host side of the exact checks of the bf16 GEMM mode (wunet_set_h3(ctx, 3 | 4); the wunet_op_*_bf16 entry points), shared by
tests/test_emu_bf16_ops.py (CPU emulator) and tests/test_gpu_bf16_ops.py (MI355X).

Why the comparison can be exact.  The mode stores every GEMM operand value as ONE bf16 word: round to nearest even (wunet_f2b) of
the value times a power-of-two scale (wunet_pow2_scale).  Scaling by a power of two is exact and commutes with the rounding, the
product of two bf16 values (8 x 8 significant bits) is exact in fp32, so what a correct kernel returns is the convolution of the
bf16-ROUNDED operands up to fp32 accumulation - the error of the fp16-split kernels, not the 2e-3 of bf16 itself.  round_bf16
restates the rounding on the host; the float64 conv of the rounded operands (oracle/wunet_oracle.c, f64 build) is the reference.

Plain data and helpers: which shapes, which operands, the reference and what was measured.  What is asserted at which bar is each
test module's own business."""
import functools

import numpy as np
import torch

import split_op_cases as C
from oracle import c_oracle, plan, torch_port


# ---------------------------------------------------------------------------------------------------------------------
# the rounding
def round_bf16(a):
    """float32 -> float32 holding bf16 values: the bit arithmetic of wunet_f2b (csrc/wunet_dev.h).  Round to nearest, ties to the
    even bf16 word; +-inf stay; a NaN keeps its sign and upper payload and gets the quiet bit (it must not round up into inf)."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) & 0xffff
    r = np.where(nan, (u >> 16) | 0x40, r)
    return (r << 16).astype(np.uint32).view(np.float32).reshape(a.shape)


def ulp_bf16(v):
    """Distance between the two bf16 neighbours of v (float64, elementwise; 0 at 0): 2^(exponent - 7)."""
    v = np.abs(np.asarray(v, np.float64))
    _, e = np.frexp(v)                       # v = m 2^e, m in [0.5, 1)
    return np.where(v > 0, np.ldexp(1.0, e - 8), 0.0)


def midpoint_distance(v):
    """|v - the midpoint of its two bf16 neighbours| (float64, elementwise): how far v is from rounding the other way."""
    v = np.abs(np.asarray(v, np.float64))
    u = ulp_bf16(v)
    lo = np.where(u > 0, np.floor(v / np.where(u > 0, u, 1.0)) * u, 0.0)
    return np.abs(v - (lo + 0.5 * u))


# ---------------------------------------------------------------------------------------------------------------------
# single ops: the cases, their operands and the reference
TIE_BASE = (2, 20, 24, 512, 5, 1e-4, 3e3)
TIE_CASE = TIE_BASE + ("ties",)


def _with_ties(a):
    """Every 97th entry replaced by an exact bf16 midpoint of its own magnitude: a bf16 value plus half its ulp (exact in fp32),
    the bf16 value's low bit alternately even and odd - round-to-nearest-even goes DOWN from the first kind and UP from the second,
    a kernel that rounds half up or truncates is one bf16 ulp (2^-8 .. 2^-7 relative) off on every other one."""
    a = a.copy()
    flat = a.reshape(-1)
    idx = np.arange(0, flat.size, 97)
    u = flat[idx].view(np.uint32) & np.uint32(0xffff0000)                      # the bf16 word below
    odd = (np.arange(idx.size) & 1).astype(np.uint32)
    u = (u & np.uint32(0xfffeffff)) | (odd << np.uint32(16))                   # low bit of the bf16 word: even, odd, even ...
    flat[idx] = (u | np.uint32(0x8000)).view(np.float32)                        # + half an ulp
    return a


# the layers of the 16-level net of bench.py's deep16_bf16 extra (65536 samples) whose rows are 16 .. 256 samples long: channel
# counts the table of tests/split_op_cases.py does not reach (192 .. 312 rows, up to 648 K channels; 27 .. 81 channel groups).
# Batch 4 where the entry points take it: they need B * L >= 256 (one whole tile), so the 32- and 16-sample levels run at the
# smallest batch that has one, 8 and 16.
def _deep16_cases():
    n, T, out = 16, 65536, []
    for i, (prefix, cin, cout, k) in enumerate(plan.conv_layers(n, 24)):
        L = T >> (i if i <= n else 2 * n - i)
        if 16 <= L <= 256:
            out.append((max(4, 256 // L), cin, cout, L, k, 1.0, 1.0))
    return out


DEEP16_CASES = _deep16_cases()


def case_id(case):
    return C.case_id(case) + ("-" + case[7] if len(case) > 7 else "")


@functools.lru_cache(maxsize=None)
def operands(case):
    """x, w, bias, gz of one case (float32, read-only): those of tests/split_op_cases.py as they are, or with the planted ties."""
    x, w, b, gz = C.operands(tuple(case[:7]))
    if len(case) > 7:
        x, w, gz = _with_ties(x), _with_ties(w), _with_ties(gz)
    return C._frozen(x, w, b, gz)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(z, dx, dw) of one case: the float64 conv of the bf16-rounded operands, the bias as it is (the epilogue adds it in fp32)."""
    x, w, b, gz = operands(case)
    xr, wr, gr = round_bf16(x), round_bf16(w), round_bf16(gz)
    z = c_oracle.conv1d_fwd(xr, wr, b)
    dx, dw, _ = c_oracle.conv1d_bwd(gr, xr, wr)
    return C._frozen(z, dx, dw)


# the cases whose bf16 run is planned differently from the fp16-split run of the same geometry (tests/test_emu_bf16_ops.py says why)
PLAN_DIVERGENCE = {"B16-288x312-L16-k15"}


def kernels_side_by_side(case, bf_names, split_names):
    """One line: the GEMM kernels (and the split-K reduce, named by its split count) of the bf16 and of the fp16-split run."""
    def gemm(names):
        return ", ".join(f"{k} x {v}" if v > 1 else k for k, v in sorted(names.items()) if k.startswith(("conv_h3", "wgrad_h3", "split_sum")))
    return f"{case_id(case)} bf16 [{gemm(bf_names)}] | split [{gemm(split_names)}]"


def _gemm_plan(names):
    return {k.replace(", bf16>", ">"): v for k, v in names.items() if k.startswith(("conv_h3", "wgrad_h3", "split_sum"))}


def plans_differ(bf_names, split_names):
    """Whether the two runs launched other kernels, other tilings or other split counts (the bf16 tag aside)."""
    return _gemm_plan(bf_names) != _gemm_plan(split_names)


def check_kernel_names(case, names, deep=False):
    """What must hold of the kernels one bf16 run of (conv, dgrad, wgrad) launched."""
    K, L = case[4], case[3]
    conv = [nm for nm in names if nm.startswith("conv_h3")]
    wg = [nm for nm in names if nm.startswith("wgrad_h3")]
    assert conv and sum(names[nm] for nm in conv) == 2, names              # (forward conv + data gradient)
    assert all("_kernel<%d," % K in nm and nm.endswith(", bf16>") for nm in conv + wg), names
    if L >= 256:
        assert all(nm.startswith("conv_h3d_kernel<") for nm in conv), names
    assert len(wg) == 1 and names[wg[0]] == 1, names
    if not deep:          # (the table's rule, which holds up to its 80 output channels: DMA-staged from 128 samples on)
        assert wg[0].startswith("wgrad_h3d_kernel<" if L >= 128 else "wgrad_h3_kernel<"), names


# ---------------------------------------------------------------------------------------------------------------------
# per-layer forward of a forced-bf16 engine, teacher-forced: every layer against a reference computed from the DEVICE's own
# previous raw conv output(s), so nothing compounds
NETS = C.NETS + [(3, 16, 3, 1024), (4, 16, 5, 1024)]
FLIP = 16.0 * 2.0 ** -24          # the fp32 slack of an activation, relative to |a z| + |s|


def _conv64(x, w, bias, K):
    import torch.nn.functional as F
    return F.conv1d(torch.from_numpy(x), torch.from_numpy(w), None if bias is None else torch.from_numpy(bias), padding=K // 2).numpy()


def _activation(z, sd, prefix, training):
    """float64 LeakyReLU(BatchNorm(z)) of a raw conv output z [B, C, Lt] and the slack delta of each value: FLIP (|a z| + |s|) for
    y = a z + s."""
    z = z.astype(np.float64)
    gamma, beta = sd[prefix + ".1.weight"].astype(np.float64), sd[prefix + ".1.bias"].astype(np.float64)
    if training:
        mean, var = z.mean(axis=(0, 2)), z.var(axis=(0, 2))
    else:
        mean, var = sd[prefix + ".1.running_mean"].astype(np.float64), sd[prefix + ".1.running_var"].astype(np.float64)
    a = gamma / np.sqrt(var + torch_port.BN_EPS)
    s = beta - a * mean
    az = a[None, :, None] * z
    y = az + s[None, :, None]
    return np.where(y >= 0, y, torch_port.SLOPE * y), FLIP * (np.abs(az) + np.abs(s)[None, :, None]), np.abs(y)


def _up(a):
    return torch_port.upsample_fp32_coords(torch.from_numpy(np.ascontiguousarray(a))).numpy()


def measure_layer_forward(engine, device, net, training):
    """One forward of `net` (weights plan.golden_state(n, ci, 0), batch plan.golden_batch(B, T, 5)) on a forced-bf16 engine.
    Returns a dict:
      first     error of layer 0 (conv_first_kernel, fp32) against the plain float64 conv, over max(1, max |ref|)
      layers    one record per layer i >= 1: prefix, outside (outputs beyond their tolerance), ratio (worst error / tolerance),
                share (outputs beyond the base part of the tolerance alone), tol (largest tolerance over the layer's scale),
                pad_exact (None, or whether the raw output behind the true row end of a padded row holds exactly the bias)
      head      error of the network output against tanh of the 1x1 conv of the device's last activation and the input
    Reference of layer i: float64 conv of round_bf16(input) with round_bf16(weight) and the fp32 bias, the input formed in float64
    from the device's raw output of the producing layer(s) - BatchNorm (batch statistics over the true length, or the running ones),
    LeakyReLU, decimation / upsampling at ATen's fp32 coordinates and the skip.  Tolerance of one output: 1e-5 max(1, max |ref|)
    plus, for the inputs that the device's fp32 activation may round to the OTHER bf16 neighbour (distance to the rounding midpoint
    <= delta), one bf16 ulp of the input times |round_bf16(weight)|: a float64 conv of the two."""
    n, ci, B, T = net
    noisy, _ = plan.golden_batch(B, T, 5)
    sd = plan.golden_state(n, ci, 0)
    params = [torch.tensor(sd[k]).to(device) for k in plan.param_names(n, ci)]
    bnames = plan.buffer_names(n, ci)
    running = [torch.tensor(sd[k]).to(device) for k in bnames if not k.endswith("num_batches_tracked")]
    nbt = [torch.tensor(int(sd[k]), dtype=torch.int64).to(device) for k in bnames if k.endswith("num_batches_tracked")]
    out, ws = engine.forward(n, ci, torch.tensor(noisy).to(device), params, running, nbt, training, False)
    if out.is_cuda:
        torch.cuda.synchronize()
    layers = plan.conv_layers(n, ci)
    raw = [engine.layer_output(n, ci, B, T, ws, i).cpu().numpy() for i in range(len(layers))]
    res = {"layers": []}
    acts = []                     # (activation, delta, |y|) of every layer at its true length
    for i, (prefix, cin, cout, K) in enumerate(layers):
        Lt = T >> (i if i <= n else 2 * n - i)
        z = raw[i]
        assert z.shape[:2] == (B, cout) and z.shape[-1] >= Lt and np.isfinite(z).all(), (prefix, z.shape)
        w, bias = sd[prefix + ".0.weight"], sd[prefix + ".0.bias"]
        if i == 0:
            ref = _conv64(noisy.astype(np.float64), w.astype(np.float64), bias.astype(np.float64), K)
            res["first"] = float(np.abs(z[..., :Lt] - ref).max()) / max(1.0, float(np.abs(ref).max()))
        else:
            if i <= n:            # encoder / middle: every second sample of the previous activation
                x, delta = acts[i - 1][0][..., ::2], acts[i - 1][1][..., ::2]
            else:                 # decoder: the upsampled previous activation | the skip
                h, dh, yh = acts[i - 1]
                sk, dsk, _ = acts[2 * n - i]
                x = np.concatenate([_up(h), sk], axis=1)
                delta = np.concatenate([_up(dh) + FLIP * _up(yh), dsk], axis=1)
            assert x.shape == (B, cin, Lt), (prefix, x.shape)
            wr = round_bf16(w).astype(np.float64)
            x32 = x.astype(np.float32)
            # (the fp32 value nearest the float64 activation is what gets rounded; its own rounding, 2^-24 |x|, is inside delta)
            ref = _conv64(round_bf16(x32).astype(np.float64), wr, bias.astype(np.float64), K)
            ambiguous = midpoint_distance(x) <= delta
            base = 1e-5 * max(1.0, float(np.abs(ref).max()))
            tol = base + _conv64(ambiguous * ulp_bf16(x), np.abs(wr), None, K)
            err = np.abs(z[..., :Lt] - ref)
            res["layers"].append({"prefix": prefix, "outside": int((err > tol).sum()), "ratio": float((err / tol).max()),
                                  "share": float((err > base).mean()), "tol": float(tol.max() / max(1.0, float(np.abs(ref).max()))),
                                  "pad_exact": None})
            if z.shape[-1] > Lt:
                assert z.shape[-1] - Lt > 2 * (K // 2)
                tail = z[..., Lt + K // 2:]
                res["layers"][-1]["pad_exact"] = bool(np.array_equal(tail, np.broadcast_to(bias[None, :, None], tail.shape)))
        acts.append(_activation(z[..., :Lt], sd, prefix, training))
    h = np.concatenate([acts[-1][0], noisy.astype(np.float64)], axis=1)
    ref_out = np.tanh(_conv64(h, sd["out.0.weight"].astype(np.float64), sd["out.0.bias"].astype(np.float64), 1))
    res["head"] = float(np.abs(out.detach().cpu().numpy() - ref_out).max())
    return res


def layer_forward_summary(res):
    """(largest count outside the tolerance, worst error / tolerance, largest share beyond the base part, largest tolerance)."""
    ls = res["layers"]
    return max(l["outside"] for l in ls), max(l["ratio"] for l in ls), max(l["share"] for l in ls), max(l["tol"] for l in ls)
