"""TEST INFRASTRUCTURE ONLY.  The float64 arbiter of the frozen-BatchNorm tests: oracle/torch_port.forward with autograd, each
layer's BatchNorm in the mode a per-prefix set picks (nn.BatchNorm1d obeys its own .training flag).  oracle/ stays as it is: the
per-layer mode comes from a wrapper around torch_port._conv_bn_act that is patched in for the duration of one call."""
import contextlib

import numpy as np
import torch

from oracle import plan, torch_port


@contextlib.contextmanager
def frozen_layers(frozen_prefixes):
    """torch_port.forward(..., training=True) with the layers named in `frozen_prefixes` on their running statistics."""
    orig = torch_port._conv_bn_act
    frozen_prefixes = frozenset(frozen_prefixes)

    def conv_bn_act(x, sd, prefix, taps, training):
        return orig(x, sd, prefix, taps, training and prefix not in frozen_prefixes)

    torch_port._conv_bn_act = conv_bn_act
    try:
        yield
    finally:
        torch_port._conv_bn_act = orig


def prefixes(n, ci):
    """Conv layer prefixes in the C ABI's layer order (encoder, middle, decoder)."""
    return [p for p, _, _, _ in plan.conv_layers(n, ci)]


def run(sd_np, noisy, clean, n, ci, loss, frozen_mask, training=True, dtype=torch.float64, bf16_autocast=False):
    """Forward + loss + backward on the CPU (float64: the arbiter; float32 / float32 under bf16 autocast: the reference's own
    arithmetics).  frozen_mask: one bool per conv layer.  Returns (out, loss, grads by name, state after)."""
    sd = torch_port.state_to_torch(sd_np, dtype=dtype, requires_grad=True)
    pre = prefixes(n, ci)
    x = torch.as_tensor(np.asarray(noisy), dtype=dtype)
    y = torch.as_tensor(np.asarray(clean), dtype=dtype)
    with frozen_layers([p for p, f in zip(pre, frozen_mask) if f]), \
            torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16_autocast):
        out = torch_port.forward(sd, x, n, ci, training=training)
        lv = torch_port.loss_value(loss, y, out)
    lv.backward()
    grads = {k: v.grad.detach().float().numpy() if bf16_autocast else v.grad.detach().numpy() for k, v in sd.items() if v.requires_grad}
    state = {k: v.detach().numpy() for k, v in sd.items()}
    return out.detach().float().numpy() if bf16_autocast else out.detach().numpy(), lv.item(), grads, state


def set_bn_modes(model, frozen_mask):
    """Put each layer's BatchNorm module in eval mode where the mask says so (train mode elsewhere)."""
    for (_, bn), f in zip(model._leaves(), frozen_mask):
        bn.train(not f)


def masks(n):
    """The masks the tests run: encoder frozen with the rest on batch statistics, every other layer frozen."""
    nl = 2 * n + 1
    return {"enc": [i < n for i in range(nl)], "alt": [i % 2 == 0 for i in range(nl)]}
