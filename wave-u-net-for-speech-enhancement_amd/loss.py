"""Loss plugins, same factory convention as the reference (/root/reference/model/loss.py:3-7):
zero-argument factories returning a module called as `loss(clean, enhanced)`
(trainer/trainer.py:36 - the prediction is the second argument).

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "mse_loss", "args": {}}

`smooth_l1_loss` (torch.nn.SmoothL1Loss semantics, beta = 1) is the loss BASELINE.json's config 3
names; the reference only mentions it in its README.

`si_sdr_loss` / `snr_loss` (no reference counterpart): the negative mean over the utterances of the batch of the scale-invariant
SDR / the SNR in dB, each row of the last dimension on its own (include/wunet_hip.h: wunet_loss_rows_*):

    "loss_function": {"module": "wave-u-net-for-speech-enhancement_amd.loss", "main": "si_sdr_loss", "args": {}}
"""
import torch
import torch.nn as nn

from .engine import default_engine


class _LossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, engine, clean, enhanced):
        clean_c, enh_c = clean.detach().contiguous(), enhanced.detach().contiguous()
        ctx.kind, ctx.engine = kind, engine
        ctx.save_for_backward(clean_c, enh_c)
        return engine.loss_forward(kind, clean_c, enh_c)

    @staticmethod
    def backward(ctx, grad_loss):
        clean, enh = ctx.saved_tensors
        g = ctx.engine.loss_backward(ctx.kind, clean, enh, grad_loss)
        g_clean = -g if ctx.needs_input_grad[2] else None
        return None, None, g_clean, (g if ctx.needs_input_grad[3] else None)


class HipLoss(nn.Module):
    def __init__(self, kind):
        super().__init__()
        self.kind = kind
        self._engine_override = None

    def forward(self, clean, enhanced):
        engine = self._engine_override if self._engine_override is not None else default_engine()
        return _LossFn.apply(self.kind, engine, clean, enhanced)


def mse_loss():
    return HipLoss("mse")


def l1_loss():
    return HipLoss("l1")


def smooth_l1_loss():
    return HipLoss("smooth_l1")


class _RowLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, zero_mean, eps, engine, clean, enhanced):
        if clean.requires_grad:                 # (before anything runs)
            raise NotImplementedError(f"{kind}_loss: no gradient with respect to `clean` (the target also sets the signal energy, so it is "
                                      "not minus the gradient of `enhanced` as for the element-wise losses): detach it")
        clean_c, enh_c = clean.detach().contiguous(), enhanced.detach().contiguous()
        loss, coefs, _ = engine.loss_rows_forward(kind, clean_c, enh_c, zero_mean, eps)
        ctx.kind, ctx.engine = kind, engine
        ctx.save_for_backward(clean_c, enh_c, coefs)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        clean, enh, coefs = ctx.saved_tensors
        g = ctx.engine.loss_rows_backward(ctx.kind, clean, enh, coefs, grad_loss) if ctx.needs_input_grad[5] else None
        return None, None, None, None, None, g


class HipRowLoss(nn.Module):
    """loss(clean, enhanced) -> -mean over rows of si_sdr / snr [dB]; the last dimension is the utterance."""

    def __init__(self, kind, zero_mean=True, eps=1e-8):
        super().__init__()
        if not (eps >= 0.0 and eps < float("inf")):
            raise ValueError(f"{kind}_loss: eps must be finite and >= 0 (got {eps})")
        self.kind, self.zero_mean, self.eps = kind, bool(zero_mean), float(eps)
        self._engine_override = None

    def forward(self, clean, enhanced):
        engine = self._engine_override if self._engine_override is not None else default_engine()
        return _RowLossFn.apply(self.kind, self.zero_mean, self.eps, engine, clean, enhanced)


def si_sdr_loss(zero_mean=True, eps=1e-8):
    return HipRowLoss("si_sdr", zero_mean, eps)


def snr_loss(zero_mean=True, eps=1e-8):
    return HipRowLoss("snr", zero_mean, eps)
