"""Drop-in replacement of the reference model plugin.

Select it from the reference's config exactly like any other plugin (util/utils.py:55-72):

    "model": {"module": "wave-u-net-for-speech-enhancement_amd.model", "main": "Model", "args": {}}

`Model(n_layers=12, channels_interval=24)` mirrors /root/reference/model/unet_basic.py:32-100:
same constructor, `forward(input[B,1,T]) -> [B,1,T]`, same 177 state_dict entries
(`encoder.{i}.main.0.weight`, `encoder.{i}.main.1.running_mean`, `middle.0.*`, `decoder.{i}.main.*`,
`out.0.*`), same default initialisation under the same seed (the parameter containers are created in
the reference's order), `.train()/.eval()` switching BatchNorm behaviour, `.to(device)/.cpu()`.  Like the reference's
nn.BatchNorm1d modules, each layer's BatchNorm obeys its own `.training` flag: a layer put in eval mode inside a training
model (frozen BatchNorm fine-tuning) normalises with its running statistics, leaves them untouched and back-propagates.
The arithmetic is not torch's: forward and backward run the hand-written gfx950 kernels behind the
C ABI of include/wunet_hip.h.  There is no CPU fallback: calling the module on a CPU tensor raises.
"""
import torch
import torch.nn as nn

from .engine import FlatGrads, bump_versions as _bump_versions, default_engine
from .plan import conv_layer_shapes


def _conv_bn(c_in, c_out, taps):
    # parameter containers only (their forward is never called): keys main.0.* / main.1.*
    return nn.Sequential(nn.Conv1d(c_in, c_out, kernel_size=taps, stride=1, padding=taps // 2),
                         nn.BatchNorm1d(c_out))


class _Level(nn.Module):
    """Holds `main.0` (conv) and `main.1` (batch norm) like the reference's Down/UpSamplingLayer."""

    def __init__(self, c_in, c_out, taps):
        super().__init__()
        self.main = _conv_bn(c_in, c_out, taps)


class _WaveUNetFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, owner, need_grad, noisy, *params):
        if noisy.requires_grad and not getattr(owner, "input_grad", False):     # before anything runs: a training-mode forward updates the running statistics
            raise NotImplementedError("gradient w.r.t. the waveform input is off by default (the training step needs none): build the "
                                      "model with Model(..., input_grad=True) or set model.input_grad = True, or detach the input")
        engine = owner._engine()
        running, nbt = owner._wunet_buffers()
        # Every BatchNorm module obeys its own .training flag.  None frozen: the training forward.  All frozen in an eval-mode model:
        # the eval forward (inference - enhancement.py's grad-enabled chunks - keeps its path and holds no backward workspace; a
        # backward runs the forward again first).  Any other mix: the training forward with the frozen layers on their running statistics.
        frozen = owner._bn_frozen()
        nfrozen = sum(frozen)
        training = nfrozen < len(frozen) or owner.training
        mask = frozen if (training and nfrozen) else None
        # (grad mode is off inside Function.forward and the engine only takes addresses: no detached copies of the 102 parameters)
        out, ws = engine.forward(owner.n_layers, owner.channels_interval, noisy, params, running, nbt,
                                 training, with_backward=need_grad and training, frozen=mask)
        if training and nfrozen < len(frozen):      # the kernels updated running statistics through raw pointers: tell the version counters
            _bump_versions(running + nbt)
        ctx.owner = owner
        ctx.training = training
        ctx.frozen = mask if training else frozen
        ctx.ws = ws if (need_grad and training) else None
        ctx.save_for_backward(noisy, out, *params)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        owner = ctx.owner
        if not ctx.training:
            # eval-mode forward: run it again as a saving training forward with every BatchNorm frozen (the same arithmetic on the
            # running statistics, which stay untouched), then back-propagate through that
            noisy, _, *params = ctx.saved_tensors
            running, nbt = owner._wunet_buffers()
            out, ws = owner._engine().forward(owner.n_layers, owner.channels_interval, noisy, params, running, nbt, True,
                                              with_backward=True, frozen=ctx.frozen)
            return _WaveUNetFn._backward(ctx, grad_out, noisy, out, params, ws)
        if ctx.ws is None:
            raise RuntimeError("backward through this forward has already run: its workspace (the saved activations) was "
                               "released; run the forward again (retain_graph=True cannot keep it)")
        noisy, out, *params = ctx.saved_tensors
        return _WaveUNetFn._backward(ctx, grad_out, noisy, out, params, ctx.ws)

    @staticmethod
    def _backward(ctx, grad_out, noisy, out, params, ws):
        owner = ctx.owner
        engine = owner._engine()
        sizes = [p.numel() for p in params]
        flat = torch.empty(sum(sizes), dtype=torch.float32, device=noisy.device)
        sync = owner.grad_sync
        # the kernels only need addresses (flat buffer + offsets): enqueue first, cut the 102 views autograd wants while the GPU runs
        offsets, off = [], 0
        for n in sizes:
            offsets.append(off)
            off += n
        fg = FlatGrads(flat, offsets)
        mask = ctx.frozen if any(ctx.frozen or ()) else None
        if sync is None:
            engine.backward(owner.n_layers, owner.channels_interval, noisy, params, out, grad_out.contiguous(), ws, fg, frozen=mask)
        else:
            sync.run(engine, owner, noisy, params, out, grad_out.contiguous(), ws, fg, flat, frozen=mask)
        # the input gradient: behind the backward's last range on this stream, from what it left in the workspace (each rank's own
        # input: not reduced, not scaled)
        gx = engine.backward_input(owner.n_layers, owner.channels_interval, noisy, params, ws) if ctx.needs_input_grad[2] else None
        grads = [g.view(p.shape) for g, p in zip(flat.split(sizes), params)]
        owner.last_flat_grad = flat
        ctx.ws = None
        return (None, None, gx, *grads)


class Model(nn.Module):
    def __init__(self, n_layers=12, channels_interval=24, input_grad=False):
        super().__init__()
        self.n_layers = n_layers
        self.channels_interval = channels_interval
        # an input that requires grad gets dL/d(input) (cascades, a trainable front end, attacks / saliency on a trained model); off:
        # such an input is refused, as the reference hot path never needs it
        self.input_grad = input_grad
        shapes = conv_layer_shapes(n_layers, channels_interval)
        enc, mid, dec = shapes[:n_layers], shapes[n_layers], shapes[n_layers + 1:]
        # construction order == reference order, so default init consumes the RNG identically
        self.encoder = nn.ModuleList([_Level(*s) for s in enc])
        self.middle = _conv_bn(*mid)
        self.decoder = nn.ModuleList([_Level(*s) for s in dec])
        self.out = nn.Sequential(nn.Conv1d(1 + channels_interval, 1, kernel_size=1, stride=1))
        self.grad_sync = None          # set by parallel.GradSync for RCCL data parallelism
        self.last_flat_grad = None     # flat fp32 gradient buffer of the latest backward
        self._engine_override = None

    # -- plumbing -------------------------------------------------------------------------------
    def _engine(self):
        return self._engine_override if self._engine_override is not None else default_engine()

    # The 102 parameters / 75 buffers in the C ABI's order, read through the modules' own dicts on every call (nothing cached: a
    # replaced sub-module or parameter is seen) - through nn.Module.__getattr__ and Sequential indexing the two lists cost the host
    # ~0.3 ms per forward, which a loop that synchronises every step (trainer/trainer.py:40) pays in full as GPU idle time.
    def _leaves(self):
        m = self._modules
        seqs = [lv._modules["main"]._modules for lv in m["encoder"]._modules.values()]
        seqs.append(m["middle"]._modules)
        seqs += [lv._modules["main"]._modules for lv in m["decoder"]._modules.values()]
        return [(q["0"], q["1"]) for q in seqs]

    @staticmethod
    def _param(mod, name):
        p = mod._parameters.get(name)
        return p if p is not None else getattr(mod, name)         # (nn.DataParallel replicas keep plain tensors as attributes)

    def _wunet_params(self):
        ps, P = [], self._param
        for conv, bn in self._leaves():
            ps += [P(conv, "weight"), P(conv, "bias"), P(bn, "weight"), P(bn, "bias")]
        head = self._modules["out"]._modules["0"]
        ps += [P(head, "weight"), P(head, "bias")]
        return ps

    def _bn_frozen(self):
        """Per conv layer (the C ABI's order): True where its BatchNorm module is in eval mode - what nn.BatchNorm1d obeys."""
        return tuple(not bn.training for _, bn in self._leaves())

    def _wunet_buffers(self):
        running, nbt = [], []
        for _, bn in self._leaves():
            b = bn._buffers
            running += [b["running_mean"], b["running_var"]]
            nbt.append(b["num_batches_tracked"])
        return running, nbt

    def forward(self, input):
        if input.dtype != torch.float32:
            raise TypeError(f"Model expects float32 waveforms, got {input.dtype}")
        params = self._wunet_params()
        need_grad = torch.is_grad_enabled() and ((getattr(self, "input_grad", False) and input.requires_grad) or any(p.requires_grad for p in params))
        return _WaveUNetFn.apply(self, need_grad, input.contiguous(), *params)
