"""fused Adam for the hot loop.

Drop-in for the optimiser the reference builds in train.py:31-35
(`torch.optim.Adam(params=model.parameters(), lr=..., betas=(beta1, beta2))`): same constructor arguments the
reference uses, same update rule and operation order as torch's single-tensor path (eps=1e-8, weight_decay=0,
amsgrad=False), same `state_dict()` layout ("step", "exp_avg", "exp_avg_sq" per parameter; param_groups carry every key
torch.optim.Adam's do) so the reference's checkpoints (trainer/base_trainer.py:62-124) load both ways - but one or two HIP
launches over all 102 tensors instead of ~10 multi-tensor ATen kernels.

`grad_scale` (attribute): every gradient is multiplied by it inside the step - the 1/world_size of the data-parallel average
(parallel.GradSync(scale_in_optimizer=True)).
`device_step=True`: the step counter lives on the device (incremented by the step's own kernel, bias corrections computed there
in double), so forward + loss + backward + step can be captured in one hipGraph and replayed (trainer.Trainer(graph=True));
the host-side `state["step"]` is kept in step by `advance_host_step()` after every replay.

Opt-in, no reference counterpart (with all of them off the step enqueues exactly the launches above; with any of them on, the same
two kernels - adam_hyper_kernel, adam_kernel of csrc/wunet_adam.h - with the optional slots of the hyper buffer in use):
`max_grad_norm=<float>`: clipping by the global 2-norm inside the step, the arithmetic of
`torch.nn.utils.clip_grad_norm_(params, max_grad_norm)` in front of `step()` - one extra read of the gradients (summed in double),
the factor min(1, max_grad_norm / (norm + 1e-6)) multiplies every gradient inside the update.  `p.grad` is NOT modified
(clip_grad_norm_ scales it in place; the fused step does not pay that write): code that reads the gradients after the step sees
them unclipped.  `last_grad_norm` is the norm before clipping as a device scalar; reading it is the caller's synchronisation.
`device_lr=True`: the learning rate is read from device memory, so a captured step replays unchanged under a per-step schedule:
`sync_device_hyper()` uploads a changed `group["lr"]` (the eager `step()` calls it itself; a graph driver calls it before
`replay()`, trainer.Trainer does).
`FusedAdamW`: decoupled weight decay, `torch.optim.AdamW`'s update and state_dict layout.
"""
import torch

from .engine import ADAM_HYPER_FLOATS, bump_versions as _bump_versions, default_engine

_ADAM_DEFAULTS = dict(weight_decay=0, amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False,
                      fused=None, decoupled_weight_decay=False)


class FusedAdam(torch.optim.Optimizer):
    _decoupled_weight_decay = False          # FusedAdamW: group["weight_decay"] is applied (decoupled)

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, device_step=False, max_grad_norm=None, device_lr=False,
                 _defaults=None):
        if lr < 0.0 or eps < 0.0 or not (0.0 <= betas[0] < 1.0) or not (0.0 <= betas[1] < 1.0):
            raise ValueError("invalid Adam hyper-parameters")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 or None (got {max_grad_norm})")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, **(_ADAM_DEFAULTS if _defaults is None else _defaults)))
        self._engine_override = None
        self.grad_scale = 1.0
        self.device_step = device_step
        self.max_grad_norm = max_grad_norm       # attributes, not param_groups keys: the groups keep torch.optim.Adam's keys
        self.device_lr = bool(device_lr)
        # group index -> (int64 step counter, hyper buffer of ADAM_HYPER_FLOATS floats[, float64 lr, partial sums of the norm]) on the
        # parameters' device; the last two exist once max_grad_norm / device_lr / a weight decay is in use
        self._dev = {}
        self._live_counter = {}   # group index -> the counter tensor a device_step step seeded and has kept counting since
        self._lr_written = {}     # group index -> (the device lr tensor, the value it holds)

    def hyper_signature(self):
        """Everything a captured step() bakes into its kernel arguments (lr, betas, eps, weight_decay per group, grad_scale,
        max_grad_norm): a driver that replays a graph compares it with the signature at capture time and re-captures when it changed
        (trainer.Trainer._step).  With device_lr the lr is NOT part of it: the captured step reads it from device memory."""
        return tuple((None if self.device_lr else g["lr"], tuple(g["betas"]), g["eps"], g.get("weight_decay", 0))
                     for g in self.param_groups) + (self.grad_scale, self.max_grad_norm, self.device_lr)

    @property
    def last_grad_norm(self):
        """The 2-norm of all gradients of the last step before clipping, with grad_scale applied (the norm of the AVERAGED gradient
        in a data-parallel job): a 0-dim view of the device hyper buffer that every step - eager or replayed - overwrites, None
        before the first step or without max_grad_norm.  Reading its value is the caller's synchronisation."""
        dev = self._dev.get(0)
        return dev[1][3] if self.max_grad_norm is not None and dev is not None and len(dev) > 2 else None

    def sync_device_hyper(self):
        """device_lr: bring the device copy of every group's lr up to date with group["lr"] - one 8-byte write per changed group,
        enqueued on the current stream like a kernel (no host memory is read later), nothing when no lr changed.  Never inside a
        capture (a write captured there would be replayed with the old value): the captured step() skips it and the driver calls
        this before replay().  The buffers are created and seeded by the first eager step()."""
        if not self.device_lr:
            return
        for gi, group in enumerate(self.param_groups):
            dev = self._dev.get(gi)
            if dev is None or len(dev) < 3:
                continue
            lr_dev, lr = dev[2], float(group["lr"])
            w = self._lr_written.get(gi)
            if w is not None and w[0] is lr_dev and w[1] == lr:
                continue
            if lr_dev.is_cuda and torch.cuda.is_current_stream_capturing():
                continue
            lr_dev.fill_(lr)
            self._lr_written[gi] = (lr_dev, lr)

    def _device_buffers(self, gi, step, n_tensors, device, lr, ex):
        """The group's device-side scalars (see _dev), created on first use - outside any capture: the first eager step does it."""
        dev = self._dev.get(gi)
        live = dev is not None and self._live_counter.get(gi) is dev[0]
        if dev is None or (self.device_step and not live):
            # (a counter nobody incremented - steps counted on the host in between - starts again from the host's count)
            dev = (torch.full((), step - 1, dtype=torch.int64, device=device),
                   dev[1] if dev is not None else torch.zeros(ADAM_HYPER_FLOATS, dtype=torch.float32, device=device)) + (dev or ())[2:]
        if self.device_step:
            self._live_counter[gi] = dev[0]
        else:
            self._live_counter.pop(gi, None)
        if ex:
            n_part = max(self._engine().adam_scratch_bytes(n_tensors) // 8, 1) if self.max_grad_norm is not None else 1
            if len(dev) < 4 or dev[3].numel() < n_part:
                lr_dev = dev[2] if len(dev) > 2 else torch.full((), float(lr), dtype=torch.float64, device=device)
                if len(dev) <= 2:
                    self._lr_written[gi] = (lr_dev, float(lr))
                dev = dev[:2] + (lr_dev, torch.empty(n_part, dtype=torch.float64, device=device))
        self._dev[gi] = dev
        return dev

    def _engine(self):
        return self._engine_override if self._engine_override is not None else default_engine()

    def state_dict(self):
        """torch.optim.Adam's layout, with a "step" tensor of ITS OWN per parameter (inside this class the parameters of a group
        share one counter object, see step(): an optimiser that increments per parameter - torch.optim.Adam after loading this
        checkpoint, trainer/base_trainer.py:74 - must not see them aliased)."""
        sd = super().state_dict()
        sd["state"] = {k: ({**v, "step": v["step"].clone()} if "step" in v else v) for k, v in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        for g in state_dict["param_groups"]:
            if (not self._decoupled_weight_decay and g.get("weight_decay", 0) != 0) or g.get("amsgrad", False) or g.get("maximize", False):
                raise ValueError("FusedAdam implements the reference's Adam (train.py:31-35: weight_decay=0, amsgrad=False, "
                                 "maximize=False); the checkpoint asks for something else"
                                 + (" (FusedAdamW takes a decoupled weight_decay)" if not self._decoupled_weight_decay else ""))
        super().load_state_dict(state_dict)
        for g in self.param_groups:
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        # "step" as this class keeps it: a float32 scalar on the HOST.  A checkpoint loaded with map_location=<gpu>
        # (trainer.Trainer._resume_checkpoint, the reference's base_trainer.py:70-74) leaves it on the device - step() would then
        # synchronise once per parameter and abort a graph capture - and the torch 1.2 the reference was tested with stored a
        # Python int (README.md:27).
        for st in self.state.values():
            if "step" in st:
                v = st["step"]
                st["step"] = torch.tensor(float(v.item() if torch.is_tensor(v) else v), dtype=torch.float32, device="cpu")
        self._dev = {}            # re-seeded from the loaded host step (and lr) at the next step()

    def advance_host_step(self, n=1):
        """After replaying a captured graph that contains step(): the device counter advanced, bring state["step"] along."""
        seen = {}
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st:
                    seen[id(st["step"])] = st["step"]           # (the parameters of a group share one counter object, see step())
        for t in seen.values():
            t += n
        # the replay rewrote the weights on the device; no Python version counter moved (engine.py: the eval weight-pack cache)
        self._engine().note_weights_changed()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            ps, gs, ms, vs, steps, skipped = [], [], [], [], [], []
            state = self.state
            for p in group["params"]:
                g = p.grad
                if g is None:
                    skipped.append(p)
                    continue
                st = state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)      # host scalar, like torch's default
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                ps.append(p); gs.append(g if g.is_contiguous() else g.contiguous())
                ms.append(st["exp_avg"]); vs.append(st["exp_avg_sq"]); steps.append(st["step"])
            if not ps:
                continue
            # The host-side step counters.  torch.optim.Adam's layout wants one "step" tensor per parameter; 102 scalar `+= 1`
            # (or one _foreach_add_ over 102 CPU scalars) cost the host 0.2 - 0.3 ms per step, so parameters whose counts agree
            # share ONE tensor object (state_dict() and checkpoints look the same: the value per key).
            s0 = steps[0]
            for p in skipped:               # a parameter without a gradient does not step (torch.optim.Adam): it leaves the shared counter
                st = state.get(p)
                if st and st.get("step") is s0:
                    st["step"] = s0.clone()
            if all(t is s0 for t in steps):
                s0 += 1
                launches = [(int(s0.item()), ps, gs, ms, vs)]
            else:
                # counts that differ (a parameter that sat out some steps, a checkpoint just loaded): one launch per distinct count -
                # a launch has one bias correction - and one shared counter per such sub-group from here on
                by = {}
                for k, t in enumerate(steps):
                    by.setdefault(float(t.item()), []).append(k)
                if self.device_step and len(by) != 1:
                    # (checked BEFORE any counter is rewritten: a caller that catches this finds host counters, device counter and
                    # moments as they were)
                    raise RuntimeError("FusedAdam(device_step=True): the parameters of one group must share the step count "
                                       "(the group has ONE counter on the device)")
                launches = []
                for v, idx in by.items():
                    sv = torch.tensor(v + 1.0, dtype=torch.float32)
                    for k in idx:
                        state[ps[k]]["step"] = sv
                    launches.append((int(v) + 1, [ps[k] for k in idx], [gs[k] for k in idx], [ms[k] for k in idx], [vs[k] for k in idx]))
            b1, b2 = group["betas"]
            wd = float(group["weight_decay"]) if self._decoupled_weight_decay else 0.0
            ex = self.max_grad_norm is not None or self.device_lr or wd != 0.0
            if self.max_grad_norm is not None and (len(launches) != 1 or len(self.param_groups) != 1):
                raise RuntimeError("FusedAdam(max_grad_norm=...): ONE norm over all gradients needs one param group whose parameters "
                                   "share the step count (per-group clipping is not implemented)")
            step_dev = hyper_dev = None
            options = {}
            if self.device_step and len(launches) != 1:
                raise RuntimeError("FusedAdam(device_step=True): the parameters of one group must share the step count "
                                   "(the group has ONE counter on the device)")
            if self.device_step or ex:
                # (outside any capture: the first eager step creates and seeds the buffers)
                dev = self._device_buffers(gi, launches[0][0], max(len(l[1]) for l in launches), ps[0].device, group["lr"], ex)
                hyper_dev = dev[1]
                if self.device_step:
                    step_dev = dev[0]
                if ex:
                    options = dict(weight_decay=wd, max_grad_norm=self.max_grad_norm, lr_dev=dev[2] if self.device_lr else None,
                                   scratch=dev[3])
                    if self.device_lr:
                        self.sync_device_hyper()
            for step, lp, lg, lm, lv in launches:
                self._engine().adam_step(lp, lg, lm, lv, group["lr"], b1, b2, group["eps"], step, self.grad_scale, step_dev, hyper_dev,
                                         **options)
                # the kernel wrote p, exp_avg and exp_avg_sq through raw pointers: tell autograd's version counters, as every in-place
                # torch op would (a graph that saved a parameter and is back-propagated after this step must fail loudly, and anything
                # keyed on `_version` must see the change)
                _bump_versions(lp + lm + lv)
        return loss


class FusedAdamW(FusedAdam):
    """`torch.optim.AdamW(params, lr, betas, eps, weight_decay)` as one fused step: p <- p * (1 - lr * weight_decay) in front of
    FusedAdam's update, in torch's order.  Same param_groups keys and state_dict layout as torch.optim.AdamW (checkpoints load both
    ways); amsgrad and maximize are refused.  Takes FusedAdam's options (device_step, max_grad_norm, device_lr)."""
    _decoupled_weight_decay = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False,
                 device_step=False, max_grad_norm=None, device_lr=False):
        if amsgrad or maximize:
            raise ValueError("FusedAdamW implements torch.optim.AdamW with amsgrad=False and maximize=False")
        if weight_decay < 0.0:
            raise ValueError(f"invalid weight_decay {weight_decay}")
        # the keys (and untouched defaults) of this torch's AdamW, whatever they are
        ref = torch.optim.AdamW([torch.zeros(1)], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay).defaults
        defaults = {k: v for k, v in ref.items() if k not in ("lr", "betas", "eps")}
        super().__init__(params, lr=lr, betas=betas, eps=eps, device_step=device_step, max_grad_norm=max_grad_norm,
                         device_lr=device_lr, _defaults=defaults)
