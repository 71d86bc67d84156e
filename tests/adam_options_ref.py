"""TEST INFRASTRUCTURE ONLY.  Shared by tests/test_adam_options_emu.py (CPU emulator) and tests/test_gpu_adam_options.py (MI355X):
the cases of the fused Adam step's options (gradient clipping by global norm, decoupled weight decay, device-side lr), a float64
restatement of `torch.nn.utils.clip_grad_norm_` + `torch.optim.Adam` / `AdamW` in torch's operation order - the yardstick - and
torch's own fp32 pair, printed for information only (its norm is accumulated in fp32)."""
import functools
import math

import torch

STEPS = 4
MAX_NORM = 5.0
LRS = (1e-3, 7e-4, 1.3e-3, 5e-4)                  # the lr changes every step
BETAS = (0.9, 0.999)
EPS = 1e-8
WEIGHT_DECAY = 0.01

# every way the kernels can go wrong: one element, less than a wave, odd sizes, more than one block, and one tensor past the
# 256-block cap of the grid with a grid-stride tail
SHAPES_MIXED = ((1,), (7,), (33,), (7, 3, 15), (300,), (256 * 1024 + 5,))
# 70 tensors of 5 - 40 elements: more than WUNET_ADAM_MAX = 64, so two table launches - the second launch's partial sums sit behind
# the first's
SHAPES_MANY = tuple((5 + (11 * k) % 36,) for k in range(70))
CASES = {"mixed": SHAPES_MIXED, "many": SHAPES_MANY}


@functools.lru_cache(maxsize=None)
def initial(case):
    g = torch.Generator().manual_seed(100 + len(CASES[case]))
    return tuple(torch.randn(s, generator=g) for s in CASES[case])


@functools.lru_cache(maxsize=None)
def gradients(case):
    """Per step, one tensor per parameter: magnitudes 10^(it - 2), so that some steps clip at MAX_NORM and some do not."""
    out = []
    for it in range(STEPS):
        g = torch.Generator().manual_seed(200 + it)
        out.append(tuple(torch.randn(s, generator=g) * (10.0 ** (it - 2)) for s in CASES[case]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(case, decoupled, max_norm=MAX_NORM, grad_scale=1.0):
    """float64: clip as clip_grad_norm_ (norm of the scaled gradients, coefficient max_norm / (norm + 1e-6) clamped to 1), then
    Adam / AdamW in torch's single-tensor order.  Returns (params, exp_avg, exp_avg_sq, norms, clipped flags)."""
    p = [t.double().clone() for t in initial(case)]
    m = [torch.zeros_like(t) for t in p]
    v = [torch.zeros_like(t) for t in p]
    b1, b2 = BETAS
    norms, clipped = [], []
    for it in range(STEPS):
        lr, t = LRS[it], it + 1
        gs = [g.double() * grad_scale for g in gradients(case)[it]]
        coef = 1.0
        if max_norm is not None:
            norm = math.sqrt(sum(float((g * g).sum()) for g in gs))
            coef = min(1.0, max_norm / (norm + 1e-6))
            norms.append(norm)
            clipped.append(coef < 1.0)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for k, g in enumerate(gs):
            g = g * coef
            if decoupled:
                p[k] = p[k] * (1.0 - lr * WEIGHT_DECAY)
            m[k] = m[k] + (1.0 - b1) * (g - m[k])
            v[k] = v[k] * b2 + (1.0 - b2) * g * g
            denom = v[k].sqrt() / math.sqrt(bc2) + EPS
            p[k] = p[k] - (lr / bc1) * (m[k] / denom)
    return p, m, v, norms, clipped


@functools.lru_cache(maxsize=None)
def torch_fp32(case, decoupled):
    """torch's own fp32 clip_grad_norm_ + Adam / AdamW on the CPU (for information: its norm is an fp32 accumulation)."""
    p = [torch.nn.Parameter(t.clone()) for t in initial(case)]
    opt = (torch.optim.AdamW(p, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY) if decoupled
           else torch.optim.Adam(p, lr=LRS[0], betas=BETAS, eps=EPS))
    norms = []
    for it in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = LRS[it]
        for q, g in zip(p, gradients(case)[it]):
            q.grad = g.clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_(p, MAX_NORM)))
        opt.step()
    return ([q.detach() for q in p], [opt.state[q]["exp_avg"] for q in p], [opt.state[q]["exp_avg_sq"] for q in p], norms)


def run_fused(optim_mod, case, *, decoupled=False, max_grad_norm=MAX_NORM, device_lr=False, device_step=False, grad_scale=1.0,
              prescale=1.0, engine=None, device="cpu", want_norms=True):
    """STEPS steps of FusedAdam / FusedAdamW on `device` with the case's gradients (multiplied by `prescale` beforehand) and lrs.
    Returns (params, exp_avg, exp_avg_sq, norms) as CPU tensors / floats, and the optimiser."""
    p = [torch.nn.Parameter(t.clone().to(device)) for t in initial(case)]
    kw = dict(lr=LRS[0], betas=BETAS, eps=EPS, device_step=device_step, max_grad_norm=max_grad_norm, device_lr=device_lr)
    opt = optim_mod.FusedAdamW(p, weight_decay=WEIGHT_DECAY, **kw) if decoupled else optim_mod.FusedAdam(p, **kw)
    if engine is not None:
        opt._engine_override = engine
    opt.grad_scale = grad_scale
    norms = []
    for it in range(STEPS):
        for g in opt.param_groups:
            g["lr"] = LRS[it]
        given = []
        for q, g in zip(p, gradients(case)[it]):
            q.grad = (g * prescale).to(device)
            given.append(q.grad.clone())
        opt.step()
        for q, g in zip(p, given):
            assert torch.equal(q.grad, g), "the fused step must not modify p.grad"
        if max_grad_norm is not None and want_norms:
            norms.append(float(opt.last_grad_norm))                    # (the read is the synchronisation)
    out = ([q.detach().cpu() for q in p], [opt.state[q]["exp_avg"].cpu() for q in p], [opt.state[q]["exp_avg_sq"].cpu() for q in p], norms)
    return out, opt


SENTINEL = -123.0                                  # finite: slots compare with ==


def check_hyper_buffer_bounds(lib, device="cpu", stream=None):
    """The two C entry points share their kernels; their hyper buffers differ: wunet_adam_step documents 2 floats (or none), wunet_adam_step_ex
    WUNET_ADAM_HYPER_FLOATS = 8 of which 5 are used.  One tensor of 7 elements, an 8-float buffer pre-filled with SENTINEL per call: the
    plain entry with a device counter writes slots 0 and 1 only and increments the counter by one; without a counter it takes a NULL
    hyper pointer; the _ex entry with everything off writes clip = 1, norm = 0 and decay = 1 to slots 2..4 and nothing behind them."""
    import ctypes
    g = torch.Generator().manual_seed(7)
    arr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())                 # noqa: E731
    numels = (ctypes.c_size_t * 1)(7)

    def fresh():
        ts = [torch.randn(7, generator=g).to(device), torch.randn(7, generator=g).to(device), torch.zeros(7, device=device), torch.zeros(7, device=device)]
        return ts, torch.full((8,), SENTINEL, device=device), torch.full((), 4, dtype=torch.int64, device=device)

    def done(rc, p0, ts):
        assert rc == 0, lib.wunet_last_error()
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize()
        assert torch.isfinite(ts[0]).all() and not torch.equal(ts[0], p0) and ts[2].any() and ts[3].any()      # the step ran

    hp = (1e-3, 0.9, 0.999, 1e-8)
    # wunet_adam_step, device counter
    ts, hyper, counter = fresh()
    p0 = ts[0].clone()
    done(lib.wunet_adam_step(1, *(arr(t) for t in ts), numels, *hp, 1, 1.0, counter.data_ptr(), hyper.data_ptr(), stream), p0, ts)
    h = hyper.cpu()
    assert int(counter) == 5
    assert (h[2:] == SENTINEL).all(), h
    want = (1e-3 / (1.0 - 0.9 ** 5), math.sqrt(1.0 - 0.999 ** 5))      # (doubles rounded to float once: 2^-24, and an ulp of pow)
    assert all(abs(float(h[k]) - want[k]) <= 1.2e-7 * want[k] for k in range(2)), h
    # wunet_adam_step, host step: no hyper buffer at all
    ts, hyper, counter = fresh()
    p0 = ts[0].clone()
    done(lib.wunet_adam_step(1, *(arr(t) for t in ts), numels, *hp, 5, 1.0, None, None, stream), p0, ts)
    assert int(counter) == 4 and (hyper.cpu() == SENTINEL).all()
    # wunet_adam_step_ex, every option off
    ts, hyper, counter = fresh()
    p0 = ts[0].clone()
    done(lib.wunet_adam_step_ex(1, *(arr(t) for t in ts), numels, *hp, 1, 1.0, 0.0, 0.0, counter.data_ptr(), hyper.data_ptr(), None, None, stream), p0, ts)
    h = hyper.cpu()
    assert int(counter) == 5
    assert (h[5:] == SENTINEL).all(), h
    assert h[2] == 1.0 and h[3] == 0.0 and h[4] == 1.0 and h[0] != SENTINEL and h[1] != SENTINEL, h


def distances(got, ref):
    """(norm: worst relative distance; exp_avg, exp_avg_sq: worst distance as a fraction of the tensor's largest reference value;
    params: worst absolute distance, and the bar STEPS * 2^-23 * max|p|)."""
    gp, gm, gv, gn = got[:4]
    rp, rm, rv, rn = ref[:4]
    d_norm = max((abs(a - b) / b for a, b in zip(gn, rn)), default=0.0)
    d_m = max(float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(gm, rm))
    d_v = max(float((a.double() - b.double()).abs().max() / b.double().abs().max()) for a, b in zip(gv, rv))
    d_p = max(float((a.double() - b.double()).abs().max()) for a, b in zip(gp, rp))
    p_bar = STEPS * 2.0 ** -23 * max(float(b.abs().max()) for b in rp)
    return d_norm, d_m, d_v, d_p, p_bar


# The bars against the float64 restatement, from the roundings per step:
NORM_BAR = 2.5e-7          # a double sum rounded to float once: 2^-24, margin x4
EXP_AVG_BAR = 1e-6         # about 4 roundings of 2^-24 per step, margin x3 - 4
EXP_AVG_SQ_BAR = 2e-6      # the squared gradient doubles the relative error of the clipped gradient


def check_against_reference(label, got, case, decoupled, **ref_kw):
    ref = reference(case, decoupled, **ref_kw)
    d_norm, d_m, d_v, d_p, p_bar = distances(got, ref)
    print(f"{label}: norm {d_norm:.2e} (bar {NORM_BAR:.1e})  exp_avg {d_m:.2e} (bar {EXP_AVG_BAR:.0e})  "
          f"exp_avg_sq {d_v:.2e} (bar {EXP_AVG_SQ_BAR:.0e})  params {d_p:.2e} (bar {p_bar:.2e})")
    assert d_norm <= NORM_BAR, (label, d_norm)
    assert d_m <= EXP_AVG_BAR, (label, d_m)
    assert d_v <= EXP_AVG_SQ_BAR, (label, d_v)
    assert d_p <= p_bar, (label, d_p, p_bar)
    return d_norm, d_m, d_v, d_p, p_bar
