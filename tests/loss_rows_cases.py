"""The op cases of the row losses, shared by tests/test_loss_rows_emu.py (CPU emulator) and tests/test_gpu_loss_rows.py (MI355X):
what runs, on which tensors, and the checks against tests/si_sdr_ref.py.  `engine` None = the product's default engine."""
import importlib

import torch

import si_sdr_ref as R
from conftest import PKG_NAME

KINDS = ("si_sdr", "snr")
# (rows, T) -> pieces per row / lanes per row in the finalize (csrc/wunet_ops.cpp: row_pieces) / rows per trip of its row loop:
#   (1,1) one sample; (3,7) odd and tiny; (2,1000) one piece with a tail; (70,257) many rows of odd length - all 1 piece, 1 lane, 1 trip
#   (5,4099)   2 pieces, 2 lanes per row: rows whose 16-byte phase differs (odd T), a 3-sample second piece
#   (1,200003) one row over 49 pieces (64 lanes), odd tail
#   (300,7)    1 lane per row, 256 rows per trip: TWO trips of the finalize's row loop
#   (100,8200) 3 pieces, 4 lanes per row, 64 rows per trip: two trips with the butterfly between them, the second one partly filled
SHAPES = ((1, 1), (3, 7), (2, 1000), (5, 4099), (70, 257), (1, 200003), (300, 7), (100, 8200))


def mods():
    return importlib.import_module(PKG_NAME + ".loss"), importlib.import_module(PKG_NAME + ".metrics")


def run(engine, device, kind, zero_mean, s, e, grad_loss=None, eps=1e-8):
    """loss(clean, enhanced) through the public module, backward with `grad_loss` (None: plain .backward()).
    Returns (loss, gradient w.r.t. enhanced)."""
    loss_mod, _ = mods()
    crit = getattr(loss_mod, kind + "_loss")(zero_mean=zero_mean, eps=eps)
    crit._engine_override = engine
    s = s.to(device)
    e = e.detach().to(device).requires_grad_(True)         # (detach: a leaf of its own on the same memory - an unaligned view stays one)
    loss = crit(s, e)
    if grad_loss is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(grad_loss, device=device))
    return loss.detach(), e.grad


def rows_db(engine, device, kind, zero_mean, s, e, eps=1e-8):
    _, metrics = mods()
    return getattr(metrics, kind)(s.to(device), e.to(device), zero_mean=zero_mean, eps=eps, engine=engine)


def check_case(what, engine, device, kind, zero_mean, s, e, grad_rows=None):
    """loss, per-row values and gradient of one pair against the float64 yardstick; grad_rows: the rows the gradient bar is asked of."""
    loss, g = run(engine, device, kind, zero_mean, s, e)
    rows = rows_db(engine, device, kind, zero_mean, s, e)
    rl, rv, rg = R.reference(kind, s, e, zero_mean)
    dv = R.check_values(what, loss, rows, rl, rv)
    T = s.shape[-1]
    g2, rg2 = g.reshape(-1, T), rg.reshape(-1, T)
    if grad_rows is not None:
        g2, rg2 = g2[list(grad_rows)], rg2[list(grad_rows)]
    dg = R.check_grad(what, g2, rg2)
    return dv, dg, loss, rows, g


def degenerate(T=64, seed=5):
    """Rows: s = 0 and e = 0; s = 0 with unit-variance e; e = s; an ordinary row."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(4, 1, T, generator=g)
    e = torch.randn(4, 1, T, generator=g)
    s[0] = 0.0
    e[0] = 0.0
    s[1] = 0.0
    e[2] = s[2]
    return s, e


def unaligned(R_, T, device, seed=3):
    """Both inputs as views one float into their buffers: a base pointer with 4-byte alignment only."""
    s, e = R.pair(R_, T, seed)
    bs = torch.zeros(R_ * T + 8, device=device)
    be = torch.zeros(R_ * T + 8, device=device)
    bs[1:1 + R_ * T] = s.reshape(-1).to(device)
    be[1:1 + R_ * T] = e.reshape(-1).to(device)
    return s, e, bs[1:1 + R_ * T].view(R_, 1, T), be[1:1 + R_ * T].view(R_, 1, T)


def check_degenerate(engine, device, kind):
    """s = 0 and e = 0: exactly 0 dB and a zero gradient; s = 0: about -98 dB (eps over the energy of 64 unit-variance samples),
    finite gradient; e = s: about +98 dB, finite gradient.  Each row as a batch of its own against the yardstick with the usual bars
    (the loss is then minus the row's value), then the four rows as one batch: rows and gradients with the usual bars.  The loss of
    that batch is only asked to be finite and minus the mean of its own rows: it is a mean in which +97 and -98 dB cancel to 3 dB,
    and the yardstick's own e = s row (the rounding of a full cancellation next to eps) is good to 4e-6 dB, not to 2^-22 of 3 dB."""
    s, e = degenerate()
    for k in range(4):
        check_case(f"degenerate {kind} row {k}", engine, device, kind, True, s[k:k + 1].contiguous(), e[k:k + 1].contiguous())
    loss, g = run(engine, device, kind, True, s, e)
    rows = rows_db(engine, device, kind, True, s, e)
    _, rv, rg = R.reference(kind, s, e, True)
    R.check_values(f"degenerate {kind}", -rows.double().mean(), rows, -rows.double().mean(), rv)
    R.check_grad(f"degenerate {kind}", g, rg)
    print(f"degenerate {kind}: rows {rows.tolist()}")
    assert rows[0].item() == 0.0 and not g[0].any()
    assert -99.5 < rows[1].item() < -96.5 and torch.isfinite(g[1]).all() and g[1].any()
    assert 96.5 < rows[2].item() < 99.5 and torch.isfinite(g[2]).all()
    # (the float rounding of each row, 2^-24 of at most 98 dB, and of the loss itself, 2^-24 of 3 dB: together below 2^-23 * 98)
    assert torch.isfinite(loss) and abs(float(loss) + rows.double().mean().item()) <= 2.0 ** -23 * 98.0
