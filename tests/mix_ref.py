"""TEST INFRASTRUCTURE: the float64 numpy oracle of the on-device mix (include/wunet_hip.h: wunet_mix_windows).  It works from the two
flat arrays and the two tables alone - nothing is taken from the loader's or the kernels' arithmetic - and returns, per row, the
gains in double, the two waveforms formed in double from the gains rounded once to float32, and the magnitudes the bars are stated in."""
import math

import numpy as np

SILENT = 1e-12          # mean square below which a window counts as silent (RMS 1e-6)


def clamp_row(row, clean_total, noise_total, L):
    """(clean start, noise start, noise length, phase) of one table row after the clamps of the ABI, in Python integers."""
    cs, ns, nl, ph = (int(v) for v in row)
    cs = min(max(cs, 0), clean_total - L)
    nl = min(max(nl, 0), noise_total)
    lo, hi = max(ns, 0), min(ns + nl, noise_total)
    nl = max(hi - lo, 0)
    if nl == 0:
        lo, ph = 0, 0                # (nothing is left of the item: its start means nothing)
    else:
        ph %= nl
    return cs, lo, nl, ph


def mix_reference(clean_flat, noise_flat, rows, params, L, peak_limit):
    """clean_flat / noise_flat: float32 [total]; rows: int64 [B, 4]; params: float32 [B, 2]; peak_limit: the float the call passes.
    Returns a dict of arrays: g, a (float64 [B], before rounding), mixture, clean (float64 [B, L]), ac = |a c|, agn = |a g n| (the
    magnitudes of the bars), Et = sum (a c)^2, En = sum (a g n)^2, peak_fired (bool [B])."""
    clean_flat = np.asarray(clean_flat, np.float32)
    noise_flat = np.asarray(noise_flat, np.float32)
    rows = np.asarray(rows, np.int64)
    params = np.asarray(params, np.float32)
    B = rows.shape[0]
    peak = float(np.float32(peak_limit))
    out = {k: np.zeros(B) for k in ("g", "a", "Et", "En")}
    out["peak_fired"] = np.zeros(B, bool)
    for k in ("mixture", "clean", "ac", "agn"):
        out[k] = np.zeros((B, L))
    j = np.arange(L)
    for b in range(B):
        cs, ns, nl, ph = clamp_row(rows[b], len(clean_flat), len(noise_flat), L)
        c = clean_flat[cs:cs + L].astype(np.float64)
        n = noise_flat[ns + (ph + j) % nl].astype(np.float64) if nl > 0 else np.zeros(L)
        Pc, Pn = math.fsum(c * c), math.fsum(n * n)
        Mc, Mn = np.abs(c).max(), np.abs(n).max()
        g = 0.0
        if nl > 0 and Pc >= L * SILENT and Pn >= L * SILENT:
            g = math.sqrt(Pc / (Pn * 10.0 ** (float(params[b, 0]) / 10.0)))
        a = float(params[b, 1])
        if peak > 0.0:
            bound = a * (Mc + g * Mn)
            if bound > peak:
                a = a * peak / bound
                out["peak_fired"][b] = True
        g32, a32 = float(np.float32(g)), float(np.float32(a))
        out["g"][b], out["a"][b] = g, a
        out["clean"][b] = a32 * c
        out["mixture"][b] = a32 * (c + g32 * n)
        out["ac"][b] = np.abs(a32 * c)
        out["agn"][b] = np.abs(a32 * g32 * n)
        out["Et"][b] = math.fsum((a32 * c) ** 2)
        out["En"][b] = math.fsum((a32 * g32 * n) ** 2)
    return out
