"""TEST INFRASTRUCTURE: the oracle of the on-device biquad cascades (include/wunet_hip.h: wunet_sos_windows).  It works from the flat
array, the row table and the coefficient table alone: the clamps of the ABI in Python integers, the source of a row built explicitly
(lead-in and window, lead_b + L samples), and three runs of the recurrence
    o = b0 v + s0;  s0 = b1 v - a1 o + s1;  s1 = b2 v - a2 o
over it: in np.longdouble (the arbiter), by scipy.signal.sosfilt in float64 (the reference whose own error sizes the bar) and with
float32 state (what a kernel that dropped to single precision would give: the bar must reject it)."""
import numpy as np
import scipy.signal

HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
IMPULSE = 1 << 16            # samples of the impulse response that sum |h| is taken over (pole radius 0.999: 0.999^65536 = 3e-29)


def clamp_row(row, total, L, lead):
    """One table row after the clamps of the ABI, in Python integers: ("linear", ws, is, lead_b), ("circular", item start, nl, ph,
    lead_b) or ("zeros",) for a circular row of which nothing is left."""
    ws, is_, nl, ph = (int(v) for v in row)
    if nl <= 0:
        ws = min(max(ws, 0), total - L)
        is_ = min(max(is_, 0), ws)
        return ("linear", ws, is_, min(lead, ws - is_))
    nl = min(nl, total)              # (first, as the mix does: mix_ref.clamp_row)
    lo, hi = max(is_, 0), min(is_ + nl, total)
    if hi <= lo:
        return ("zeros",)
    return ("circular", lo, hi - lo, ph % (hi - lo), lead)


def source(flat, row, L, lead):
    """(x float32 [lead_b + L], lead_b) of one row, or (None, 0) for a row of zeros."""
    c = clamp_row(row, len(flat), L, lead)
    if c[0] == "zeros":
        return None, 0
    if c[0] == "linear":
        _, ws, _, lb = c
        return np.asarray(flat[ws - lb:ws + L], np.float32), lb
    _, lo, nl, ph, lb = c
    j = np.arange(-lb, L)
    return np.asarray(flat, np.float32)[lo + (ph + j) % nl], lb


def to_sos6(coefs):
    """[S, 5] (b0 b1 b2 a1 a2) -> scipy's float64 [S, 6]."""
    k = np.ascontiguousarray(coefs, np.float64)
    return np.concatenate([k[:, :3], np.ones((k.shape[0], 1)), k[:, 3:]], axis=1)


def recurrence(x, coefs, dtype):
    """The recurrence over x through the cascade coefs [S, 5], every value and operation in `dtype`.  Section after section (the
    cascade's sections only talk forwards), so the inner loop is over samples with scalars of the dtype."""
    v = np.asarray(x).astype(dtype)
    for b0, b1, b2, a1, a2 in np.asarray(coefs, np.float32).astype(dtype):
        o = np.empty_like(v)
        s0 = s1 = dtype(0)
        for t, vt in enumerate(v):
            ot = b0 * vt + s0
            s0 = b1 * vt - a1 * ot + s1
            s1 = b2 * vt - a2 * ot
            o[t] = ot
        v = o
    return v


def gain_bound(coefs):
    """sum |h| of the cascade's float64 impulse response."""
    imp = np.zeros(IMPULSE)
    imp[0] = 1.0
    return float(np.abs(scipy.signal.sosfilt(to_sos6(coefs), imp)).sum())


def sos_reference(flat, rows, coefs, L, lead, state_dtype=None):
    """flat float32 [total]; rows int64 [B, 4]; coefs float32 [B, S, 5].  Returns a dict of [B, L] arrays: arb (np.longdouble, the
    arbiter), bar (float64, per element), x (float32, the window as values) and [B] arrays e_ref, A, second (the bar's second term),
    rms.  With state_dtype (np.float32) only {"out": the recurrence in that dtype, as float64 [B, L]} is made."""
    flat, rows, coefs = np.asarray(flat, np.float32), np.asarray(rows, np.int64), np.asarray(coefs, np.float32)
    B = rows.shape[0]
    if state_dtype is not None:
        out = np.zeros((B, L))
        for b in range(B):
            x, lb = source(flat, rows[b], L, lead)
            if x is not None:
                out[b] = recurrence(x, coefs[b], state_dtype)[lb:].astype(np.float64)
        return {"out": out}
    ref = {"arb": np.zeros((B, L), np.longdouble), "bar": np.zeros((B, L)), "x": np.zeros((B, L), np.float32)}
    for k in ("e_ref", "A", "second", "rms"):
        ref[k] = np.zeros(B)
    for b in range(B):
        x, lb = source(flat, rows[b], L, lead)
        if x is None:
            continue
        arb = recurrence(x, coefs[b], np.longdouble)[lb:]
        sci = scipy.signal.sosfilt(to_sos6(coefs[b]), x.astype(np.float64))[lb:]
        e_ref = float(np.abs(sci.astype(np.longdouble) - arb).max())
        A = float(np.abs(x).max()) * gain_bound(coefs[b])
        second = max(8.0 * e_ref, 2.0 ** -50 * A)
        ref["arb"][b], ref["x"][b] = arb, x[lb:]
        ref["bar"][b] = 2.0 ** -24 * np.abs(arb).astype(np.float64) + second
        ref["e_ref"][b], ref["A"][b], ref["second"][b] = e_ref, A, second
        ref["rms"][b] = float(np.sqrt(np.mean(arb.astype(np.float64) ** 2)))
    return ref
