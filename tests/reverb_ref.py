"""TEST INFRASTRUCTURE: the float64 numpy oracle of the on-device reverb (include/wunet_hip.h: wunet_reverb_windows).  It works from the
two flat arrays and the row table alone: the clamps of the ABI in Python integers, then np.convolve per row on the float32 inputs
in double.  Beside the two outputs it returns the magnitudes the bars are stated in, S[b][j] = sum_k |h[k]| |x[cs + j - k]|."""
import numpy as np

MAX_TAPS = 16384        # WUNET_REVERB_MAX_TAPS
U = 2.0 ** -24          # unit roundoff of float32


def clamp_row(row, clean_total, rir_total, L):
    """(window start, item start, RIR start, taps) of one table row after the clamps of the ABI, in Python integers."""
    cs, it, hs, K = (int(v) for v in row)
    cs = min(max(cs, 0), clean_total - L)
    it = min(max(it, 0), cs)
    K = min(max(K, 0), rir_total)
    lo, hi = max(hs, 0), min(hs + K, rir_total)
    K = min(max(hi - lo, 0), MAX_TAPS)
    if K == 0:
        lo = 0                       # (nothing is left of the response: its start means nothing)
    return cs, it, lo, K


def gamma(n):
    """The bound of a chain of n float32 fused adds in any order (Higham, gamma_n)."""
    return n * U / (1.0 - n * U)


def _fir(x, h, skip, L):
    """out[j] = sum_k h[k] x[skip + j - k], j < L, for x that is zero in front of x[0] (double)."""
    if len(h) == 0:
        return np.zeros(L)
    return np.convolve(x, h)[skip:skip + L]


def reverb_reference(clean_flat, rir_flat, rows, L, early_taps):
    """clean_flat / rir_flat: float32 [total]; rows: int64 [B, 4].  Returns a dict of arrays: rows (the clamped table, int64 [B, 4]),
    reverberant, direct (float64 [B, L]; a row without taps is the window itself), S, Sd (float64 [B, L]: the sums of magnitudes behind
    the two), n, nd (int [B]: the chain lengths K + 256 and min(E, K) + 256 of the bars)."""
    clean_flat, rir_flat = np.asarray(clean_flat, np.float32), np.asarray(rir_flat, np.float32)
    rows = np.asarray(rows, np.int64)
    B = rows.shape[0]
    out = {k: np.zeros((B, L)) for k in ("reverberant", "direct", "S", "Sd")}
    out["rows"] = np.zeros((B, 4), np.int64)
    out["n"], out["nd"] = np.zeros(B, np.int64), np.zeros(B, np.int64)
    for b in range(B):
        cs, it, lo, K = clamp_row(rows[b], len(clean_flat), len(rir_flat), L)
        out["rows"][b] = (cs, it, lo, K)
        E = min(int(early_taps), K)
        out["n"][b], out["nd"][b] = K + 256, E + 256
        if K == 0:
            w = clean_flat[cs:cs + L].astype(np.float64)
            out["reverberant"][b], out["direct"][b], out["S"][b], out["Sd"][b] = w, w, np.abs(w), np.abs(w)
            continue
        first = max(it, cs - (K - 1))                    # nothing in front of it is reached by a tap (or it is the zero-fill)
        x = clean_flat[first:cs + L].astype(np.float64)
        h = rir_flat[lo:lo + K].astype(np.float64)
        out["reverberant"][b], out["S"][b] = _fir(x, h, cs - first, L), _fir(np.abs(x), np.abs(h), cs - first, L)
        out["direct"][b], out["Sd"][b] = _fir(x, h[:E], cs - first, L), _fir(np.abs(x), np.abs(h[:E]), cs - first, L)
    return out
