"""TEST INFRASTRUCTURE ONLY.  A float64 oracle of rational resampling (include/wunet_hip.h: wunet_resample_rows) in numpy only: the
textbook form - put up - 1 zeros between the samples, convolve with the filter, keep every down-th sample from the filter's centre on,
np.convolve(z, h)[L::down][:T_out], evaluated only at the samples that are kept.
With T_out = ceil(T up / down) it is scipy.signal.resample_poly(x, up, down, window = h' / up) (tests/test_resample_emu.py compares the
two where scipy imports).  It shares no code with the kernel: no phases, no i_hi."""
import numpy as np


def natural_length(T, up, down):
    return -((-int(T) * up) // down)


def resample(x, up, down, taps, T_out=None):
    """x: [T] (float32 or float64), taps: the float32 filter h' (gain folded in), widened to double here.  Returns (y float64 [T_out],
    s float64 [T_out] = sum |h'| |x| over the same terms - the bar of tests/resample_cases.py needs it).  A T_out above the natural
    length reads zeros behind the row."""
    x = np.asarray(x, np.float64)
    h = np.asarray(taps, np.float32).astype(np.float64)
    assert len(h) % 2 == 1
    L = (len(h) - 1) // 2
    T = len(x)
    T_out = natural_length(T, up, down) if T_out is None else int(T_out)
    # the zero-stuffed signal with L zeros in front and as many behind as the last kept sample reaches: full[k] of np.convolve(z, h)
    # is sum_t h[t] zp[k + 2 L - t], and only full[L + m down] is kept, so only those are evaluated (a strided view, no copy)
    n = max((T - 1) * up + 1, L + (T_out - 1) * down + 1) + 2 * L
    zp = np.zeros(n + 2 * L, np.float64)
    zp[2 * L:2 * L + (T - 1) * up + 1:up] = x
    win = np.lib.stride_tricks.as_strided(zp[L:], shape=(T_out, 2 * L + 1), strides=(down * zp.strides[0], zp.strides[0]), writeable=False)
    hr = h[::-1].copy()
    y = np.einsum("mk,k->m", win, hr)
    s = np.einsum("mk,k->m", np.abs(win), np.abs(hr)) if T_out * len(h) < (1 << 22) else _abs_sum(win, hr)
    assert len(y) == T_out
    return y, s


def _abs_sum(win, hr, step=64):
    """sum |h| |z| of every window, a slab of rows at a time (np.abs of the whole view would be a copy of T_out x n_taps doubles)."""
    a = np.abs(hr)
    return np.concatenate([np.einsum("mk,k->m", np.abs(win[i:i + step]), a) for i in range(0, win.shape[0], step)])
