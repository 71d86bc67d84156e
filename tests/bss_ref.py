"""TEST INFRASTRUCTURE: the oracle of the on-device BSS Eval SDR (include/wunet_hip.h: wunet_bss_sdr_forward), one source per row:
    r[k] = sum_t s[t] s[t + k],  b[k] = sum_t s[t] e[t + k]  (k < n),  E = sum e^2,  G = toeplitz(r),  G c = b,
    P = c'b,  R = E - 2 c'b + c'G c,  SDR = 10 log10(P / R)
which is mir_eval.separation.bss_eval_sources for a single source (reference padded with n - 1 zeros, no mean removal).  Four runs:
  arbiter       everything in np.longdouble: correlations as direct dot products (float32 x float32 is exact there), Levinson's
                recursion, the three quadratic forms
  reference     float64: np.correlate, scipy.linalg.solve_toeplitz, the same formulas - what a careful host implementation gives; its
                distance from the arbiter sizes the bar (tests/bss_cases.py)
  kernel model  float64, the kernel's own scheme: correlation partials per segment of `tile` samples added in segment order, then
                Levinson's recursion as the kernel orders it - measured against the reference's error when the bar was chosen
  single        the reference with float32 correlation accumulators: what a kernel that summed in single precision would give; the
                bar must reject it."""
import numpy as np
import scipy.linalg

HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant >= 63
K10 = 10.0 / np.log(10.0)


def correlations(s, e, n, dtype):
    """(r [n], b [n], E) of one row by direct dot products with every value and sum in `dtype`."""
    s, e = np.asarray(s).astype(dtype), np.asarray(e).astype(dtype)
    T = len(s)
    r, b = np.zeros(n, dtype), np.zeros(n, dtype)
    for k in range(min(n, T)):
        r[k] = np.dot(s[:T - k], s[k:])
        b[k] = np.dot(s[:T - k], e[k:])
    return r, b, np.dot(e, e)


def correlations_np(s, e, n, dtype):
    """The same by np.correlate on arrays of `dtype` (float64: the reference; float32: single-precision accumulators)."""
    s, e = np.asarray(s).astype(dtype), np.asarray(e).astype(dtype)
    T = len(s)
    m = min(n, T)
    r, b = np.zeros(n, dtype), np.zeros(n, dtype)
    # np.correlate(a, v, "full")[T - 1 + k] = sum_t a[t + k] v[t]
    r[:m] = np.correlate(s, s, "full")[T - 1:T - 1 + m]
    b[:m] = np.correlate(e, s, "full")[T - 1:T - 1 + m]
    return r, b, np.dot(e, e)


def correlations_segmented(s, e, n, tile):
    """float64, the kernel's order: per segment of `tile` samples and lag k the products s[t] s[t + k] of the segment's t in order; the
    segments' partials added in segment order."""
    s, e = np.asarray(s, np.float64), np.asarray(e, np.float64)
    T = len(s)
    sp, ep = np.concatenate([s, np.zeros(n)]), np.concatenate([e, np.zeros(n)])
    r, b, E = np.zeros(n), np.zeros(n), 0.0
    for t0 in range(0, T, tile):
        t1 = min(T, t0 + tile)
        pr, pb = np.zeros(n), np.zeros(n)
        for k in range(n):
            # (a sequential sum, as a thread of the kernel forms it: cumsum adds left to right)
            pr[k] = np.cumsum(s[t0:t1] * sp[t0 + k:t1 + k])[-1]
            pb[k] = np.cumsum(s[t0:t1] * ep[t0 + k:t1 + k])[-1]
        r, b, E = r + pr, b + pb, E + np.cumsum(e[t0:t1] * e[t0:t1])[-1]
    return r, b, E


def levinson(r, b, dtype):
    """Solve toeplitz(r) c = b by Levinson's recursion in `dtype`: a the prediction polynomial (a[0] = 1), eps its error."""
    r, b = np.asarray(r).astype(dtype), np.asarray(b).astype(dtype)
    n = len(r)
    a, x = np.zeros(n, dtype), np.zeros(n, dtype)
    a[0], x[0], eps = 1, b[0] / r[0], r[0]
    for m in range(1, n):
        back = r[m:0:-1]                                 # r[m], r[m - 1], .., r[1]
        acc, q = np.dot(a[:m], back), np.dot(x[:m], back)
        k = -acc / eps
        a[:m + 1] = a[:m + 1] + k * a[m::-1]
        eps = eps * (1 - k * k)
        x[:m + 1] = x[:m + 1] + ((b[m] - q) / eps) * a[m::-1]
    return x


def score(r, b, E, c, dtype):
    """(SDR in dB, E / R) from the correlations and the solution, in `dtype`."""
    r, b, c = np.asarray(r).astype(dtype), np.asarray(b).astype(dtype), np.asarray(c).astype(dtype)
    idx = np.abs(np.arange(len(r))[:, None] - np.arange(len(r))[None, :])
    P = np.dot(c, b)
    Q = np.dot(c, np.dot(r[idx], c))
    R = (dtype(E) - 2 * P) + Q
    with np.errstate(divide="ignore", invalid="ignore"):
        return K10 * np.log(P / R), dtype(E) / R


def arbiter_row(s, e, n):
    r, b, E = correlations(s, e, n, np.longdouble)
    return score(r, b, E, levinson(r, b, np.longdouble), np.longdouble)


def reference_row(s, e, n, accumulate=np.float64):
    """float64 reference; accumulate=np.float32: the correlations summed in single precision, everything behind them as before."""
    r, b, E = (np.asarray(v, np.float64) for v in correlations_np(s, e, n, accumulate))
    c = scipy.linalg.solve_toeplitz(r, b)
    return float(score(r, b, float(E), c, np.float64)[0])


def kernel_model_row(s, e, n, tile):
    r, b, E = correlations_segmented(s, e, n, tile)
    return float(score(r, b, E, levinson(r, b, np.float64), np.float64)[0])


def live(s, e):
    """A row scores a number when neither its reference nor its estimate is silent (and it has samples)."""
    return len(s) > 0 and bool(np.any(s)) and bool(np.any(e))


def bss_reference(clean, est, n, lengths=None, K=1.0, floor_units=8.0):
    """clean, est float32 [rows, T]; lengths None or [rows].  Returns [rows] arrays: arb (np.longdouble dB; NaN for a row that is not
    live), ref (float64), e_ref, ratio (E / R of the arbiter), first, second, bar (the terms of tests/bss_cases.py's bar)."""
    clean, est = np.asarray(clean, np.float32), np.asarray(est, np.float32)
    rows, T = clean.shape
    out = {"arb": np.full(rows, np.nan, np.longdouble)}
    for key in ("ref", "e_ref", "ratio", "first", "second", "bar"):
        out[key] = np.full(rows, np.nan)
    for i in range(rows):
        L = T if lengths is None else int(min(max(int(lengths[i]), 0), T))
        s, e = clean[i, :L], est[i, :L]
        if not live(s, e):
            continue
        arb, ratio = arbiter_row(s, e, n)
        ref = reference_row(s, e, n)
        out["arb"][i], out["ref"][i], out["ratio"][i] = arb, ref, float(ratio)
        if not np.isfinite(arb):
            continue
        out["e_ref"][i] = float(abs(np.longdouble(ref) - arb))
        out["first"][i] = 2.0 ** -24 * float(abs(arb))
        out["second"][i] = max(K * out["e_ref"][i], floor_units * 2.0 ** -53 * K10 * float(ratio))
        out["bar"][i] = out["first"][i] + out["second"][i]
    return out
