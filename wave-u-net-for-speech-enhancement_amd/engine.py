"""Python face of the C ABI: owns per-shape contexts, turns torch tensors into raw device pointers
and enqueues the HIP path on torch's current stream.  PyTorch is plumbing here (device memory,
streams); every arithmetic kernel lives in csrc/."""
import collections
import ctypes
import os
import threading
import weakref

import torch

from . import _lib

_C = _lib.CONSTANTS                            # the #defines of include/wunet_hip.h
LOSS_KINDS = {k: _C["WUNET_LOSS_" + k.upper()] for k in ("mse", "l1", "smooth_l1")}
ROW_LOSS_KINDS = {k: _C["WUNET_LOSS_" + k.upper()] for k in ("si_sdr", "snr")}      # per-row criteria, wunet_loss_rows_* only
LOSS_ROW_COEFS = _C["WUNET_LOSS_ROW_COEFS"]


class WunetError(RuntimeError):
    pass


def bump_versions(tensors):
    """Tell autograd's version counters that a kernel wrote these tensors through raw pointers (what every in-place torch op does
    by itself).  torch >= 2.1 has the call (a list where it is accepted, else tensor by tensor); older ones are left as they were."""
    inc = getattr(torch.autograd.graph, "increment_version", None)
    if inc is None:
        return
    try:
        inc(tensors)                     # (recent torch takes the whole list)
    except TypeError:                    # torch 2.1 - 2.4: one tensor per call
        for t in tensors:
            inc(t)


class _ParamSignature:
    """What the eval-mode weight-pack cache is valid for: THESE parameter tensor objects (weak references - an address the caching
    allocator hands to the next model's weights is not the same tensor), at these addresses and autograd versions, and no device-side
    rewrite (Engine.weights_generation) since."""
    __slots__ = ("refs", "state", "gen")

    def __init__(self, params, gen):
        self.refs = [weakref.ref(p) for p in params]
        self.state = tuple((p.data_ptr(), p._version) for p in params)
        self.gen = gen

    def matches(self, other):
        """self: the cached entry; other: the signature of the call's parameters (alive by construction)."""
        if self.gen != other.gen or self.state != other.state or len(self.refs) != len(other.refs):
            return False
        return all(a() is b() and a() is not None for a, b in zip(self.refs, other.refs))


class FlatGrads:
    """The gradient tensors of `Engine.backward` as ONE flat fp32 buffer + the element offset of every parameter in it."""

    def __init__(self, flat, offsets):
        self.flat, self.offsets = flat, offsets


def _load_torch_ext():
    """The optional C++ marshalling layer (torch_ext/wunet_torch.cpp, built by __graft_entry__.build()); None when it is not there or
    when WUNET_LIB_PATH selects another build of the library (the extension is linked to csrc/libwunet_hip.so)."""
    if os.environ.get("WUNET_LIB_PATH") or os.environ.get("WUNET_NO_TORCH_EXT"):
        return None
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "torch_ext", "_wunet_torch.so")
    stamp = path + ".torch"              # the torch version the extension was built against (__graft_entry__._build_torch_ext)
    if not os.path.exists(path):
        return None
    try:
        if open(stamp).read().strip() != torch.__version__:
            return None                  # built against another torch: its ABI is not this one's - the ctypes path instead
    except OSError:
        return None
    try:
        import importlib.util
        spec = importlib.util.spec_from_file_location("_wunet_torch", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    except Exception:                    # noqa: BLE001 - optional: a stale build (other torch) falls back to ctypes
        return None


# ---------------------------------------------------------------------- multi-resolution STFT loss (include/wunet_hip.h: wunet_stft_*)
STFT_COEFS = _C["WUNET_STFT_COEFS"]                       # a, b, sc, mag per resolution
STFT_MAX_RESOLUTIONS = _C["WUNET_STFT_MAX_RESOLUTIONS"]
CSPEC_COEFS = _C["WUNET_CSPEC_COEFS"]                     # the two gradient scales, the two term values per resolution (wunet_cspec_*)
MEL_COEFS = _C["WUNET_MEL_COEFS"]                         # likewise (wunet_mel_*)
MEL_MAX_FILTERS = _C["WUNET_MEL_MAX_FILTERS"]


class _SpectralFamily:
    """What tells the spectral losses apart on their one host path (Engine._spectral_loss_*): c - the entry points are wunet_<c>_*;
    what - starts the messages; coefs - float64 values per resolution; cspec - wunet_cspec_*'s call shape: scalars (compress, clamp) not
    (clamp,), one finalize weight not two, byte counts behind the scratch and saved pointers (wunet_stft_forward: mag_out); saved_by_dtype
    - the backward holds saved[i] to float32 and leaves its size to the C call, else it holds its bytes to wunet_<c>_saved_bytes; mel -
    wunet_mel_*'s call shape: cspec's byte counts, and per resolution a filterbank (n_mels, filt) in front of the scalars (power, clamp,
    floor), n_mels in the saved-size query and in the finalize's table, two finalize weights."""

    def __init__(self, c, what, coefs, cspec, saved_by_dtype, mel=False):
        self.c, self.what, self.coefs, self.cspec, self.saved_by_dtype, self.mel = c, what, coefs, cspec, saved_by_dtype, mel


_STFT = _SpectralFamily("stft", "stft loss", STFT_COEFS, False, False)
_CSPEC = _SpectralFamily("cspec", "compressed spectral loss", CSPEC_COEFS, True, True)
_MEL = _SpectralFamily("mel", "mel loss", MEL_COEFS, False, True, mel=True)


def _ptr(t):
    return t.data_ptr() if t is not None else None


def check_stft_resolution(n_fft, hop, win_length):
    """The constraints of one resolution that do not depend on the waveform (what wunet_stft_* refuses with WUNET_E_ARG)."""
    n_fft, hop, win_length = int(n_fft), int(hop), int(win_length)
    if n_fft < 16 or n_fft > 4096 or n_fft % 16:
        raise ValueError(f"stft: n_fft must be a multiple of 16 in 16 .. 4096 (got {n_fft})")
    if hop < 1 or hop > n_fft:
        raise ValueError(f"stft: hop must be in 1 .. n_fft (got {hop}, n_fft {n_fft})")
    if win_length < 1 or win_length > n_fft:
        raise ValueError(f"stft: win_length must be in 1 .. n_fft (got {win_length}, n_fft {n_fft})")
    return n_fft, hop, win_length


def _hz_to_mel(f, mel_scale):
    import numpy as np
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    return np.where(f < 1000.0, f / (200.0 / 3.0), 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0))


def _mel_to_hz(m, mel_scale):
    import numpy as np
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m < 15.0, m * (200.0 / 3.0), 1000.0 * np.exp((np.log(6.4) / 27.0) * (np.maximum(m, 15.0) - 15.0)))


def mel_filterbank(sample_rate, n_fft, n_mels, fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney"):
    """The triangular mel filterbank of the mel loss: a float32 [n_mels, n_fft // 2 + 1] CPU tensor, computed in float64 with numpy and
    rounded once.  n_mels + 2 points equally spaced on the mel axis between mel(fmin) and mel(fmax) (fmax None: sample_rate / 2), mapped
    back to Hz as p; filter j at the bin frequency f = b sample_rate / n_fft is max(0, min((f - p[j]) / (p[j+1] - p[j]),
    (p[j+2] - f) / (p[j+2] - p[j+1]))).  mel_scale "htk": mel = 2595 log10(1 + f / 700); "slaney": f / (200 / 3) below 1000 Hz,
    15 + ln(f / 1000) / (ln 6.4 / 27) from there up.  norm "slaney": row j times 2 / (p[j+2] - p[j]); None: peaks of 1.  These are the
    formulas of librosa.filters.mel (whose defaults are the ones here); the agreement is by the formulas only - librosa was not at hand
    to compare against.  A bank with filters that no bin falls under (all-zero rows) is allowed and warned about."""
    import warnings
    import numpy as np
    sample_rate, n_fft, n_mels = float(sample_rate), int(n_fft), int(n_mels)
    if not (sample_rate > 0.0 and sample_rate < float("inf")):
        raise ValueError(f"mel_filterbank: sample_rate must be finite and > 0 (got {sample_rate})")
    if n_fft < 2 or n_fft % 2:
        raise ValueError(f"mel_filterbank: n_fft must be even and >= 2 (got {n_fft})")
    if n_mels < 1 or n_mels > MEL_MAX_FILTERS:
        raise ValueError(f"mel_filterbank: n_mels must be in 1 .. {MEL_MAX_FILTERS} (got {n_mels})")
    fmax = sample_rate / 2.0 if fmax is None else float(fmax)
    fmin = float(fmin)
    if not (0.0 <= fmin < fmax <= sample_rate / 2.0):
        raise ValueError(f"mel_filterbank: 0 <= fmin < fmax <= sample_rate / 2 (got fmin {fmin}, fmax {fmax}, sample_rate {sample_rate})")
    if mel_scale not in ("slaney", "htk"):
        raise ValueError(f"mel_filterbank: mel_scale is 'slaney' or 'htk' (got {mel_scale!r})")
    if norm not in ("slaney", None):
        raise ValueError(f"mel_filterbank: norm is 'slaney' or None (got {norm!r})")
    p = _mel_to_hz(np.linspace(float(_hz_to_mel(fmin, mel_scale)), float(_hz_to_mel(fmax, mel_scale)), n_mels + 2), mel_scale)
    f = np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)
    up = (f[None, :] - p[:-2, None]) / (p[1:-1] - p[:-2])[:, None]
    down = (p[2:, None] - f[None, :]) / (p[2:] - p[1:-1])[:, None]
    fb = np.maximum(0.0, np.minimum(up, down))
    if norm == "slaney":
        fb *= (2.0 / (p[2:] - p[:-2]))[:, None]
    empty = int((fb.max(axis=1) == 0.0).sum())
    if empty:
        warnings.warn(f"mel_filterbank: {empty} of {n_mels} filters have no bin under them at n_fft {n_fft} (all-zero rows): fewer mels or "
                      "a larger n_fft would fill them")
    return torch.from_numpy(fb.astype(np.float32))


# ---------------------------------------------------------------------- STOI per row (include/wunet_hip.h: wunet_stoi_*)
STOI_FS = 10000
STOI_MAX_TAPS = 4096                 # WUNET_STOI_MAX_TAPS of csrc/wunet_stoi.h
_STOI_TAPS = {}                      # sample rate -> (p, q, float32 taps of pystoi's resampler) or None at 10 kHz


def stoi_resampler_taps(sample_rate):
    """pystoi's resampling filter for `sample_rate` -> 10 kHz: (p, q, h) with 10000 / sample_rate = p / q in lowest terms and
    h[t + L] = kaiser(2 L + 1, 0.1102 (60 - 8.7))[t + L] 2 p fc sinc(2 fc t), fc = 1 / (2 max(p, q)), L = ceil(52 / (28.714 fc / 10)),
    normalised to sum 1 - computed in float64 with numpy, rounded once to float32, cached per rate.  None at 10 kHz."""
    fs = int(sample_rate)
    if fs not in _STOI_TAPS:
        import math
        import numpy as np
        if fs <= 0:
            raise ValueError(f"stoi: the sample rate must be > 0 (got {sample_rate})")
        if fs == STOI_FS:
            _STOI_TAPS[fs] = None
        else:
            g = math.gcd(STOI_FS, fs)
            p, q = STOI_FS // g, fs // g
            fc = 1.0 / (2.0 * max(p, q))
            L = int(math.ceil(52.0 / (28.714 * fc / 10.0)))
            t = np.arange(-L, L + 1, dtype=np.float64)
            h = np.kaiser(2 * L + 1, 0.1102 * (60.0 - 8.7)) * (2.0 * p * fc * np.sinc(2.0 * fc * t))
            _STOI_TAPS[fs] = (p, q, (h / h.sum()).astype(np.float32))
    return _STOI_TAPS[fs]


def check_stoi_rate(sample_rate):
    """The sample rates wunet_stoi_* accept (what wunet_stoi_tables_bytes refuses with 0): > 0 and a resampling filter of at most
    STOI_MAX_TAPS taps."""
    fs = int(sample_rate)
    taps = stoi_resampler_taps(fs)
    if taps is not None and len(taps[2]) > STOI_MAX_TAPS:
        raise ValueError(f"stoi: {fs} Hz is {taps[1]} / {taps[0]} of 10 kHz and needs {len(taps[2])} filter taps; at most {STOI_MAX_TAPS} "
                         "are supported (max(p, q) <= 56)")
    return fs


ADAM_HYPER_FLOATS = _C["WUNET_ADAM_HYPER_FLOATS"]


class Engine:
    """One per process is enough (see `default_engine`).  `lib`/`host_memory` exist so the CPU test
    suite can drive the same host logic against the emulator build with CPU tensors; product code
    never passes them."""

    def __init__(self, lib=None, host_memory=False, h3=None):
        self.lib = lib if lib is not None else _lib.load_hip()
        self.host_memory = host_memory
        # GEMM arithmetic of the levels >= 16 samples (include/wunet_hip.h: wunet_set_h3): 1 = fp16-split MFMA where the grid
        # fills the chip (default), 0 = fp32 MFMA everywhere (WUNET_H3=0), 2 = fp16-split wherever it can run (tests),
        # 3 = bf16 operands, one MFMA pass, on the planner's layers (BASELINE configs[4]), 4 = bf16 wherever it can run (tests)
        self.h3 = int(os.environ.get("WUNET_H3", "1")) if h3 is None else int(h3)
        # contexts are keyed by shape AND device (the ctx owns a weight-gradient side stream per device it runs on; replicas
        # of one shape on several devices - a stock nn.DataParallel wrap, trainer/base_trainer.py:26-27 - get their own),
        # least-recently-used ones are destroyed beyond MAX_CONTEXTS (variable-length inference would otherwise leak one per shape)
        self._ctx = collections.OrderedDict()
        self._lock = threading.Lock()
        self._eval_ws = collections.OrderedDict()     # (shape, device, stream) -> (workspace of the last eval forward, parameter signature)
        # Bumped by everything that rewrites weights WITHOUT moving a Python version counter: the replay of a captured step graph
        # (FusedAdam.advance_host_step) - part of the eval cache's signature, so an eval forward after N replays re-packs.
        self.weights_generation = 0
        self._spectral = {}                           # "stft" / "cspec" / "mel" -> their five C calls in self.lib (_spectral_calls)
        self._stft_bases = {}                         # (n_fft, win_length, device) -> windowed DFT basis (stft_basis)
        self._mel_banks = {}                          # (device, sample_rate, n_fft, n_mels, fmin, fmax, mel_scale, norm) -> filterbank (mel_bank)
        self._stoi_tables_cache = {}                  # (sample rate, device) -> basis | window | resampler taps (stoi_tables)
        self._resample_taps_cache = {}                # (up, down, device) -> the resampling filter on the device (resample_taps)
        # per-step calls marshalled in C++ when the extension is built and this engine drives the HIP library it is linked to
        self._fast = _load_torch_ext() if (lib is None and not host_memory) else None

    # ------------------------------------------------------------------ helpers
    def _check(self, rc):
        if rc != 0:
            raise WunetError(f"wunet error {rc}: {self.lib.wunet_last_error().decode()}")

    MAX_CONTEXTS = 32

    def _ctx_for(self, n_layers, ci, batch, length, device=None):
        """The context of one (shape, device), created on first use.  Every C call that takes the handle runs inside
        `with self._using(...) as h` (below): a handle that some thread still holds is never destroyed by the eviction of
        another thread (stock nn.DataParallel calls forward from one thread per replica, trainer/base_trainer.py:26-27)."""
        key = (n_layers, ci, batch, length, str(device))
        with self._lock:
            ent = self._ctx.get(key)
            if ent is None:
                h = ctypes.c_void_p()
                self._check(self.lib.wunet_create(n_layers, ci, batch, length, ctypes.byref(h)))
                if self.h3:
                    self._check(self.lib.wunet_set_h3(h, self.h3))
                ent = self._ctx[key] = [h, 0, None]              # [handle, holders, BatchNorm mask set on it (None: none frozen)]
            else:
                self._ctx.move_to_end(key)
            ent[1] += 1
            # least-recently-used contexts nobody holds go beyond MAX_CONTEXTS (oldest first; the one just handed out is held)
            for k in [k for k, e in self._ctx.items() if e[1] == 0][:max(0, len(self._ctx) - self.MAX_CONTEXTS)]:
                self.lib.wunet_destroy(self._ctx.pop(k)[0])       # (HIP defers the side stream's destruction until its work has drained)
        return key, ent

    def _release(self, ent):
        with self._lock:
            ent[1] -= 1

    def _using(self, n_layers, ci, batch, length, device=None):
        return _CtxHold(self, *self._ctx_for(n_layers, ci, batch, length, device))

    def _set_frozen(self, hold, frozen):
        """Per-layer BatchNorm mode of the held context (include/wunet_hip.h: wunet_set_bn_frozen) for the call that follows in the
        same hold: `frozen` - one truthy entry per conv layer for a BatchNorm on the running statistics, or None.  The context is
        shared by every model of its shape, so each call states its mask; the C call is only made when the mask changes."""
        ent = hold.ent
        want = bytes(1 if f else 0 for f in frozen) if frozen is not None and any(frozen) else None
        if ent[2] != want:
            if want is None:
                self._check(self.lib.wunet_set_bn_frozen(ent[0], None, 0))
            else:
                self._check(self.lib.wunet_set_bn_frozen(ent[0], ctypes.create_string_buffer(want, len(want)), len(want)))
            ent[2] = want

    def _require(self, t, name):
        if t.dtype != torch.float32 and t.dtype != torch.int64:
            raise WunetError(f"{name}: expected float32, got {t.dtype}")
        if not t.is_contiguous():
            raise WunetError(f"{name}: tensor must be contiguous")
        if self.host_memory:
            if not t.is_cpu:
                raise WunetError(f"{name}: emulator engine takes CPU tensors")
        elif not t.is_cuda:              # (device.type != "cuda", without making the device object)
            raise WunetError(f"{name}: the HIP path needs tensors on an MI355X (got device {t.device}); "
                             "there is no CPU fallback")

    def _stream(self, device):
        if self.host_memory:
            return None
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    @staticmethod
    def _ptrs(tensors):
        return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])

    def _require_all(self, tensors, what, device=None):
        """`_require` of a whole list (+ same device as `device`) in one pass - the 102 parameters, 75 buffers and 4 x 102 Adam
        tensors of a step: the per-tensor form cost the host ~0.8 us per tensor, a third of the time it needs to issue a step.
        The slow path below names the offender."""
        f32, i64 = torch.float32, torch.int64
        on_gpu = not self.host_memory
        idx = -1 if device is None or device.index is None else device.index
        for t in tensors:
            dt = t.dtype
            if (dt is not f32 and dt is not i64) or not t.is_contiguous() or t.is_cuda is not on_gpu or (on_gpu and idx >= 0 and t.get_device() != idx):
                break
        else:
            return
        for k, t in enumerate(tensors):
            self._require(t, f"{what}[{k}]")
            if device is not None and t.device != device:
                raise WunetError(f"{what}[{k}] lives on {t.device}, the call runs on {device}: parameters and input live on different devices")

    def _device_guard(self, device):
        return torch.cuda.device(device) if not self.host_memory else _NullCtx()

    def _wave_pair(self, what, clean, other, other_name="enhanced"):
        """The checks every (clean, other) waveform pair gets; `what` starts the messages.  The last dimension is the row, all leading
        ones are flattened: returns (rows, T, device)."""
        self._require(clean, "clean")
        self._require(other, other_name)
        if clean.dtype != torch.float32 or other.dtype != torch.float32:
            raise WunetError(f"{what}: expected float32 waveforms")
        if clean.shape != other.shape or clean.device != other.device:
            raise WunetError(f"{what}: shape / device mismatch {tuple(clean.shape)} vs {tuple(other.shape)}")
        if other.dim() < 1 or other.numel() == 0:
            raise WunetError(f"{what}: needs at least one row of at least one sample, got {tuple(other.shape)}")
        T = other.shape[-1]
        return other.numel() // T, T, other.device

    def _table_op(self, op, label, expected, tensors, table):
        """The checks every row-table op (mix_windows .. resample_rows) starts with; `op` starts the messages.  tensors: the op's, in
        argument order (None: an optional one not given), float32 except the int64 `table`; `expected` words the dtype message; each then
        goes through _require as `label`.  Returns the tensors given, for _same_device once the op has checked its own shapes."""
        given = [t for t in tensors if t is not None]
        for t in given:
            if t.dtype is not (torch.int64 if t is table else torch.float32):
                raise WunetError(f"{op}: {expected} expected")
        for t in given:
            self._require(t, label)
        return given

    @staticmethod
    def _same_device(op, tensors, device, where):
        for t in tensors:
            if t.device != device:
                raise WunetError(f"{op}: every tensor must live on {where}")

    def _sized(self, nbytes):
        """The answer of a size query of the C ABI: 0 is a refused shape, and wunet_last_error says why."""
        if nbytes == 0:
            raise WunetError(f"wunet error -1: {self.lib.wunet_last_error().decode()}")
        return nbytes

    # ------------------------------------------------------------------ network
    def forward(self, n_layers, ci, noisy, params, running, nbt, training, with_backward, frozen=None):
        """Returns (enhanced, workspace).  Keep `workspace` alive until backward has been enqueued.  frozen (training mode): per conv
        layer, True where its BatchNorm uses the running statistics and leaves them untouched (nn.BatchNorm1d in eval mode)."""
        if not training:
            frozen = None                    # (eval mode: every layer already runs on the running statistics)
        if noisy.dim() != 3 or noisy.shape[1] != 1:
            raise WunetError(f"input must be [batch, 1, samples], got {tuple(noisy.shape)}")
        # eval mode (enhancement.py:57-69: the same weights over every chunk of every file): the workspace of the previous eval forward
        # on this (shape, device, stream) is used again, and while no parameter has changed - addresses and autograd version counters,
        # which every in-place torch op, load_state_dict and FusedAdam.step move - the weight packs in it are not rebuilt
        cache = sig = None
        if training and self._eval_ws:
            self.drop_eval_cache()           # training resumes: the eval workspaces (up to MAX_EVAL_WORKSPACES whole forwards) go back to the allocator
        if (not training and not with_backward and not self.host_memory and noisy.is_cuda and noisy.dtype == torch.float32
                and not os.environ.get("WUNET_NO_EVAL_CACHE")):                       # (switch: A/B; a CPU / non-float input falls through to _require's error)
            key = (n_layers, ci, noisy.shape[0], noisy.shape[2], str(noisy.device), torch.cuda.current_stream(noisy.device).cuda_stream)
            try:
                sig = _ParamSignature(params, self.weights_generation)
            except (RuntimeError, TypeError):                                         # inference tensors have no version counter: no cache
                sig = None
            if sig is not None:
                with self._lock:
                    cache = self._eval_ws.pop(key, None)         # (popped: a second thread on the same key takes a fresh workspace)
                if cache is not None and not cache[1].matches(sig):
                    cache = (cache[0], None)
        if self._fast is not None:
            hold = self._using(n_layers, ci, noisy.shape[0], noisy.shape[2], noisy.device)
            with hold as h:
                self._set_frozen(hold, frozen)
                try:
                    out, ws = self._fast.forward(h.value, noisy, params, running, nbt, bool(training), bool(with_backward),
                                                 cache[0] if cache else None, bool(cache and cache[1] is not None))
                except RuntimeError as e:
                    raise WunetError(str(e).split("\n")[0]) from None
            if sig is not None:
                self._remember_eval_ws(key, ws, sig)
            return out, ws
        self._require(noisy, "input")
        self._require_all(params, "param", noisy.device)
        self._require_all(running, "buffer", noisy.device)
        self._require_all(nbt, "buffer", noisy.device)
        B, _, T = noisy.shape
        hold = self._using(n_layers, ci, B, T, noisy.device)
        with hold as h, self._device_guard(noisy.device):
            self._set_frozen(hold, frozen)
            nbytes = self.lib.wunet_workspace_bytes(h, 1 if with_backward else 0)
            reuse = cache is not None and cache[0].numel() * 4 >= nbytes
            ws = cache[0] if reuse else torch.empty(nbytes // 4, dtype=torch.float32, device=noisy.device)
            out = torch.empty_like(noisy)
            flags = (_C["WUNET_FWD_SAVE"] if with_backward else 0) | (_C["WUNET_FWD_PACKS_VALID"] if reuse and cache[1] is not None else 0)
            self._check(self.lib.wunet_forward(h, noisy.data_ptr(), self._ptrs(params), self._ptrs(running),
                                               self._ptrs(nbt), 1 if training else 0, flags, ws.data_ptr(),
                                               out.data_ptr(), self._stream(noisy.device)))
        if sig is not None:
            self._remember_eval_ws(key, ws, sig)
        return out, ws

    MAX_EVAL_WORKSPACES = 4

    def _remember_eval_ws(self, key, ws, sig):
        with self._lock:
            self._eval_ws[key] = (ws, sig)
            while len(self._eval_ws) > self.MAX_EVAL_WORKSPACES:            # (variable-length inference: the oldest shapes go)
                self._eval_ws.pop(next(iter(self._eval_ws)))

    def note_weights_changed(self):
        """Weights were rewritten on the device without a Python-side in-place op (a graph replay that contains the optimiser step):
        cached eval weight packs of every model on this engine are stale from here on."""
        self.weights_generation += 1

    def drop_eval_cache(self):
        """Forget the eval-mode workspaces (and with them the cached weight packs): for a caller that changed weights behind autograd's
        back (`p.data[...] = ...` does not move a version counter)."""
        with self._lock:
            self._eval_ws.clear()

    def backward(self, n_layers, ci, noisy, params, enhanced, grad_enhanced, ws, grads, layer_range=None, join=True, frozen=None):
        """join=False: the caller's stream does not wait for the range's weight gradients (side stream); make a stream see them
        with `join_weight_gradients` (parallel.GradSync does, on the stream that launches the bucket's all-reduce).
        frozen: the mask of the training forward that filled `ws` (see `forward`)."""
        B, _, T = noisy.shape
        self._require(grad_enhanced, "grad_output")
        nl = 2 * n_layers + 1
        lb, le = layer_range if layer_range is not None else (0, nl)
        if self._fast is not None and isinstance(grads, FlatGrads):
            hold = self._using(n_layers, ci, B, T, noisy.device)
            with hold as h:
                self._set_frozen(hold, frozen)
                try:
                    self._fast.backward_range(h.value, noisy, params, enhanced, grad_enhanced, ws, grads.flat, grads.offsets, lb, le, bool(join))
                except RuntimeError as e:
                    raise WunetError(str(e).split("\n")[0]) from None
            return
        fn = self.lib.wunet_backward_range if join else self.lib.wunet_backward_range_async
        if isinstance(grads, FlatGrads):         # one flat buffer + element offsets: the pointers are arithmetic, no 102 views first
            base = grads.flat.data_ptr()
            gptrs = (ctypes.c_void_p * len(grads.offsets))(*[base + 4 * o for o in grads.offsets])
        else:
            gptrs = self._ptrs(grads)
        hold = self._using(n_layers, ci, B, T, noisy.device)
        with hold as h, self._device_guard(noisy.device):
            self._set_frozen(hold, frozen)
            self._check(fn(h, noisy.data_ptr(), self._ptrs(params), enhanced.data_ptr(), grad_enhanced.data_ptr(), ws.data_ptr(),
                           gptrs, lb, le, self._stream(noisy.device)))

    def backward_input(self, n_layers, ci, noisy, params, ws):
        """dL/d(noisy) [B, 1, T] (include/wunet_hip.h: wunet_backward_input): enqueued on the current stream right behind the backward
        call that covered layer 0 on `ws` (same context, frozen mask and stream)."""
        self._require(noisy, "input")
        B, _, T = noisy.shape
        g = torch.empty_like(noisy)
        with self._using(n_layers, ci, B, T, noisy.device) as h, self._device_guard(noisy.device):
            self._check(self.lib.wunet_backward_input(h, noisy.data_ptr(), self._ptrs(params), ws.data_ptr(), g.data_ptr(),
                                                      self._stream(noisy.device)))
        return g

    def join_weight_gradients(self, n_layers, ci, noisy):
        """Torch's current stream waits for everything the weight-gradient side stream has been given so far."""
        B, _, T = noisy.shape
        with self._using(n_layers, ci, B, T, noisy.device) as h, self._device_guard(noisy.device):
            self._check(self.lib.wunet_backward_join(h, self._stream(noisy.device)))

    def layer_output(self, n_layers, ci, batch, length, ws, layer):
        """Raw conv output (pre-BatchNorm) of conv layer `layer` as a view into a workspace (tests/profiling)."""
        off, ch, ln = ctypes.c_size_t(), ctypes.c_int(), ctypes.c_int()
        with self._using(n_layers, ci, batch, length, ws.device) as h:
            self._check(self.lib.wunet_layer_info(h, layer, ctypes.byref(off), ctypes.byref(ch), ctypes.byref(ln)))
        return ws[off.value: off.value + batch * ch.value * ln.value].view(batch, ch.value, ln.value)

    # ------------------------------------------------------------------ losses
    def loss_forward(self, kind, clean, enhanced):
        self._require(clean, "clean")
        self._require(enhanced, "enhanced")
        if clean.shape != enhanced.shape:
            raise WunetError(f"loss: shape mismatch {tuple(clean.shape)} vs {tuple(enhanced.shape)}")
        out = torch.empty((), dtype=torch.float32, device=enhanced.device)
        scratch = torch.empty(self.lib.wunet_loss_scratch_bytes() // 8, dtype=torch.float64, device=enhanced.device)
        with self._device_guard(enhanced.device):
            self._check(self.lib.wunet_loss_forward(LOSS_KINDS[kind], clean.data_ptr(), enhanced.data_ptr(),
                                                    enhanced.numel(), out.data_ptr(), scratch.data_ptr(),
                                                    self._stream(enhanced.device)))
        return out

    def loss_backward(self, kind, clean, enhanced, grad_loss):
        g = torch.empty_like(enhanced)
        gl = grad_loss.to(torch.float32).contiguous()
        with self._device_guard(enhanced.device):
            self._check(self.lib.wunet_loss_backward(LOSS_KINDS[kind], clean.data_ptr(), enhanced.data_ptr(),
                                                     gl.data_ptr(), enhanced.numel(), g.data_ptr(),
                                                     self._stream(enhanced.device)))
        return g

    # ------------------------------------------------------------------ row losses (SI-SDR / SNR per utterance)
    def loss_rows_forward(self, kind, clean, enhanced, zero_mean=True, eps=1e-8, per_row=False, with_backward=True):
        """include/wunet_hip.h: wunet_loss_rows_forward.  The last dimension is the row, all leading ones are flattened.  Returns
        (loss, coefs, per_row_db): loss - device scalar, -mean of the rows' dB values; coefs - float64 [rows, LOSS_ROW_COEFS] for
        `loss_rows_backward` (None with with_backward=False); per_row_db - float32 [rows] with per_row=True, else None."""
        if kind not in ROW_LOSS_KINDS:
            raise WunetError(f"row loss: unknown kind {kind!r} (one of {sorted(ROW_LOSS_KINDS)})")
        R, T, dev = self._wave_pair("row loss", clean, enhanced)
        out = torch.empty((), dtype=torch.float32, device=dev)
        rows = torch.empty(R, dtype=torch.float32, device=dev) if per_row else None
        coefs = torch.empty(R, LOSS_ROW_COEFS, dtype=torch.float64, device=dev) if with_backward else None
        scratch = torch.empty(max(1, self.lib.wunet_loss_rows_scratch_bytes(R, T) // 8), dtype=torch.float64, device=dev)
        with self._device_guard(dev):
            self._check(self.lib.wunet_loss_rows_forward(ROW_LOSS_KINDS[kind], 1 if zero_mean else 0, float(eps), clean.data_ptr(),
                                                         enhanced.data_ptr(), R, T, out.data_ptr(), _ptr(rows), _ptr(coefs),
                                                         scratch.data_ptr(), self._stream(dev)))
        return out, coefs, rows

    def loss_rows_backward(self, kind, clean, enhanced, coefs, grad_loss):
        """d loss / d enhanced of the `loss_rows_forward` of the same kind that produced `coefs`, times grad_loss (a scalar tensor)."""
        if kind not in ROW_LOSS_KINDS:
            raise WunetError(f"row loss: unknown kind {kind!r} (one of {sorted(ROW_LOSS_KINDS)})")
        R, T, dev = self._wave_pair("row loss", clean, enhanced)
        if coefs.dtype != torch.float64 or coefs.numel() != R * LOSS_ROW_COEFS or not coefs.is_contiguous() or coefs.device != dev:
            raise WunetError(f"row loss: coefs must be the float64 [{R}, {LOSS_ROW_COEFS}] tensor of loss_rows_forward")
        g = torch.empty_like(enhanced)
        gl = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
        with self._device_guard(dev):
            self._check(self.lib.wunet_loss_rows_backward(ROW_LOSS_KINDS[kind], clean.data_ptr(), enhanced.data_ptr(), coefs.data_ptr(), gl.data_ptr(), R, T,
                                                          g.data_ptr(), self._stream(dev)))
        return g

    # ------------------------------------------------------------------ multi-resolution STFT loss (wunet_stft_*)
    def stft_basis(self, n_fft, win_length, device):
        """The windowed DFT basis of (n_fft, win_length) on `device`, built once: on the first (eager) call, so that a later graph capture
        sees neither its allocation nor its launch."""
        return self._basis(n_fft, win_length, device, str(device))

    def _basis(self, n_fft, win_length, device, where):
        key = (n_fft, win_length, where)                 # (where = str(device): a loop over resolutions makes the string once)
        basis = self._stft_bases.get(key)
        if basis is None:
            basis = torch.empty(self._sized(self.lib.wunet_stft_basis_bytes(n_fft)) // 4, dtype=torch.float32, device=device)
            with self._device_guard(device):
                self._check(self.lib.wunet_stft_basis(n_fft, win_length, basis.data_ptr(), self._stream(device)))
            self._stft_bases[key] = basis
        return basis

    def _spectral_calls(self, fam):
        """(scratch_bytes, saved_bytes, forward, finalize, backward) of one spectral loss in this engine's library, looked up once."""
        if fam.c not in self._spectral:
            self._spectral[fam.c] = tuple(getattr(self.lib, f"wunet_{fam.c}_{n}") for n in ("scratch_bytes", "saved_bytes", "forward", "finalize", "backward"))
        return self._spectral[fam.c]

    def _spectral_loss_forward(self, fam, clean, enhanced, resolutions, knobs, weights, with_backward, banks=None):
        """Every spectral loss: per resolution wunet_<c>_forward with the scalars `knobs`, then one wunet_<c>_finalize with `weights`.
        banks (the mel loss): per resolution (n_mels, filterbank on the device)."""
        R, T, dev = self._wave_pair(fam.what, clean, enhanced)
        n = len(resolutions)
        if n < 1 or n > STFT_MAX_RESOLUTIONS:
            raise WunetError(f"{fam.what}: 1 .. {STFT_MAX_RESOLUTIONS} resolutions (got {n})")
        scratch_bytes, saved_bytes, forward, finalize, _ = self._spectral_calls(fam)
        out = torch.empty((), dtype=torch.float32, device=dev)
        coefs = torch.empty(n, fam.coefs, dtype=torch.float64, device=dev)
        scratch, saved = [], []
        where = str(dev)
        with self._device_guard(dev):
            st = self._stream(dev)
            for i, (N, H, W) in enumerate(resolutions):
                basis = self._basis(N, W, dev, where)
                scr = torch.empty(self._sized(scratch_bytes(R, T, N, H, 0)) // 8, dtype=torch.float64, device=dev)
                more = (banks[i][0],) if fam.mel else ()
                sv = torch.empty(saved_bytes(R, T, N, H, *more) // 4, dtype=torch.float32, device=dev) if with_backward else None
                if fam.mel:
                    rc = forward(clean.data_ptr(), enhanced.data_ptr(), R, T, N, H, W, banks[i][0], banks[i][1].data_ptr(), int(knobs[0]),
                                 float(knobs[1]), float(knobs[2]), basis.data_ptr(), scr.data_ptr(), scr.numel() * 8, _ptr(sv),
                                 sv.numel() * 4 if sv is not None else 0, None, st)
                elif fam.cspec:
                    rc = forward(clean.data_ptr(), enhanced.data_ptr(), R, T, N, H, W, float(knobs[0]), float(knobs[1]), basis.data_ptr(),
                                 scr.data_ptr(), scr.numel() * 8, _ptr(sv), sv.numel() * 4 if sv is not None else 0, st)
                else:
                    rc = forward(clean.data_ptr(), enhanced.data_ptr(), R, T, N, H, W, float(knobs[0]), basis.data_ptr(), scr.data_ptr(), _ptr(sv), None, st)
                self._check(rc)
                scratch.append(scr)
                saved.append(sv)
            ffts, hops = (ctypes.c_int * n)(*[r[0] for r in resolutions]), (ctypes.c_int * n)(*[r[1] for r in resolutions])
            if fam.mel:
                rc = finalize(n, self._ptrs(scratch), R, T, ffts, hops, (ctypes.c_int * n)(*[b[0] for b in banks]), float(weights[0]),
                              float(weights[1]), out.data_ptr(), coefs.data_ptr(), st)
            elif fam.cspec:
                rc = finalize(n, self._ptrs(scratch), R, T, ffts, hops, float(weights[0]), out.data_ptr(), coefs.data_ptr(), st)
            else:
                rc = finalize(n, self._ptrs(scratch), R, T, ffts, hops, float(weights[0]), float(weights[1]), out.data_ptr(), coefs.data_ptr(), st)
            self._check(rc)
        return out, coefs, (saved if with_backward else None)

    def _spectral_loss_backward(self, fam, shape, resolutions, coefs, saved, grad_loss, knobs, banks=None):
        """Every spectral loss: per resolution wunet_<c>_backward with the scalars `knobs`; the first writes g, the others add to it."""
        n = len(resolutions)
        if coefs.dtype != torch.float64 or coefs.numel() != n * fam.coefs or not coefs.is_contiguous() or saved is None or len(saved) != n:
            raise WunetError(f"{fam.what}: coefs / saved must be those of {fam.c}_loss_forward over the same {n} resolutions")
        dev = coefs.device
        T = shape[-1]
        g = torch.empty(shape, dtype=torch.float32, device=dev)
        R = g.numel() // T
        gl = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
        scratch_bytes, saved_bytes, _, _, backward = self._spectral_calls(fam)
        where = str(dev)
        with self._device_guard(dev):
            st = self._stream(dev)
            for i, (N, H, W) in enumerate(resolutions):
                sv = saved[i]
                wrong = sv.dtype != torch.float32 if fam.saved_by_dtype else sv.numel() * 4 != saved_bytes(R, T, N, H)
                if wrong or sv.device != dev:
                    raise WunetError(f"{fam.what}: saved[{i}] is not the buffer of resolution {(N, H, W)} on {tuple(shape)}")
                scr = torch.empty(scratch_bytes(R, T, N, H, 1) // 4, dtype=torch.float32, device=dev)
                basis = self._basis(N, W, dev, where)
                if fam.mel:
                    rc = backward(sv.data_ptr(), sv.numel() * 4, coefs.data_ptr() + 8 * fam.coefs * i, gl.data_ptr(), R, T, N, H, W, banks[i][0],
                                  banks[i][1].data_ptr(), int(knobs[0]), float(knobs[1]), float(knobs[2]), basis.data_ptr(), scr.data_ptr(),
                                  scr.numel() * 4, g.data_ptr(), 1 if i else 0, st)
                elif fam.cspec:
                    rc = backward(sv.data_ptr(), sv.numel() * 4, coefs.data_ptr() + 8 * fam.coefs * i, gl.data_ptr(), R, T, N, H, W, float(knobs[0]),
                                  float(knobs[1]), basis.data_ptr(), scr.data_ptr(), scr.numel() * 4, g.data_ptr(), 1 if i else 0, st)
                else:
                    rc = backward(sv.data_ptr(), coefs.data_ptr() + 8 * fam.coefs * i, gl.data_ptr(), R, T, N, H, W, float(knobs[0]),
                                  basis.data_ptr(), scr.data_ptr(), g.data_ptr(), 1 if i else 0, st)
                self._check(rc)
        return g

    def stft_loss_forward(self, clean, enhanced, resolutions, sc_weight=1.0, mag_weight=1.0, clamp=1e-7, with_backward=True):
        """resolutions: a sequence of (n_fft, hop, win_length).  The last dimension is the utterance, all leading ones are flattened.
        Returns (loss, coefs, saved): loss - device scalar; coefs - float64 [n_res, STFT_COEFS] (a, b, sc, mag per resolution);
        saved - one float32 buffer per resolution for `stft_loss_backward` (None with with_backward=False)."""
        return self._spectral_loss_forward(_STFT, clean, enhanced, resolutions, (clamp,), (sc_weight, mag_weight), with_backward)

    def stft_loss_backward(self, shape, resolutions, coefs, saved, grad_loss, clamp=1e-7):
        """d loss / d enhanced (a tensor of `shape`) of the `stft_loss_forward` that produced `coefs` and `saved`, times grad_loss (a scalar
        tensor).  The resolutions are added in their order: one fixed order of sums."""
        return self._spectral_loss_backward(_STFT, shape, resolutions, coefs, saved, grad_loss, (clamp,))

    # ------------------------------------------------------------------ compressed spectral loss (wunet_cspec_*)
    def cspec_loss_forward(self, clean, enhanced, resolutions, compress=0.3, complex_weight=0.3, clamp=1e-7, with_backward=True):
        """resolutions: a sequence of (n_fft, hop, win_length).  The last dimension is the utterance, all leading ones are flattened.
        Returns (loss, coefs, saved): loss - device scalar; coefs - float64 [n_res, CSPEC_COEFS] (the two gradient scales, the two term
        values per resolution); saved - one float32 buffer per resolution for `cspec_loss_backward` (None with with_backward=False)."""
        return self._spectral_loss_forward(_CSPEC, clean, enhanced, resolutions, (compress, clamp), (complex_weight,), with_backward)

    def cspec_loss_backward(self, shape, resolutions, coefs, saved, grad_loss, compress=0.3, clamp=1e-7):
        """d loss / d enhanced (a tensor of `shape`) of the `cspec_loss_forward` that produced `coefs` and `saved`, times grad_loss (a
        scalar tensor).  The resolutions are added in their order: one fixed order of sums."""
        return self._spectral_loss_backward(_CSPEC, shape, resolutions, coefs, saved, grad_loss, (compress, clamp))

    # ------------------------------------------------------------------ multi-scale log-mel loss (wunet_mel_*)
    def mel_bank(self, device, sample_rate, n_fft, n_mels, fmin=0.0, fmax=None, mel_scale="slaney", norm="slaney"):
        """(n_mels, filterbank [n_mels, BP] on `device`) of one key: loss.mel_filterbank's float32 rows padded with zeros to the bins
        rounded up to 32, uploaded once - on the first (eager) call, so that a later graph capture sees no allocation (stft_basis's rule)."""
        key = (str(device), float(sample_rate), int(n_fft), int(n_mels), float(fmin), None if fmax is None else float(fmax), mel_scale, norm)
        bank = self._mel_banks.get(key)
        if bank is None:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # (empty filters: the warning belongs to the construction of the loss)
                fb = mel_filterbank(sample_rate, n_fft, n_mels, fmin, fmax, mel_scale, norm)
            padded = torch.zeros(fb.shape[0], (fb.shape[1] + 31) // 32 * 32, dtype=torch.float32)
            padded[:, :fb.shape[1]] = fb
            bank = self._mel_banks[key] = (int(n_mels), padded.to(device))
        return bank

    def mel_loss_forward(self, clean, enhanced, resolutions, banks, power=1, log_weight=1.0, lin_weight=0.0, clamp=1e-7, floor=1e-5,
                         with_backward=True):
        """resolutions: a sequence of (n_fft, hop, win_length); banks: per resolution the pair of `mel_bank`.  The last dimension is the
        utterance, all leading ones are flattened.  Returns (loss, coefs, saved): loss - device scalar; coefs - float64 [n_res, MEL_COEFS]
        (the two gradient scales, the two term values per resolution); saved - one float32 buffer per resolution for `mel_loss_backward`
        (None with with_backward=False)."""
        if len(banks) != len(resolutions):
            raise WunetError(f"mel loss: one filterbank per resolution (got {len(banks)} for {len(resolutions)})")
        return self._spectral_loss_forward(_MEL, clean, enhanced, resolutions, (power, clamp, floor), (log_weight, lin_weight), with_backward, banks)

    def mel_loss_backward(self, shape, resolutions, banks, coefs, saved, grad_loss, power=1, clamp=1e-7, floor=1e-5):
        """d loss / d enhanced (a tensor of `shape`) of the `mel_loss_forward` that produced `coefs` and `saved`, times grad_loss (a scalar
        tensor).  The resolutions are added in their order: one fixed order of sums.  The call writes into `saved` (the plane of dS)."""
        if len(banks) != len(resolutions):
            raise WunetError(f"mel loss: one filterbank per resolution (got {len(banks)} for {len(resolutions)})")
        return self._spectral_loss_backward(_MEL, shape, resolutions, coefs, saved, grad_loss, (power, clamp, floor), banks)

    def mel_spectrogram(self, x, bank, n_fft=512, hop=128, win_length=512, power=1, floor=0.0):
        """The mel spectrogram of every row of x through `bank` (the pair of `mel_bank`; stft_magnitude's conventions, no clamp): float32
        [rows, F, n_mels] - m, or ln max(m, floor) where floor > 0."""
        self._require(x, "x")
        if x.dtype != torch.float32 or x.dim() < 1 or x.numel() == 0:
            raise WunetError(f"mel: expected a float32 waveform tensor, got {x.dtype} {tuple(x.shape)}")
        n_fft, hop, win_length = check_stft_resolution(n_fft, hop, win_length)
        T = x.shape[-1]
        R = x.numel() // T
        dev = x.device
        n_mels, filt = bank
        if filt.device != dev:
            raise WunetError(f"mel: the filterbank lives on {filt.device}, x on {dev}")
        out = torch.empty(R, 1 + T // hop, n_mels, dtype=torch.float32, device=dev)
        with self._device_guard(dev):
            basis = self.stft_basis(n_fft, win_length, dev)
            scr = torch.empty(self._sized(self.lib.wunet_mel_scratch_bytes(R, T, n_fft, hop, 0)) // 8, dtype=torch.float64, device=dev)
            self._check(self.lib.wunet_mel_forward(None, x.data_ptr(), R, T, n_fft, hop, win_length, n_mels, filt.data_ptr(), int(power), 0.0,
                                                   float(floor), basis.data_ptr(), scr.data_ptr(), scr.numel() * 8, None, 0, out.data_ptr(),
                                                   self._stream(dev)))
        return out

    def stft_magnitude(self, x, n_fft=320, hop=160, win_length=320):
        """|STFT| of every row of x (periodic Hann, center=True, reflect padding - torch.stft's conventions): float32 [rows, F, n_fft/2 + 1]."""
        self._require(x, "x")
        if x.dtype != torch.float32 or x.dim() < 1 or x.numel() == 0:
            raise WunetError(f"stft: expected a float32 waveform tensor, got {x.dtype} {tuple(x.shape)}")
        n_fft, hop, win_length = check_stft_resolution(n_fft, hop, win_length)
        T = x.shape[-1]
        R = x.numel() // T
        dev = x.device
        if n_fft // 2 > T - 1:
            raise WunetError(f"stft: reflect padding needs n_fft / 2 <= T - 1 (n_fft {n_fft}, T {T})")
        F, bins = 1 + T // hop, n_fft // 2 + 1
        mag = torch.empty(R, F, bins, dtype=torch.float32, device=dev)
        with self._device_guard(dev):
            basis = self.stft_basis(n_fft, win_length, dev)
            self._check(self.lib.wunet_stft_forward(None, x.data_ptr(), R, T, n_fft, hop, win_length, 0.0, basis.data_ptr(), None, None,
                                                    mag.data_ptr(), self._stream(dev)))
        return mag

    # ------------------------------------------------------------------ STOI per row (wunet_stoi_*)
    def stoi_tables(self, sample_rate, device):
        """The tables of one (sample rate, device) - DFT basis, window, resampler taps - built once: on the first (eager) call, so that a
        later graph capture sees neither their allocation nor their launch."""
        key = (int(sample_rate), str(device))
        tables = self._stoi_tables_cache.get(key)
        if tables is None:
            taps = stoi_resampler_taps(sample_rate)
            tables = torch.empty(self._sized(self.lib.wunet_stoi_tables_bytes(key[0])) // 4, dtype=torch.float32, device=device)
            h = torch.from_numpy(taps[2]).to(device) if taps is not None else None
            with self._device_guard(device):
                self._check(self.lib.wunet_stoi_tables_build(key[0], _ptr(h), h.numel() if h is not None else 0, tables.data_ptr(),
                                                             self._stream(device)))
                if h is not None and not self.host_memory:
                    h.record_stream(torch.cuda.current_stream(device))       # (the copy kernel may still be reading it when h is freed)
            self._stoi_tables_cache[key] = tables
        return tables

    def _stoi_call(self, extended, name):
        """wunet_stoi_<name>, or wunet_estoi_<name> with `extended` (ESTOI: the same arguments, the same tables)."""
        return getattr(self.lib, ("wunet_estoi_" if extended else "wunet_stoi_") + name)

    def stoi(self, clean, estimate, sample_rate=16000, return_frames=False, extended=False):
        """include/wunet_hip.h: wunet_stoi_forward (extended: wunet_estoi_forward).  The last dimension is the utterance, all leading ones
        are flattened.  Returns float32 [rows] (and int32 [rows], the spectral frame count of every row, with return_frames).  Nothing is
        read back to the host."""
        R, T, dev = self._wave_pair("stoi", clean, estimate, "estimate")
        fs = int(sample_rate)
        tables = self.stoi_tables(fs, dev)
        scratch = torch.empty(self._sized(self._stoi_call(extended, "scratch_bytes")(R, T, fs)) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(R, dtype=torch.float32, device=dev)
        frames = torch.empty(R, dtype=torch.int32, device=dev) if return_frames else None
        with self._device_guard(dev):
            self._check(self._stoi_call(extended, "forward")(clean.data_ptr(), estimate.data_ptr(), R, T, fs, tables.data_ptr(), scratch.data_ptr(),
                                                             out.data_ptr(), _ptr(frames), self._stream(dev)))
        return (out, frames) if return_frames else out

    def stoi_loss_forward(self, clean, enhanced, sample_rate=16000, per_row=False, with_backward=True, extended=False):
        """include/wunet_hip.h: wunet_stoi_loss_forward (extended: wunet_estoi_loss_forward).  The last dimension is the utterance, all
        leading ones are flattened.  Returns (loss, saved, per_row): loss - device scalar, -mean of the rows' STOI; saved - the buffer
        `stoi_loss_backward` needs (kept even with with_backward=False: the forward writes its spectra there); per_row - float32 [rows]
        with per_row=True, else None."""
        R, T, dev = self._wave_pair("stoi loss", clean, enhanced)
        fs = int(sample_rate)
        tables = self.stoi_tables(fs, dev)
        scratch = torch.empty(self._sized(self._stoi_call(extended, "loss_scratch_bytes")(R, T, fs)) // 8, dtype=torch.float64, device=dev)
        saved = torch.empty(self._sized(self._stoi_call(extended, "loss_saved_bytes")(R, T, fs)) // 4, dtype=torch.float32, device=dev)
        out = torch.empty((), dtype=torch.float32, device=dev)
        rows = torch.empty(R, dtype=torch.float32, device=dev) if per_row else None
        with self._device_guard(dev):
            self._check(self._stoi_call(extended, "loss_forward")(clean.data_ptr(), enhanced.data_ptr(), R, T, fs, tables.data_ptr(),
                                                                  scratch.data_ptr(), saved.data_ptr(), out.data_ptr(),
                                                                  _ptr(rows), None, self._stream(dev)))
        return out, (saved if with_backward else None), rows

    def stoi_loss_backward(self, shape, saved, grad_loss, sample_rate=16000, extended=False):
        """d loss / d enhanced (a tensor of `shape`, every sample written) of the `stoi_loss_forward` that produced `saved` (with the
        same `extended`), times grad_loss (a scalar tensor)."""
        fs = int(sample_rate)
        T = shape[-1]
        dev = saved.device
        g = torch.empty(shape, dtype=torch.float32, device=dev)
        R = g.numel() // T
        if saved.dtype != torch.float32 or not saved.is_contiguous() or saved.numel() * 4 != self._stoi_call(extended, "loss_saved_bytes")(R, T, fs):
            raise WunetError(f"stoi loss: saved is not the buffer of stoi_loss_forward on {tuple(shape)} at {fs} Hz")
        tables = self.stoi_tables(fs, dev)
        scratch = torch.empty(self._sized(self._stoi_call(extended, "loss_scratch_bytes")(R, T, fs)) // 8, dtype=torch.float64, device=dev)
        gl = grad_loss.to(device=dev, dtype=torch.float32).contiguous()
        with self._device_guard(dev):
            self._check(self._stoi_call(extended, "loss_backward")(saved.data_ptr(), gl.data_ptr(), R, T, fs, tables.data_ptr(), scratch.data_ptr(),
                                                                   g.data_ptr(), self._stream(dev)))
        return g

    # ------------------------------------------------------------------ fused Adam, data input
    def adam_step(self, params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0, step_dev=None, hyper_dev=None, *,
                  weight_decay=0.0, max_grad_norm=None, lr_dev=None, scratch=None):
        """One fused Adam step over a list of tensors.  step_dev (int64 device scalar) + hyper_dev (2 floats):
        the step count lives on the device and the call increments it (capturable in a hipGraph); otherwise `step` is the host's.
        Keyword arguments (include/wunet_hip.h: wunet_adam_step_ex - the kernels of wunet_adam_step with an 8-float hyper buffer; with
        all of them off the call is wunet_adam_step, whose hyper buffer has 2 floats or is None):
        weight_decay - decoupled (AdamW); max_grad_norm - clipping by the global norm inside the step, `scratch` then holds
        adam_scratch_bytes(len(params)) bytes (p.grad is NOT modified); lr_dev - a float64 device scalar the learning rate is read from.
        Any of them needs hyper_dev with ADAM_HYPER_FLOATS floats: [2] clip, [3] the norm before clipping, [4] 1 - lr * weight_decay."""
        ex = bool(weight_decay) or max_grad_norm is not None or lr_dev is not None
        if ex:
            clip = float(max_grad_norm) if max_grad_norm is not None else 0.0
            if max_grad_norm is not None and not clip > 0.0:
                raise WunetError(f"adam_step: max_grad_norm must be > 0 (got {max_grad_norm}); None turns clipping off")
            if hyper_dev is None or hyper_dev.dtype != torch.float32 or hyper_dev.numel() < ADAM_HYPER_FLOATS or not hyper_dev.is_contiguous():
                raise WunetError(f"adam_step: weight_decay / max_grad_norm / lr_dev need hyper_dev with {ADAM_HYPER_FLOATS} float32")
            if lr_dev is not None and (lr_dev.dtype != torch.float64 or lr_dev.numel() != 1):
                raise WunetError("adam_step: lr_dev must be ONE float64")
            if clip > 0.0 and (scratch is None or scratch.numel() * scratch.element_size() < self.adam_scratch_bytes(len(params))):
                raise WunetError("adam_step: max_grad_norm needs `scratch` of adam_scratch_bytes(len(params)) bytes")
            extra = [t for t in (step_dev, hyper_dev, lr_dev, scratch) if t is not None]
            if any(t.device != params[0].device for t in extra):
                raise WunetError("adam_step: step_dev / hyper_dev / lr_dev / scratch must live on the parameters' device")
        if self._fast is not None:
            try:
                if ex:
                    self._fast.adam_step_ex(params, grads, exp_avg, exp_avg_sq, float(lr), float(beta1), float(beta2), float(eps), int(step),
                                            float(grad_scale), float(weight_decay), clip, step_dev, hyper_dev, lr_dev, scratch)
                else:
                    self._fast.adam_step(params, grads, exp_avg, exp_avg_sq, float(lr), float(beta1), float(beta2), float(eps), int(step),
                                         float(grad_scale), step_dev, hyper_dev)
            except RuntimeError as e:
                raise WunetError(str(e).split("\n")[0]) from None
            return
        for name, ts in (("param", params), ("grad", grads), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            self._require_all(ts, "adam " + name, params[0].device)
        n = len(params)
        numels = (ctypes.c_size_t * n)(*[p.numel() for p in params])
        dev = params[0].device
        with self._device_guard(dev):
            if ex:
                self._check(self.lib.wunet_adam_step_ex(n, self._ptrs(params), self._ptrs(grads), self._ptrs(exp_avg), self._ptrs(exp_avg_sq),
                                                        numels, float(lr), float(beta1), float(beta2), float(eps), int(step),
                                                        float(grad_scale), float(weight_decay), clip, _ptr(step_dev), _ptr(hyper_dev),
                                                        _ptr(lr_dev), _ptr(scratch), self._stream(dev)))
            else:
                self._check(self.lib.wunet_adam_step(n, self._ptrs(params), self._ptrs(grads), self._ptrs(exp_avg),
                                                     self._ptrs(exp_avg_sq), numels, float(lr), float(beta1), float(beta2),
                                                     float(eps), int(step), float(grad_scale), _ptr(step_dev), _ptr(hyper_dev), self._stream(dev)))

    def adam_scratch_bytes(self, n_tensors):
        """Device bytes of the partial sums of the gradient norm (adam_step(max_grad_norm=...)) over n_tensors tensors."""
        return int(self.lib.wunet_adam_scratch_bytes(int(n_tensors)))

    def crop_windows(self, mixture_flat, clean_flat, starts, mixture, clean):
        """mixture[b, 0, :] = mixture_flat[starts[b] : starts[b] + L], clean likewise (one launch for the batch)."""
        for t in (mixture_flat, clean_flat, starts, mixture, clean):
            self._require(t, "crop tensor")
        if starts.dtype != torch.int64 or mixture_flat.dtype != torch.float32 or mixture.dtype != torch.float32:
            raise WunetError("crop_windows: float32 arrays and int64 starts expected")
        if mixture_flat.numel() != clean_flat.numel() or mixture.shape != clean.shape or starts.numel() != mixture.shape[0]:
            raise WunetError("crop_windows: shape mismatch")
        B, L = mixture.shape[0], mixture.shape[-1]
        with self._device_guard(mixture.device):
            self._check(self.lib.wunet_crop_windows(mixture_flat.data_ptr(), clean_flat.data_ptr(), starts.data_ptr(), mixture_flat.numel(),
                                                    B, L, mixture.data_ptr(), clean.data_ptr(), self._stream(mixture.device)))

    def mix_windows(self, clean_flat, noise_flat, rows, params, mixture, clean_out, gains=None, peak_limit=0.99):
        """include/wunet_hip.h: wunet_mix_windows.  mixture[b, 0, :] = a (c + g n), clean_out[b, 0, :] = a c for the clean window and the
        circular noise window that rows[b] = (clean start, noise item start, noise item length, noise phase) names, at params[b] =
        (snr_db, linear level); gains (optional float32 [B, 2]) receives (g, a).  Two launches, nothing read back; the scratch comes from
        torch's allocator."""
        given = self._table_op("mix_windows", "mix tensor", "float32 arrays, params, outputs and gains and int64 rows",
                               (clean_flat, noise_flat, rows, params, mixture, clean_out, gains), rows)
        if clean_flat.dim() != 1 or noise_flat.dim() != 1 or mixture.dim() < 2:
            raise WunetError("mix_windows: the two arrays must be flat and the outputs [B, ..., L]")
        B, L = mixture.shape[0], mixture.shape[-1]
        if mixture.shape != clean_out.shape or mixture.numel() != B * L or tuple(rows.shape) != (B, 4) or tuple(params.shape) != (B, 2) or \
                (gains is not None and tuple(gains.shape) != (B, 2)):
            raise WunetError("mix_windows: shape mismatch (rows [B, 4], params [B, 2], gains [B, 2], outputs [B, 1, L])")
        dev = mixture.device
        self._same_device("mix_windows", given, dev, "the outputs' device")
        nbytes = self.lib.wunet_mix_scratch_bytes(B, L)
        if nbytes == 0:
            raise WunetError(f"mix_windows: bad shape (batch={B} length={L})")
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        with self._device_guard(dev):
            self._check(self.lib.wunet_mix_windows(clean_flat.data_ptr(), clean_flat.numel(), noise_flat.data_ptr(), noise_flat.numel(),
                                                   rows.data_ptr(), params.data_ptr(), float(peak_limit), B, L, scratch.data_ptr(),
                                                   mixture.data_ptr(), clean_out.data_ptr(), _ptr(gains), self._stream(dev)))

    def reverb_windows(self, clean_flat, rir_flat, rows, reverberant, direct=None, early_taps=1):
        """include/wunet_hip.h: wunet_reverb_windows.  reverberant[b, 0, :] = the clean window that rows[b] = (window start, clean item
        start, RIR start, RIR taps) names, convolved with its room impulse response (the source is zero in front of the item start);
        direct (optional, the same shape) receives the first min(early_taps, taps) taps' share.  A row with no taps is passed through.
        One launch, nothing read back, no scratch."""
        given = self._table_op("reverb_windows", "reverb tensor", "float32 arrays and outputs and int64 rows",
                               (clean_flat, rir_flat, rows, reverberant, direct), rows)
        if clean_flat.dim() != 1 or rir_flat.dim() != 1 or reverberant.dim() < 2:
            raise WunetError("reverb_windows: the two arrays must be flat and the outputs [B, ..., L]")
        B, L = reverberant.shape[0], reverberant.shape[-1]
        if reverberant.numel() != B * L or tuple(rows.shape) != (B, 4) or (direct is not None and direct.shape != reverberant.shape):
            raise WunetError("reverb_windows: shape mismatch (rows [B, 4], outputs [B, 1, L])")
        dev = reverberant.device
        self._same_device("reverb_windows", given, dev, "the outputs' device")
        with self._device_guard(dev):
            self._check(self.lib.wunet_reverb_windows(clean_flat.data_ptr(), clean_flat.numel(), rir_flat.data_ptr(), rir_flat.numel(),
                                                      rows.data_ptr(), int(early_taps), B, L, reverberant.data_ptr(), _ptr(direct),
                                                      self._stream(dev)))

    def apply_level(self, src, gains, dst=None):
        """include/wunet_hip.h: wunet_apply_level.  dst[b] = gains[b, 1] * src[b] for the [B, 2] gains table that mix_windows wrote - the
        multiply that made its clean_out.  dst None: in place.  Returns dst."""
        dst = src if dst is None else dst
        given = self._table_op("apply_level", "apply_level tensor", "float32 src, gains and dst", (src, gains, dst), None)
        if src.dim() < 2:
            raise WunetError("apply_level: shape mismatch (src and dst [B, ..., L], gains [B, 2])")
        B, L = src.shape[0], src.shape[-1]
        if src.numel() != B * L or dst.shape != src.shape or tuple(gains.shape) != (B, 2):
            raise WunetError("apply_level: shape mismatch (src and dst [B, ..., L], gains [B, 2])")
        self._same_device("apply_level", given, src.device, "one device")
        with self._device_guard(src.device):
            self._check(self.lib.wunet_apply_level(src.data_ptr(), gains.data_ptr(), B, L, dst.data_ptr(), self._stream(src.device)))
        return dst

    def chunk_gather(self, flat, rows, chunks):
        """include/wunet_hip.h: wunet_chunk_gather.  chunks[i, 0, j] = flat[start + s + j] inside the recording that rows[i] = (flat start,
        T, chunk start s) names, 0 outside it.  One launch, nothing read back, no scratch."""
        given = self._table_op("chunk_gather", "chunk_gather tensor", "a float32 array and chunks and int64 rows", (flat, rows, chunks), rows)
        if flat.dim() != 1 or chunks.dim() < 2:
            raise WunetError("chunk_gather: the array must be flat and the chunks [n, ..., L]")
        n, L = chunks.shape[0], chunks.shape[-1]
        if chunks.numel() != n * L or tuple(rows.shape) != (n, 3):
            raise WunetError("chunk_gather: shape mismatch (rows [n, 3], chunks [n, 1, L])")
        dev = chunks.device
        self._same_device("chunk_gather", given, dev, "the chunks' device")
        with self._device_guard(dev):
            self._check(self.lib.wunet_chunk_gather(flat.data_ptr(), flat.numel(), rows.data_ptr(), n, L, chunks.data_ptr(), self._stream(dev)))

    def chunk_overlap_add(self, chunks, recs, out_flat, margin, fade, ramp, max_len):
        """include/wunet_hip.h: wunet_chunk_overlap_add.  out_flat[start + t], t < T, for every recording recs[r] = (flat start, T, first
        chunk row, chunk count): chunk k's sample m + j outside the cross-fades, ramp[j] y_k + (1 - ramp[j]) y_(k-1) inside them.  ramp:
        float32 [fade], None exactly when fade == 0; max_len: the largest T.  One launch, nothing read back, no scratch."""
        given = self._table_op("chunk_overlap_add", "chunk_overlap_add tensor", "float32 chunks, ramp and output and int64 recs",
                               (chunks, recs, out_flat, ramp), recs)
        if out_flat.dim() != 1 or chunks.dim() < 2:
            raise WunetError("chunk_overlap_add: the output must be flat and the chunks [n, ..., L]")
        n, L = chunks.shape[0], chunks.shape[-1]
        margin, fade = int(margin), int(fade)
        if chunks.numel() != n * L or recs.dim() != 2 or recs.shape[1] != 4 or (ramp is not None and tuple(ramp.shape) != (fade,)) or \
                (ramp is None) != (fade == 0):
            raise WunetError("chunk_overlap_add: shape mismatch (chunks [n, 1, L], recs [R, 4], ramp [fade] or None when fade == 0)")
        dev = chunks.device
        self._same_device("chunk_overlap_add", given, dev, "the chunks' device")
        with self._device_guard(dev):
            self._check(self.lib.wunet_chunk_overlap_add(chunks.data_ptr(), n, L, margin, fade, _ptr(ramp), recs.data_ptr(), recs.shape[0],
                                                         int(max_len), out_flat.data_ptr(), out_flat.numel(), self._stream(dev)))

    # ------------------------------------------------------------------ sample-rate conversion (wunet_resample_rows)
    def resample_taps(self, rate_in, rate_out, device):
        """(up, down, the device copy of resample.resample_taps' filter) of one (rate pair, device), made once: on the first (eager)
        call, so that a later graph capture sees no allocation (the rule of stft_basis and stoi_tables)."""
        from .resample import resample_taps
        up, down, h = resample_taps(rate_in, rate_out)
        key = (up, down, str(device))
        taps = self._resample_taps_cache.get(key)
        if taps is None:
            taps = self._resample_taps_cache[key] = torch.from_numpy(h.copy()).to(device)
        return up, down, taps

    def resample_rows(self, flat, rows, out, rate_in, rate_out, max_out):
        """include/wunet_hip.h: wunet_resample_rows.  For every row rows[i] = (in start, T_in, out start, T_out) of the flat float32
        array `flat`, out[out start + m], m < T_out, is the polyphase filter of resample.resample_taps(rate_in, rate_out) over the
        row's T_in samples.  max_out: the largest T_out.  One launch, nothing read back, no scratch."""
        given = self._table_op("resample_rows", "resample_rows tensor", "float32 arrays and int64 rows", (flat, rows, out), rows)
        if flat.dim() != 1 or out.dim() != 1 or rows.dim() != 2 or rows.shape[1] != 4 or rows.shape[0] < 1:
            raise WunetError("resample_rows: shape mismatch (flat arrays in and out, rows [n, 4] with n >= 1)")
        dev = out.device
        self._same_device("resample_rows", given, dev, "one device")
        up, down, taps = self.resample_taps(rate_in, rate_out, dev)
        with self._device_guard(dev):
            self._check(self.lib.wunet_resample_rows(flat.data_ptr(), flat.numel(), rows.data_ptr(), rows.shape[0], int(max_out), up, down,
                                                     taps.data_ptr(), taps.numel(), out.data_ptr(), out.numel(), self._stream(dev)))
        return out

    # ------------------------------------------------------------------ cascades of second-order sections (wunet_sos_windows)
    def sos_tile(self, sections):
        """(tile, chunk) of include/wunet_hip.h: wunet_sos_tile - the samples a block owns per trip and the ones a thread owns."""
        v = self._sized(int(self.lib.wunet_sos_tile(int(sections))))
        return v >> 16, v & 0xffff

    def sos_windows(self, flat, rows, coefs, out, lead=0):
        """include/wunet_hip.h: wunet_sos_windows.  out[b, 0, :] = the window of the flat float32 array `flat` that rows[b] = (window
        start, item start, circular length, phase) names, run through the cascade coefs[b] = [S, 5] (b0, b1, b2, a1, a2 per section,
        a0 = 1) from rest at `lead` samples in front of the window (fewer where the item starts later).  One launch, nothing read back,
        no scratch.  Returns out."""
        given = self._table_op("sos_windows", "sos_windows tensor", "a float32 array, coefs and output and int64 rows", (flat, rows, coefs, out), rows)
        if flat.dim() != 1 or out.dim() < 2 or coefs.dim() != 3:
            raise WunetError("sos_windows: shape mismatch (a flat array, rows [B, 4], coefs [B, S, 5], out [B, ..., L])")
        B, L, S = out.shape[0], out.shape[-1], coefs.shape[1]
        if out.numel() != B * L or tuple(rows.shape) != (B, 4) or tuple(coefs.shape) != (B, S, 5):
            raise WunetError("sos_windows: shape mismatch (a flat array, rows [B, 4], coefs [B, S, 5], out [B, 1, L])")
        dev = out.device
        self._same_device("sos_windows", given, dev, "the output's device")
        with self._device_guard(dev):
            self._check(self.lib.wunet_sos_windows(flat.data_ptr(), flat.numel(), rows.data_ptr(), coefs.data_ptr(), S, int(lead), B, L,
                                                   out.data_ptr(), self._stream(dev)))
        return out

    # ------------------------------------------------------------------ BSS Eval SDR per row (wunet_bss_sdr_*)
    def bss_sdr_tile(self, filter_length=512):
        """include/wunet_hip.h: wunet_bss_sdr_tile - the samples of a row one block of the correlation launch owns."""
        return self._sized(int(self.lib.wunet_bss_sdr_tile(int(filter_length))))

    def bss_sdr(self, clean, estimate, filter_length=512, lengths=None, out=None):
        """include/wunet_hip.h: wunet_bss_sdr_forward.  The last dimension is the utterance, all leading ones are flattened.  lengths:
        None, or an int64 tensor of one entry per row on the waveforms' device (clamped to [0, T] on the device).  Returns float32
        [rows] in dB (`out`, where given); NaN on a row whose reference or estimate is silent or whose length is 0.  Nothing is read
        back to the host."""
        R, T, dev = self._wave_pair("bss_sdr", clean, estimate, "estimate")
        if out is not None:
            self._require(out, "out")
            if out.dtype != torch.float32 or out.numel() != R or out.device != dev:
                raise WunetError(f"bss_sdr: out must be a float32 tensor of {R} elements on {dev}")
        if lengths is not None:
            if not isinstance(lengths, torch.Tensor) or lengths.dtype is not torch.int64:
                raise WunetError("bss_sdr: lengths must be an int64 tensor")
            if lengths.device != dev:
                raise WunetError(f"bss_sdr: lengths lives on {lengths.device}, the waveforms on {dev}")
            if lengths.numel() != R or not lengths.is_contiguous():
                raise WunetError(f"bss_sdr: lengths must be contiguous with one entry per row ({R}), got {tuple(lengths.shape)}")
        n = int(filter_length)
        scratch = torch.empty(self._sized(self.lib.wunet_bss_sdr_scratch_bytes(R, T, n)) // 8, dtype=torch.float64, device=dev)
        out = torch.empty(R, dtype=torch.float32, device=dev) if out is None else out
        with self._device_guard(dev):
            self._check(self.lib.wunet_bss_sdr_forward(clean.data_ptr(), estimate.data_ptr(), R, T, _ptr(lengths), n, scratch.data_ptr(),
                                                       out.data_ptr(), self._stream(dev)))
        return out


class _CtxHold:
    """`with engine._using(shape...) as handle`: the context cannot be evicted while the block runs."""

    def __init__(self, engine, key, ent):
        self.engine, self.key, self.ent = engine, key, ent

    def __enter__(self):
        return self.ent[0]

    def __exit__(self, *a):
        self.engine._release(self.ent)
        return False


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_DEFAULT = None
_DEFAULT_LOCK = threading.Lock()


def default_engine():
    global _DEFAULT
    with _DEFAULT_LOCK:
        if _DEFAULT is None:
            _DEFAULT = Engine()
    return _DEFAULT
