"""ctypes binding of csrc/libwunet_hip.so (the C ABI of include/wunet_hip.h).

There is deliberately no fallback: if the HIP library is missing or fails to load the import
raises, so a GPU box can never silently run something else.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (WUNET_LIB_PATH: measurement builds of the same library, e.g. kernel ablations - never set in production)
LIB_PATH = os.environ.get("WUNET_LIB_PATH") or os.path.join(_HERE, "csrc", "libwunet_hip.so")

EXPORTS = [
    "wunet_last_error", "wunet_create", "wunet_destroy", "wunet_workspace_bytes", "wunet_forward",
    "wunet_backward", "wunet_backward_range", "wunet_loss_scratch_bytes", "wunet_loss_forward",
    "wunet_loss_backward", "wunet_layer_info", "wunet_num_conv_layers", "wunet_op_conv1d",
    "wunet_op_conv1d_dgrad", "wunet_op_conv1d_wgrad", "wunet_profile_enable", "wunet_profile_collect",
    "wunet_adam_step", "wunet_set_h3", "wunet_op_conv1d_split", "wunet_op_conv1d_dgrad_split", "wunet_op_conv1d_wgrad_split",
    "wunet_op_conv1d_bf16", "wunet_op_conv1d_dgrad_bf16", "wunet_op_conv1d_wgrad_bf16",
    "wunet_backward_range_async", "wunet_backward_join", "wunet_debug_set_conv_trace", "wunet_crop_windows",
    "wunet_comm_unique_id", "wunet_comm_create", "wunet_comm_allreduce_sum", "wunet_comm_world", "wunet_comm_destroy",
    "wunet_debug_stamps", "wunet_set_bn_frozen", "wunet_backward_input", "wunet_adam_scratch_bytes", "wunet_adam_step_ex",
    "wunet_loss_rows_scratch_bytes", "wunet_loss_rows_forward", "wunet_loss_rows_backward",
    "wunet_stft_basis_bytes", "wunet_stft_basis", "wunet_stft_scratch_bytes", "wunet_stft_saved_bytes", "wunet_stft_forward",
    "wunet_stft_finalize", "wunet_stft_backward",
    "wunet_cspec_scratch_bytes", "wunet_cspec_saved_bytes", "wunet_cspec_forward", "wunet_cspec_finalize", "wunet_cspec_backward",
    "wunet_mel_scratch_bytes", "wunet_mel_saved_bytes", "wunet_mel_forward", "wunet_mel_finalize", "wunet_mel_backward",
    "wunet_stoi_tables_bytes", "wunet_stoi_tables_build", "wunet_stoi_scratch_bytes", "wunet_stoi_forward",
    "wunet_stoi_loss_scratch_bytes", "wunet_stoi_loss_saved_bytes", "wunet_stoi_loss_forward", "wunet_stoi_loss_backward",
    "wunet_estoi_scratch_bytes", "wunet_estoi_forward",
    "wunet_estoi_loss_scratch_bytes", "wunet_estoi_loss_saved_bytes", "wunet_estoi_loss_forward", "wunet_estoi_loss_backward",
    "wunet_mix_scratch_bytes", "wunet_mix_windows", "wunet_apply_level", "wunet_reverb_windows",
    "wunet_chunk_gather", "wunet_chunk_overlap_add", "wunet_resample_rows", "wunet_resample_tile",
    "wunet_sos_windows", "wunet_sos_tile",
    "wunet_bss_sdr_scratch_bytes", "wunet_bss_sdr_forward", "wunet_bss_sdr_tile",
]

_vp = ctypes.c_void_p
_i = ctypes.c_int
_sz = ctypes.c_size_t


def declare(lib):
    """Attach argtypes/restypes to a loaded library object (HIP build or the test emulator build)."""
    lib.wunet_last_error.restype = ctypes.c_char_p
    lib.wunet_last_error.argtypes = []
    lib.wunet_create.argtypes = [_i, _i, _i, _i, ctypes.POINTER(_vp)]
    lib.wunet_destroy.argtypes = [_vp]
    lib.wunet_destroy.restype = None
    lib.wunet_workspace_bytes.argtypes = [_vp, _i]
    lib.wunet_workspace_bytes.restype = _sz
    lib.wunet_forward.argtypes = [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]
    lib.wunet_backward.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.wunet_backward_range.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.wunet_backward_range_async.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]
    lib.wunet_backward_join.argtypes = [_vp, _vp]
    if hasattr(lib, "wunet_backward_input"):     # (saved libraries of earlier versions do not have it)
        lib.wunet_backward_input.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp]
    lib.wunet_loss_scratch_bytes.restype = _sz
    lib.wunet_loss_scratch_bytes.argtypes = []
    lib.wunet_loss_forward.argtypes = [_i, _vp, _vp, _sz, _vp, _vp, _vp]
    lib.wunet_loss_backward.argtypes = [_i, _vp, _vp, _vp, _sz, _vp, _vp]
    if hasattr(lib, "wunet_loss_rows_forward"):  # (saved libraries of earlier versions do not have it)
        lib.wunet_loss_rows_scratch_bytes.argtypes = [_sz, _sz]
        lib.wunet_loss_rows_scratch_bytes.restype = _sz
        lib.wunet_loss_rows_forward.argtypes = [_i, _i, ctypes.c_double, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _vp, _vp]
        lib.wunet_loss_rows_backward.argtypes = [_i, _vp, _vp, _vp, _vp, _sz, _sz, _vp, _vp]
    if hasattr(lib, "wunet_stft_forward"):       # (saved libraries of earlier versions do not have it)
        lib.wunet_stft_basis_bytes.argtypes = [_i]
        lib.wunet_stft_basis_bytes.restype = _sz
        lib.wunet_stft_basis.argtypes = [_i, _i, _vp, _vp]
        lib.wunet_stft_scratch_bytes.argtypes = [_sz, _sz, _i, _i, _i]
        lib.wunet_stft_scratch_bytes.restype = _sz
        lib.wunet_stft_saved_bytes.argtypes = [_sz, _sz, _i, _i]
        lib.wunet_stft_saved_bytes.restype = _sz
        lib.wunet_stft_forward.argtypes = [_vp, _vp, _sz, _sz, _i, _i, _i, ctypes.c_double, _vp, _vp, _vp, _vp, _vp]
        lib.wunet_stft_finalize.argtypes = [_i, _vp, _sz, _sz, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]
        lib.wunet_stft_backward.argtypes = [_vp, _vp, _vp, _sz, _sz, _i, _i, _i, ctypes.c_double, _vp, _vp, _vp, _i, _vp]
    if hasattr(lib, "wunet_cspec_forward"):      # (saved libraries of earlier versions do not have it)
        lib.wunet_cspec_scratch_bytes.argtypes = [_sz, _sz, _i, _i, _i]
        lib.wunet_cspec_scratch_bytes.restype = _sz
        lib.wunet_cspec_saved_bytes.argtypes = [_sz, _sz, _i, _i]
        lib.wunet_cspec_saved_bytes.restype = _sz
        lib.wunet_cspec_forward.argtypes = [_vp, _vp, _sz, _sz, _i, _i, _i, ctypes.c_double, ctypes.c_double, _vp, _vp, _sz, _vp, _sz, _vp]
        lib.wunet_cspec_finalize.argtypes = [_i, _vp, _sz, _sz, _vp, _vp, ctypes.c_double, _vp, _vp, _vp]
        lib.wunet_cspec_backward.argtypes = [_vp, _sz, _vp, _vp, _sz, _sz, _i, _i, _i, ctypes.c_double, ctypes.c_double, _vp, _vp, _sz, _vp, _i, _vp]
    if hasattr(lib, "wunet_mel_forward"):        # (saved libraries of earlier versions do not have it)
        lib.wunet_mel_scratch_bytes.argtypes = [_sz, _sz, _i, _i, _i]
        lib.wunet_mel_scratch_bytes.restype = _sz
        lib.wunet_mel_saved_bytes.argtypes = [_sz, _sz, _i, _i, _i]
        lib.wunet_mel_saved_bytes.restype = _sz
        lib.wunet_mel_forward.argtypes = [_vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _i, ctypes.c_double, ctypes.c_double, _vp, _vp, _sz, _vp, _sz,
                                          _vp, _vp]
        lib.wunet_mel_finalize.argtypes = [_i, _vp, _sz, _sz, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp, _vp]
        lib.wunet_mel_backward.argtypes = [_vp, _sz, _vp, _vp, _sz, _sz, _i, _i, _i, _i, _vp, _i, ctypes.c_double, ctypes.c_double, _vp, _vp, _sz,
                                           _vp, _i, _vp]
    if hasattr(lib, "wunet_stoi_forward"):       # (saved libraries of earlier versions do not have it)
        lib.wunet_stoi_tables_bytes.argtypes = [_i]
        lib.wunet_stoi_tables_bytes.restype = _sz
        lib.wunet_stoi_tables_build.argtypes = [_i, _vp, _sz, _vp, _vp]
        lib.wunet_stoi_scratch_bytes.argtypes = [_sz, _sz, _i]
        lib.wunet_stoi_scratch_bytes.restype = _sz
        lib.wunet_stoi_forward.argtypes = [_vp, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp, _vp]
    if hasattr(lib, "wunet_stoi_loss_forward"):
        lib.wunet_stoi_loss_scratch_bytes.argtypes = [_sz, _sz, _i]
        lib.wunet_stoi_loss_scratch_bytes.restype = _sz
        lib.wunet_stoi_loss_saved_bytes.argtypes = [_sz, _sz, _i]
        lib.wunet_stoi_loss_saved_bytes.restype = _sz
        lib.wunet_stoi_loss_forward.argtypes = [_vp, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
        lib.wunet_stoi_loss_backward.argtypes = [_vp, _vp, _sz, _sz, _i, _vp, _vp, _vp, _vp]
    if hasattr(lib, "wunet_estoi_forward"):      # (the same; every call has the signature of its wunet_stoi_* counterpart)
        for name in ("scratch_bytes", "forward", "loss_scratch_bytes", "loss_saved_bytes", "loss_forward", "loss_backward"):
            stoi, estoi = getattr(lib, "wunet_stoi_" + name), getattr(lib, "wunet_estoi_" + name)
            estoi.argtypes, estoi.restype = stoi.argtypes, stoi.restype
    lib.wunet_layer_info.argtypes = [_vp, _i, ctypes.POINTER(_sz), ctypes.POINTER(_i), ctypes.POINTER(_i)]
    lib.wunet_num_conv_layers.argtypes = [_vp]
    for name in ("wunet_op_conv1d", "wunet_op_conv1d_split", "wunet_op_conv1d_bf16"):
        getattr(lib, name).argtypes = [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]
    for name in ("wunet_op_conv1d_dgrad", "wunet_op_conv1d_wgrad", "wunet_op_conv1d_dgrad_split", "wunet_op_conv1d_wgrad_split",
                 "wunet_op_conv1d_dgrad_bf16", "wunet_op_conv1d_wgrad_bf16"):
        getattr(lib, name).argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]
    lib.wunet_adam_step.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.c_double, ctypes.c_longlong, ctypes.c_double, _vp, _vp, _vp]
    if hasattr(lib, "wunet_adam_step_ex"):       # (saved libraries of earlier versions do not have it)
        lib.wunet_adam_scratch_bytes.argtypes = [_i]
        lib.wunet_adam_scratch_bytes.restype = _sz
        lib.wunet_adam_step_ex.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           ctypes.c_double, ctypes.c_longlong, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                           _vp, _vp, _vp, _vp, _vp]
    lib.wunet_set_h3.argtypes = [_vp, _i]
    if hasattr(lib, "wunet_set_bn_frozen"):      # (saved libraries of earlier versions - tools/lib_ab.sh - do not have it)
        lib.wunet_set_bn_frozen.argtypes = [_vp, _vp, _i]
    lib.wunet_profile_enable.argtypes = [_i]
    lib.wunet_profile_collect.argtypes = [ctypes.c_char_p, _sz]
    lib.wunet_profile_collect.restype = ctypes.c_longlong
    if hasattr(lib, "wunet_debug_stamps"):       # (a measurement hook of round 6: saved libraries of earlier rounds - tools/round_vs_round.sh - do not have it)
        lib.wunet_debug_stamps.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), _i]
        lib.wunet_debug_stamps.restype = _i
    lib.wunet_crop_windows.argtypes = [_vp, _vp, _vp, ctypes.c_longlong, _i, _i, _vp, _vp, _vp]
    if hasattr(lib, "wunet_mix_windows"):        # (saved libraries of earlier versions do not have it)
        lib.wunet_mix_scratch_bytes.argtypes = [_i, _i]
        lib.wunet_mix_scratch_bytes.restype = _sz
        lib.wunet_mix_windows.argtypes = [_vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp, _vp, ctypes.c_float, _i, _i, _vp, _vp, _vp, _vp, _vp]
    if hasattr(lib, "wunet_reverb_windows"):     # (the same)
        lib.wunet_apply_level.argtypes = [_vp, _vp, _i, _i, _vp, _vp]
        lib.wunet_reverb_windows.argtypes = [_vp, ctypes.c_longlong, _vp, ctypes.c_longlong, _vp, _i, _i, _i, _vp, _vp, _vp]
    if hasattr(lib, "wunet_chunk_gather"):       # (the same)
        _ll = ctypes.c_longlong
        lib.wunet_chunk_gather.argtypes = [_vp, _ll, _vp, _ll, _i, _vp, _vp]
        lib.wunet_chunk_overlap_add.argtypes = [_vp, _ll, _i, _i, _i, _vp, _vp, _ll, _ll, _vp, _ll, _vp]
    if hasattr(lib, "wunet_resample_rows"):      # (the same)
        _ll = ctypes.c_longlong
        lib.wunet_resample_rows.argtypes = [_vp, _ll, _vp, _ll, _ll, _i, _i, _vp, _i, _vp, _ll, _vp]
        lib.wunet_resample_tile.argtypes = [_i, _i, _i]
        lib.wunet_resample_tile.restype = _ll
    if hasattr(lib, "wunet_sos_windows"):        # (the same)
        _ll = ctypes.c_longlong
        lib.wunet_sos_windows.argtypes = [_vp, _ll, _vp, _vp, _i, _i, _i, _i, _vp, _vp]
        lib.wunet_sos_tile.argtypes = [_i]
        lib.wunet_sos_tile.restype = _ll
    if hasattr(lib, "wunet_bss_sdr_forward"):    # (the same)
        lib.wunet_bss_sdr_scratch_bytes.argtypes = [_sz, _sz, _i]
        lib.wunet_bss_sdr_scratch_bytes.restype = _sz
        lib.wunet_bss_sdr_forward.argtypes = [_vp, _vp, _sz, _sz, _vp, _i, _vp, _vp, _vp]
        lib.wunet_bss_sdr_tile.argtypes = [_i]
        lib.wunet_bss_sdr_tile.restype = ctypes.c_longlong
    lib.wunet_comm_unique_id.argtypes = [_vp]
    lib.wunet_comm_create.argtypes = [_vp, _i, _i, ctypes.POINTER(_vp)]
    lib.wunet_comm_allreduce_sum.argtypes = [_vp, _vp, _sz, _vp]
    lib.wunet_comm_world.argtypes = [_vp]
    lib.wunet_comm_destroy.argtypes = [_vp]
    lib.wunet_comm_destroy.restype = None
    lib.wunet_debug_set_conv_trace.argtypes = [_vp]
    lib.wunet_debug_set_conv_trace.restype = None
    return lib


_HIP = None


def load_hip():
    """Load libwunet_hip.so or raise.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
    (or `make -C <package>/csrc -j8`)."""
    global _HIP
    if _HIP is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the MI355X HIP library has not been built "
                "(run `make -C wave-u-net-for-speech-enhancement_amd/csrc -j8`); there is no CPU fallback")
        _HIP = declare(ctypes.CDLL(LIB_PATH))
    return _HIP
