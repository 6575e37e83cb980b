"""ctypes binding of libfastdiff_hip.so (include/fastdiff_hip.h, fastdiff_hip_ext.h, fastdiff_hip_train.h).  No torch types cross this boundary."""
import ctypes as ct
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libfastdiff_hip.so")

FD_OK, FD_ERR_INVALID, FD_ERR_UNSUPPORTED, FD_ERR_HIP, FD_ERR_STATE, FD_ERR_MISSING = 0, -1, -2, -3, -4, -5
FD_RESAMPLE_TILE, FD_RESAMPLE_MAX_RATIO = 256, 1024      # fastdiff_hip_ext.h: outputs per workgroup of fd_resample; widest reduced ratio
FD_PCM_F32, FD_PCM_S16, FD_PCM_S32, FD_PCM_U8 = 0, 1, 2, 3
FD_LOUDNESS_TILE = 16384                                  # fastdiff_hip_ext.h: samples of one utterance per workgroup of the loudness filter
FD_LOUDNESS_OK, FD_LOUDNESS_SHORT, FD_LOUDNESS_SILENT, FD_LOUDNESS_CLIPPED = 0, 1, 2, 3
FD_STOI_SCAN_TILE, FD_STOI_SEG_TILE = 1024, 16            # fastdiff_hip_ext.h: frames per workgroup of fd_stoi_measure's compaction scan; segments per workgroup
FD_STOI_OK, FD_STOI_SHORT, FD_STOI_SILENT = 0, 1, 2
FD_PITCH_MAX_LAGS, FD_PITCH_FRAME_TILE, FD_PITCH_LAG_CHUNK, FD_PITCH_STAGE_FLOATS = 1024, 4, 64, 6144      # fastdiff_hip_ext.h: the largest tau_max + 2; frames per workgroup, lags per wavefront pass and samples staged together of fd_pitch_track
FD_PITCH_OK, FD_PITCH_SHORT, FD_PITCH_UNVOICED = 0, 1, 2
FD_SPECTRAL_MAX_RES, FD_SPECTRAL_FRAME_TILE, FD_SPECTRAL_SUM_CHUNK = 4, 4, 256      # fastdiff_hip_ext.h: resolutions of a configuration; frames per workgroup of fd_spectral_measure's transform stage; interleaved runs of its finaliser
FD_SPECTRAL_OK, FD_SPECTRAL_SHORT = 0, 1
FD_GL_NFFT, FD_GL_HOP, FD_GL_BINS, FD_GL_FRAME_TILE, FD_GL_SUM_CHUNK, FD_GL_MAX_ITERS, FD_GL_MAX_FRAMES, FD_GL_PHILOX_STREAM = 1024, 256, 513, 4, 256, 10000, 1048576, 0xFFFFFFF8      # fastdiff_hip_ext.h: fd_griffin_lim's transform, frames per workgroup, runs of its finaliser, caps, Philox stream word
FD_GL_OK, FD_GL_SHORT, FD_GL_SILENT, FD_GL_NONFINITE = 0, 1, 2, 3
FD_GL_PWG, FD_GL_TACOTRON = 0, 1
FD_NNLS_MAX_ITERS, FD_NNLS_FRAME_TILE = 4096, 32          # fastdiff_hip_ext.h: fd_mel_to_linear_nnls' iteration cap and frames per workgroup
FD_NNLS_OK, FD_NNLS_EMPTY, FD_NNLS_NONFINITE = 0, 1, 2
FD_BINS_CHUNK, FD_BINS_MAX_K, FD_BINS_MAX_D, FD_BINS_RECORD_BYTES = 4096, 128, 128, 1056      # fastdiff_hip_ext.h: rows per workgroup and float32 sum of fd_bins_pass, its caps, sizeof(fd_bins)
FD_BINS_OK, FD_BINS_NONFINITE, FD_BINS_EMPTY = 0, 1, 2
FD_MCD_MAX_COEF, FD_MCD_MAX_FRAMES, FD_DTW_ROWS, FD_DTW_COLS, FD_DTW_MAX_ALIGN_CELLS = 40, 1 << 22, 256, 64, 1 << 26      # fastdiff_hip_ext.h: cepstral coefficients and frames of a row; rows one workgroup of fd_dtw sweeps together, columns it stages together; cells with align_out
FD_MCD_OK, FD_MCD_SHORT, FD_MCD_NONFINITE = 0, 1, 2
FD_TRIM_CHUNK = 256                                       # fastdiff_hip_ext.h: windows of one utterance per pass of fd_trim_silences' mask kernel
FD_TRIM_OK, FD_TRIM_SILENT, FD_TRIM_EMPTY = 0, 1, 2
FD_TRIM_LONG, FD_TRIM_EDGES = 0, 1
FD_PWG_TILE, FD_PWG_PHILOX_STREAM, FD_PWG_MAX_LAYERS, FD_PWG_MAX_DILATION, FD_PWG_MAX_CONTEXT, FD_PWG_MAX_SCALES, FD_PWG_MAX_SCALE, FD_PWG_MAX_HOP, FD_PWG_MAX_FRAMES = 512, 0xFFFFFFF7, 30, 512, 4, 4, 16, 512, 32768      # fastdiff_hip_ext.h: samples per workgroup of fd_pwg_generate's layer kernel, the Philox stream word of its z, the caps of a configuration and of T
FD_PWG_CONV_IN_UPSAMPLE, FD_PWG_UPSAMPLE, FD_PWG_MELGAN = 0, 1, 2


class FdConfig(ct.Structure):
    _fields_ = [("audio_channels", ct.c_int), ("inner_channels", ct.c_int), ("cond_channels", ct.c_int),
                ("n_upsample", ct.c_int), ("upsample_ratios", ct.c_int * 8), ("lvc_layers_each_block", ct.c_int),
                ("lvc_kernel_size", ct.c_int), ("kpnet_hidden_channels", ct.c_int), ("kpnet_conv_size", ct.c_int),
                ("diffusion_step_embed_dim_in", ct.c_int), ("diffusion_step_embed_dim_mid", ct.c_int),
                ("diffusion_step_embed_dim_out", ct.c_int), ("use_weight_norm", ct.c_int)]


class FdStep(ct.Structure):
    _fields_ = [("t", ct.c_float), ("c_eps", ct.c_float), ("c_div", ct.c_float), ("sigma", ct.c_float),
                ("c1", ct.c_float), ("c2", ct.c_float), ("c3", ct.c_float), ("add_noise", ct.c_int32)]


class FdWeightRef(ct.Structure):
    _fields_ = [("name", ct.c_char_p), ("data", ct.c_void_p), ("dims", ct.POINTER(ct.c_int64)), ("ndim", ct.c_int32), ("reserved", ct.c_int32)]


class FdKernelStat(ct.Structure):
    _fields_ = [("name", ct.c_char * 48), ("launches", ct.c_int64), ("total_ms", ct.c_double)]


class FdEmaItem(ct.Structure):
    _fields_ = [("p", ct.c_void_p), ("e", ct.c_void_p), ("numel", ct.c_int64)]


class FdEmaHyper(ct.Structure):
    _fields_ = [("decay", ct.c_double), ("warmup", ct.c_double)]


class FdEmaState(ct.Structure):
    _fields_ = [("updates", ct.c_uint64), ("seen_applied", ct.c_uint64), ("w", ct.c_float), ("apply", ct.c_int32)]


class FdSpan(ct.Structure):
    _fields_ = [("mel", ct.c_void_p), ("mel_pitch", ct.c_int64), ("mel_cap", ct.c_int64), ("mel_first", ct.c_int64),
                ("mel_frames", ct.c_int64), ("utt_frames", ct.c_int64), ("t0", ct.c_int64), ("t1", ct.c_int64),
                ("stream_id", ct.c_uint64), ("out", ct.c_void_p)]


class FdSpanWindow(ct.Structure):
    _fields_ = [("span", ct.c_int32), ("batch", ct.c_int32), ("len", ct.c_int32), ("clen", ct.c_int32), ("start", ct.c_int64),
                ("c0", ct.c_int64)]


class FdRingChunk(ct.Structure):
    _fields_ = [("ring", ct.c_void_p), ("pitch", ct.c_int64), ("cap", ct.c_int64), ("first_frame", ct.c_int64), ("src", ct.c_void_p),
                ("src_pitch", ct.c_int64), ("frames", ct.c_int64)]


class FdTrimParams(ct.Structure):
    _fields_ = [("sample_rate", ct.c_int32), ("window_ms", ct.c_int32), ("average_width", ct.c_int32), ("max_silence", ct.c_int32),
                ("mode", ct.c_int32), ("reserved", ct.c_int32), ("top_db", ct.c_double), ("floor_db", ct.c_double)]


class FdPwgConfig(ct.Structure):
    _fields_ = [(k, ct.c_int32) for k in ("in_channels", "out_channels", "kernel_size", "layers", "stacks", "residual_channels", "gate_channels",
                                          "skip_channels", "aux_channels", "aux_context_window", "bias", "use_causal_conv",
                                          "upsample_conditional_features", "use_pitch_embed", "use_nsf", "upsample_net", "n_scales")] + \
               [("upsample_scales", ct.c_int32 * 8), ("upsample_activation", ct.c_int32), ("interpolate_nearest", ct.c_int32),
                ("freq_axis_kernel_size", ct.c_int32)]


def float_ptr(t):
    """A tensor's or a numpy array's address (None: NULL) as the float pointer the fd_pwg_* entry points declare."""
    if t is None:
        return None
    return ct.cast(t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data, ct.POINTER(ct.c_float))


def step_table(rows):
    """[{t, c_eps, c_div, sigma, c1, c2, c3, add_noise}] (executed first -> last) -> the fd_step array fd_sample takes."""
    steps = (FdStep * len(rows))()
    for k, row in enumerate(rows):
        steps[k] = FdStep(float(row["t"]), float(row["c_eps"]), float(row["c_div"]), float(row["sigma"]),
                          float(row["c1"]), float(row["c2"]), float(row["c3"]), int(row["add_noise"]))
    return steps


EXPORTS = ["fd_default_config", "fd_create", "fd_destroy", "fd_last_error", "fd_set_weight", "fd_commit_weights",
           "fd_forward", "fd_sample", "fd_sample_check", "fd_sample_ticket", "fd_sample_settle", "fd_set_noise_streams", "fd_sample_halo_frames", "fd_sample_span", "fd_sample_spans_plan", "fd_sample_spans", "fd_mel_ring_append", "fd_peak_normalize_int16", "fd_peak_normalize_int16_ragged", "fd_mel_spectrogram", "fd_set_mel_filterbank", "fd_get_mel_filterbank", "fd_resample_out_len", "fd_resample_taps", "fd_resample", "fd_loudness_design", "fd_loudness_blocks", "fd_loudness_measure", "fd_loudness_normalize", "fd_stoi_bands", "fd_stoi_frames", "fd_stoi_measure", "fd_pitch_default_config", "fd_pitch_lags", "fd_pitch_frames", "fd_pitch_track", "fd_pitch_compare", "fd_spectral_default_config", "fd_spectral_frames", "fd_spectral_measure", "fd_gl_samples", "fd_gl_default_iters", "fd_mel_to_linear", "fd_griffin_lim", "fd_nnls_default_iters", "fd_nnls_step_bound", "fd_mel_to_linear_nnls", "fd_bins_chunk", "fd_bins_record_bytes", "fd_bins_pass", "fd_mcd_default_config", "fd_mcd_frames", "fd_cepstra", "fd_dtw", "fd_mcd_measure", "fd_trim_default_params", "fd_trim_windows", "fd_trim_mask", "fd_trim_levels", "fd_trim_silences", "fd_pwg_default_config", "fd_pwg_samples", "fd_pwg_receptive_field", "fd_pwg_create", "fd_pwg_set_weight", "fd_pwg_commit", "fd_pwg_set_scaler", "fd_pwg_generate", "fd_pwg_draw", "fd_pwg_destroy", "fd_lvc_forward", "fd_lvc_backward", "fd_lvc_forward_strided", "fd_lvc_backward_strided", "fd_gate_forward", "fd_gate_backward", "fd_kconv_forward", "fd_kconv_backward", "fd_weight_norm_multi_forward", "fd_weight_norm_multi_backward", "fd_refresh_weights_device", "fd_get_weight_image", "fd_get_weight_flags", "fd_pack_source", "fd_fan_forward", "fd_fan_backward", "fd_input_conv_forward", "fd_input_conv_backward", "fd_kconv_backward_w_multi", "fd_kconv_forward_act_multi", "fd_kconv_backward_x_multi", "fd_input_conv_forward_multi", "fd_input_conv_backward_multi", "fd_kconv_forward_act", "fd_kconv_backward_act", "fd_kconv_forward_frames", "fd_kconv_backward_frames", "fd_lvc_forward_frames", "fd_lvc_backward_frames", "fd_conv32_forward", "fd_conv32_backward", "fd_weight_norm_forward", "fd_weight_norm_backward", "fd_conv7_forward", "fd_conv7_backward", "fd_upsample_forward", "fd_upsample_backward", "fd_train_draw", "fd_train_collate", "fd_eval_collate", "fd_item_distance", "fd_eval_accumulate", "fd_mse_forward", "fd_mse_backward", "fd_adamw_multi", "fd_ema_multi", "fd_bandpool_forward", "fd_bandpool_backward", "fd_npred_head_forward", "fd_npred_head_backward", "fd_phi_draw", "fd_phi_residual_forward", "fd_sched_init", "fd_sched_begin", "fd_sched_update", "fd_set_option", "fd_read_tap", "fd_kernel_index", "fd_bias_index",
           "fd_get_profile", "fd_reset_profile", "fd_get_counter", "fd_version", "fd_abi_revision"]

_lib = None


class FastDiffHipError(RuntimeError):
    pass


def load():
    """dlopen the HIP library.  Fails loudly: there is no Python/CPU fallback for the compute path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FastDiffHipError(
            f"{LIB_PATH} is missing: build it with `python -m fastdiff_amd.build` (hipcc, gfx950). "
            "fastdiff_amd has no CPU fallback.")
    lib = ct.CDLL(LIB_PATH)
    vp, ci, cf = ct.c_void_p, ct.c_int, ct.c_float  # noqa: F841
    lib.fd_version.restype = ct.c_char_p
    lib.fd_last_error.restype = ct.c_char_p
    lib.fd_last_error.argtypes = [vp]
    lib.fd_default_config.argtypes = [ct.POINTER(FdConfig)]
    lib.fd_create.argtypes = [ct.POINTER(FdConfig), ci, ct.POINTER(vp)]
    lib.fd_destroy.argtypes = [vp]
    lib.fd_set_weight.argtypes = [vp, ct.c_char_p, vp, ct.POINTER(ct.c_int64), ci]
    lib.fd_commit_weights.argtypes = [vp]
    lib.fd_refresh_weights_device.argtypes = [vp, ct.POINTER(FdWeightRef), ci, vp]
    lib.fd_get_weight_image.argtypes = [vp, vp, ct.POINTER(ct.c_size_t)]
    lib.fd_get_weight_flags.argtypes = [vp, ct.POINTER(ct.c_uint)]
    lib.fd_pack_source.argtypes = [ct.c_char_p, ci, ci, ci]
    lib.fd_forward.argtypes = [vp, vp, vp, vp, ci, ci, vp, vp, vp]
    lib.fd_sample.argtypes = [vp, vp, ci, ci, vp, ct.POINTER(FdStep), ci, ci, vp, vp, ct.c_uint64, vp, vp, vp]
    lib.fd_set_noise_streams.argtypes = [vp, vp, ci]
    lib.fd_sample_halo_frames.argtypes = [ci]
    i64, u64 = ct.c_int64, ct.c_uint64
    lib.fd_sample_span.argtypes = [vp, vp, i64, i64, i64, i64, i64, ct.POINTER(FdStep), ci, ci, vp, vp, u64, u64, ci, vp, vp]
    lib.fd_sample_spans_plan.argtypes = [ct.POINTER(FdSpan), ci, ci, ci, ct.POINTER(FdSpanWindow), ci, ct.POINTER(ci)]
    lib.fd_sample_spans.argtypes = [vp, ct.POINTER(FdSpan), ci, ct.POINTER(FdStep), ci, ci, u64, ci, vp]
    lib.fd_mel_ring_append.argtypes = [vp, ct.POINTER(FdRingChunk), ci, vp]
    lib.fd_sample_check.argtypes = [vp]
    lib.fd_sample_ticket.argtypes = [vp]
    lib.fd_sample_ticket.restype = ct.c_int64
    lib.fd_sample_settle.argtypes = [vp, ct.c_int64]
    lib.fd_peak_normalize_int16.argtypes = [vp, vp, ci, ct.c_int64, vp, vp]
    lib.fd_peak_normalize_int16_ragged.argtypes = [vp, vp, ci, ct.c_int64, vp, vp, vp]
    lib.fd_mel_spectrogram.argtypes = [vp, vp, ci, ct.c_int64, vp, ci, vp]
    lib.fd_set_mel_filterbank.argtypes = [vp, vp, ci, ci]
    lib.fd_get_mel_filterbank.argtypes = [vp, vp, ci, ci]
    lib.fd_resample_out_len.argtypes = [ct.c_int64, ci, ci]
    lib.fd_resample_out_len.restype = ct.c_int64
    lib.fd_resample_taps.argtypes = [ci, ci, vp, ct.c_int64, ct.POINTER(ci), ct.POINTER(ci), ct.POINTER(ci)]
    lib.fd_resample.argtypes = [vp, vp, ci, ci, ci, ct.c_int64, ct.c_int64, vp, ci, ci, vp, ct.c_int64, vp]
    lib.fd_loudness_design.argtypes = [ci, vp]
    lib.fd_loudness_blocks.argtypes = [ct.c_int64, ci]
    lib.fd_loudness_blocks.restype = ct.c_int64
    lib.fd_loudness_measure.argtypes = [vp, vp, ci, ct.c_int64, vp, ci, vp, vp]
    lib.fd_loudness_normalize.argtypes = [vp, vp, ci, ct.c_int64, vp, ci, ct.c_double, vp, vp, vp, vp]
    lib.fd_stoi_bands.argtypes = [vp, vp]
    lib.fd_stoi_frames.argtypes = [ct.c_int64]
    lib.fd_stoi_frames.restype = ct.c_int64
    lib.fd_stoi_measure.argtypes = [vp, vp, vp, ci, ct.c_int64, vp, ci, vp, vp]
    lib.fd_pitch_default_config.argtypes = [vp]
    lib.fd_pitch_lags.argtypes = [vp, vp, vp]
    lib.fd_pitch_frames.argtypes = [ct.c_int64, ci]
    lib.fd_pitch_frames.restype = ct.c_int64
    lib.fd_pitch_track.argtypes = [vp, vp, ci, ct.c_int64, vp, vp, vp, vp, ct.c_int64, vp]
    lib.fd_pitch_compare.argtypes = [vp, vp, vp, ci, ct.c_int64, vp, vp, vp]
    lib.fd_spectral_default_config.argtypes = [vp]
    lib.fd_spectral_frames.argtypes = [ct.c_int64, ci]
    lib.fd_spectral_frames.restype = ct.c_int64
    lib.fd_spectral_measure.argtypes = [vp, vp, vp, ci, ct.c_int64, vp, vp, vp, vp]
    lib.fd_gl_samples.argtypes = [ct.c_int64]
    lib.fd_gl_samples.restype = ct.c_int64
    lib.fd_gl_default_iters.argtypes = []
    lib.fd_mel_to_linear.argtypes = [vp, vp, ci, ci, vp, ci, vp, vp]
    lib.fd_griffin_lim.argtypes = [vp, vp, vp, ci, ci, vp, ci, ct.c_uint64, vp, vp, ct.c_int64, vp, vp]
    lib.fd_nnls_default_iters.argtypes = []
    lib.fd_nnls_step_bound.argtypes = [vp, ct.POINTER(ct.c_double)]
    lib.fd_mel_to_linear_nnls.argtypes = [vp, vp, ci, ci, vp, vp, vp, ci, ci, vp, vp, vp]
    lib.fd_bins_chunk.argtypes = []
    lib.fd_bins_record_bytes.argtypes = []
    lib.fd_bins_pass.argtypes = [vp, vp, ct.c_int64, ci, ct.c_int64, vp, vp, vp, ci, vp, vp, vp, vp]
    lib.fd_mcd_default_config.argtypes = [vp]
    lib.fd_mcd_frames.argtypes = [ct.c_int64]
    lib.fd_mcd_frames.restype = ct.c_int64
    lib.fd_cepstra.argtypes = [vp, vp, ci, ct.c_int64, vp, ci, vp, ct.c_int64, vp]
    lib.fd_dtw.argtypes = [vp, vp, vp, ci, ci, ct.c_int64, ct.c_int64, ct.c_int64, vp, vp, vp, vp, ct.c_int64, vp]
    lib.fd_mcd_measure.argtypes = [vp, vp, ct.c_int64, vp, ct.c_int64, ci, vp, vp, vp, vp, vp]
    lib.fd_trim_default_params.argtypes = [ci, ct.POINTER(FdTrimParams)]
    lib.fd_trim_windows.argtypes = [ct.c_int64, ci, ci, ct.POINTER(ct.c_int64), ct.POINTER(ct.c_int64)]
    lib.fd_trim_mask.argtypes = [vp, ct.c_int64, ci, ci, ci, vp]
    lib.fd_trim_levels.argtypes = [vp, vp, ci, ct.c_int64, vp, ci, ci, vp, vp]
    lib.fd_trim_silences.argtypes = [vp, vp, ci, ct.c_int64, vp, ct.POINTER(FdTrimParams), vp, vp, vp, vp, vp]
    lib.fd_pwg_default_config.argtypes = [ct.POINTER(FdPwgConfig)]
    lib.fd_pwg_default_config.restype = None
    lib.fd_pwg_samples.argtypes = [ct.POINTER(FdPwgConfig), ct.c_int64]
    lib.fd_pwg_samples.restype = ct.c_int64
    lib.fd_pwg_receptive_field.argtypes = [ct.POINTER(FdPwgConfig)]
    lib.fd_pwg_receptive_field.restype = ct.c_int64
    lib.fd_pwg_create.argtypes = [vp, ct.POINTER(FdPwgConfig), ct.POINTER(vp)]
    # (float pointers, host or device, are declared as such: pwg.py casts tensors' addresses)
    fp = ct.POINTER(ct.c_float)
    lib.fd_pwg_set_weight.argtypes = [vp, ct.c_char_p, fp, ct.c_int64]
    lib.fd_pwg_commit.argtypes = [vp]
    lib.fd_pwg_set_scaler.argtypes = [vp, fp, fp]
    lib.fd_pwg_generate.argtypes = [vp, fp, ci, ci, ci, ct.POINTER(ct.c_int64), fp, ct.c_uint64, ct.POINTER(ct.c_uint64), fp, ct.c_int64, vp]
    lib.fd_pwg_draw.argtypes = [vp, ci, ct.c_int64, ct.c_uint64, ct.POINTER(ct.c_uint64), fp, ct.c_int64, vp]
    lib.fd_pwg_destroy.argtypes = [vp]
    lib.fd_lvc_forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    lib.fd_lvc_backward.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp, vp, vp]
    lib.fd_lvc_forward_strided.argtypes = [vp, vp, vp, ct.c_int64, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    lib.fd_lvc_backward_strided.argtypes = [vp, vp, vp, ct.c_int64, vp, ci, ci, ci, ci, ci, ci, vp, vp, ct.c_int64, vp, vp]
    lib.fd_kconv_forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp]
    lib.fd_kconv_backward.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]
    lib.fd_weight_norm_multi_forward.argtypes = [vp, vp, ci, vp]
    lib.fd_weight_norm_multi_backward.argtypes = [vp, vp, ci, vp]
    lib.fd_fan_forward.argtypes = [vp, vp, ci, ct.c_int64, ci, vp, vp]
    lib.fd_fan_backward.argtypes = [vp, vp, vp, vp, vp, vp, ci, ct.c_int64, ci, vp, vp]
    lib.fd_input_conv_forward.argtypes = [vp, vp, vp, vp, ci, ci, ct.c_float, vp, vp]
    lib.fd_input_conv_backward.argtypes = [vp, vp, vp, vp, vp, ci, ci, ct.c_float, vp, vp, vp, vp]
    lib.fd_kconv_forward_act.argtypes = [vp, vp, vp, vp, ci, ci, ci, ct.c_float, vp, vp]
    lib.fd_kconv_backward_act.argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ct.c_float, ct.c_float, vp, vp, vp, vp]
    lib.fd_kconv_forward_act_multi.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ct.c_float, vp, vp]
    lib.fd_kconv_backward_x_multi.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ci, ct.c_float, ct.c_float, vp, vp]
    lib.fd_input_conv_forward_multi.argtypes = [vp, ci, vp, vp, vp, ci, ci, ct.c_float, vp, vp]
    lib.fd_input_conv_backward_multi.argtypes = [vp, ci, vp, vp, vp, vp, ci, ci, ct.c_float, vp, vp, vp, vp]
    lib.fd_kconv_backward_w_multi.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ct.c_float, vp, vp, vp]
    lib.fd_kconv_forward_frames.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp]
    lib.fd_kconv_backward_frames.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]
    lib.fd_lvc_forward_frames.argtypes = [vp, vp, vp, ct.c_int64, vp, ct.c_int64, ci, ci, ci, vp, vp]
    lib.fd_lvc_backward_frames.argtypes = [vp, vp, vp, ct.c_int64, vp, ci, ci, ci, vp, vp, ct.c_int64, vp, ct.c_int64, vp]
    lib.fd_conv32_forward.argtypes = [vp, vp, vp, vp, vp, ci, ct.c_int64, ci, cf, cf, vp, vp, vp]
    lib.fd_conv32_backward.argtypes = [vp, vp, vp, vp, vp, vp, ci, ct.c_int64, ci, cf, cf, vp, vp, vp, vp]
    lib.fd_conv7_forward.argtypes = [vp, ci, vp, vp, vp, ci, ct.c_int64, vp, vp]
    lib.fd_conv7_backward.argtypes = [vp, ci, vp, vp, vp, ci, ct.c_int64, vp, vp, vp, vp]
    lib.fd_upsample_forward.argtypes = [vp, vp, vp, vp, ci, ct.c_int64, ci, vp, vp]
    lib.fd_upsample_backward.argtypes = [vp, vp, vp, vp, ci, ct.c_int64, ci, vp, vp, vp, vp]
    lib.fd_weight_norm_forward.argtypes = [vp, vp, vp, ct.c_int64, ci, vp, vp, vp]
    lib.fd_weight_norm_backward.argtypes = [vp, vp, vp, vp, vp, ct.c_int64, ci, vp, vp, vp]
    lib.fd_gate_forward.argtypes = [vp, vp, vp, ci, ci, ct.c_int64, vp, vp]
    lib.fd_gate_backward.argtypes = [vp, vp, vp, ci, ci, ct.c_int64, vp, vp]
    lib.fd_train_draw.argtypes = [vp, vp, vp, ci, ci, ct.c_int64, ct.c_uint64, vp, ct.c_uint64, vp, vp, vp, vp]
    lib.fd_train_collate.argtypes = [vp, vp, vp, vp, ct.c_int64, ci, ci, ci, ct.c_uint64, vp, ct.c_uint64, ci, ci, vp, vp, vp, vp]
    lib.fd_eval_collate.argtypes = [vp, vp, vp, vp, ct.c_int64, ci, ci, ci, ct.c_uint64, vp, ct.c_uint64, vp, vp, vp, vp]
    lib.fd_item_distance.argtypes = [vp, vp, vp, ci, ct.c_int64, ci, vp, vp]
    lib.fd_eval_accumulate.argtypes = [vp, vp, vp, vp, ci, ci, ci, vp, vp, vp, vp]
    lib.fd_mse_forward.argtypes = [vp, vp, vp, ct.c_int64, vp, vp, vp]
    lib.fd_mse_backward.argtypes = [vp, vp, vp, vp, ct.c_int64, vp, vp]
    lib.fd_adamw_multi.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.fd_ema_multi.argtypes = [vp, vp, ci, vp, vp, vp, vp]
    lib.fd_bandpool_forward.argtypes = [vp, vp, vp, vp, ci, ct.c_int64, vp, vp]
    lib.fd_bandpool_backward.argtypes = [vp, vp, vp, vp, vp, ci, ct.c_int64, vp, vp, vp]
    lib.fd_npred_head_forward.argtypes = [vp, vp, vp, vp, ci, vp, vp, vp, vp, ci, vp, vp, vp]
    lib.fd_npred_head_backward.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, vp, vp, vp, vp, vp]
    lib.fd_phi_draw.argtypes = [vp, vp, vp, ci, ci, ci, ct.c_int64, ct.c_uint64, vp, ct.c_uint64, vp, vp, vp, vp, vp, vp, vp]
    lib.fd_phi_residual_forward.argtypes = [vp, vp, vp, vp, vp, ci, ct.c_int64, vp, vp, vp]
    lib.fd_sched_init.argtypes = [vp, vp, cf, cf, vp]
    lib.fd_sched_begin.argtypes = [vp, vp, vp, ci, ct.c_double, vp, ci, ci, vp, ci, vp]
    lib.fd_sched_update.argtypes = [vp, vp, vp, vp, ct.c_int64, vp, vp]
    lib.fd_set_option.argtypes = [vp, ct.c_char_p, ct.c_char_p]
    lib.fd_read_tap.argtypes = [vp, ct.c_char_p, vp, ct.c_int64]
    lib.fd_read_tap.restype = ct.c_int64
    lib.fd_kernel_index.argtypes = [ci, ci, ci, ci]
    lib.fd_bias_index.argtypes = [ci, ci]
    lib.fd_get_profile.argtypes = [vp, ct.POINTER(FdKernelStat), ci]
    lib.fd_reset_profile.argtypes = [vp]
    lib.fd_get_counter.argtypes = [vp, ct.c_char_p]
    lib.fd_get_counter.restype = ct.c_int64
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    """Map fd_status to the exception type the reference would raise (SURVEY 8b 'Errors')."""
    if rc >= 0:
        return rc
    msg = lib.fd_last_error(handle)
    msg = msg.decode() if msg else what
    if rc == FD_ERR_INVALID:
        raise AssertionError(msg)
    if rc == FD_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == FD_ERR_MISSING:
        raise KeyError(msg)
    raise FastDiffHipError(f"{what}: {msg} (status {rc})")
