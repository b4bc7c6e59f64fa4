"""ctypes binding of libuse_hip.so (C ABI: include/use_hip.h).

There is no CPU fallback: if the shared library is missing or fails to load, importing the product path
raises -- build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make -C
universal_speech_enhancement_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("USE_HIP_LIB") or os.path.join(_HERE, "libuse_hip.so")   # USE_HIP_LIB: same-box A/B of two builds

PREC = {"fp32": 0, "bf16": 1, "fp16": 2}
PREDICTORS = {"reverse_diffusion": 0, "euler_maruyama": 1, "none": 2}
CORRECTORS = {"none": 0, "langevin": 1, "ald": 2}


class UseConfig(C.Structure):
    _fields_ = [("nf", C.c_int), ("n_levels", C.c_int), ("ch_mult", C.c_int * 8), ("num_res_blocks", C.c_int),
                ("n_freq", C.c_int), ("precision", C.c_int), ("theta", C.c_float), ("sigma_min", C.c_float),
                ("sigma_max", C.c_float), ("input_channels", C.c_int), ("unconditional", C.c_int),
                ("no_sigma_scale", C.c_int)]


class UseSamplerConfig(C.Structure):
    _fields_ = [("N", C.c_int), ("predictor", C.c_int), ("corrector", C.c_int), ("corrector_steps", C.c_int),
                ("snr", C.c_float), ("t_eps", C.c_float), ("use_graph", C.c_int)]


class UseOdeConfig(C.Structure):
    _fields_ = [("rtol", C.c_float), ("atol", C.c_float), ("t_eps", C.c_float), ("N", C.c_int), ("group", C.c_int), ("denoise", C.c_int),
                ("first_step", C.c_float), ("max_step", C.c_float), ("max_nfe", C.c_int), ("use_graph", C.c_int)]


class UseConvCase(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("B", "H", "W", "C0", "C1", "Cout", "XC0", "XC1", "act", "gn", "temb", "res", "stats",
                                       "dtype", "variant", "iters")]


class UseConvOp(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ("B", "H", "W", "C0", "C1", "Cout", "XC0", "XC1", "ntaps", "act", "dtype", "out_dtype", "variant")] +
                [(k, C.c_void_p) for k in ("src0", "src1", "coef", "w", "bias", "temb", "x0", "x1", "w2", "res")] +
                [("out_scale", C.c_float), ("out", C.c_void_p), ("stats", C.c_void_p)] +
                [(k, C.c_void_p) for k in ("pyr", "w4", "b4", "gn_st0", "gn_st1", "gn_gamma", "gn_beta")] +
                [("gn_groups", C.c_int), ("gn_eps", C.c_float), ("temb_bstride", C.c_int)] +
                [("stats_part", C.c_void_p), ("stats_parts", C.c_int)])


class UseTraceTensor(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("dims", C.c_int * 4), ("dtype", C.c_int)]


TRACE_KINDS = {1: "temb", 2: "pack_input", 3: "conv", 4: "fir_down", 5: "fir_up", 6: "gn_finalize", 7: "attn_fused", 8: "attn_core",
               9: "combine_add", 10: "score_out", 11: "transpose", 12: "attn_gemm", 13: "softmax_rows"}     # USE_TRACE_*
TRACE_PARAMS = ("w", "b", "w2", "b2", "gn_w", "gn_b", "cb_w", "cb_b", "dense_w", "dense_b", "x0", "x1", "x2", "x3", "x4", "x5")   # USE_TP_*


class UseTraceEntry(C.Structure):
    _fields_ = [("kind", C.c_int), ("kernel", C.c_char * 32), ("inp", UseTraceTensor * 6), ("out", UseTraceTensor * 2),
                ("totals_in", C.c_void_p * 2), ("part_in", C.c_void_p * 2), ("parts_in", C.c_int * 2),
                ("totals_out", C.c_void_p), ("part_out", C.c_void_p), ("parts_out", C.c_int),
                ("coef", C.c_void_p), ("coef_out", C.c_void_p),
                ("tembias", C.c_void_p), ("temb_row", C.c_int), ("temb_stride", C.c_int),
                ("t", C.c_void_p), ("t_stride", C.c_int),
                ("act", C.c_int), ("out_scale", C.c_float), ("ntaps", C.c_int),
                ("gn_groups", C.c_int), ("gn_inv_n", C.c_float), ("gn_eps", C.c_float),
                ("params", C.c_char_p * len(TRACE_PARAMS))]


SAMPLER_TRACE_KINDS = {1: "prior", 2: "score", 3: "langevin_norms", 4: "langevin_step", 5: "corrector", 6: "predictor",
                       7: "copy_mean"}                                                                     # USE_STRACE_*


class UseSamplerTraceEntry(C.Structure):
    _fields_ = [("kind", C.c_int), ("i", C.c_int), ("k", C.c_int), ("d", C.c_int), ("t", C.c_float),
                ("std1", C.c_float), ("c_drift", C.c_float), ("c_score", C.c_float), ("c_noise", C.c_float), ("step_host", C.c_float),
                ("items", C.c_int), ("n_per_item", C.c_int64), ("blocks_per_b", C.c_int), ("per_item", C.c_int),
                ("x_in", C.c_void_p), ("score", C.c_void_p), ("step", C.c_void_p), ("x_out", C.c_void_p), ("x_mean", C.c_void_p),
                ("noise", C.c_void_p)]


CLIP_KINDS = {"none": 0, "hard": 1, "hard_on_rate": 2, "soft": 3, "sigmoid1": 4, "sigmoid2": 5, "sox": 6, "pedal": 7}      # USE_CLIP_*
VOLUME_MODES = {"none": 0, "peak": 1, "rms": 2}                                                                        # USE_VOLUME_*
DISTORT_SCALARS = ("noise_scale", "clip_threshold", "volume_scale", "norm_factor", "clip_scale", "p_clean", "p_noise", "energy_scale")


class UseDistortParams(C.Structure):
    _fields_ = ([(k, C.c_int) for k in ("reverb", "rir_len", "add_noise", "n_loud", "clip_kind", "dc", "packet_frame", "volume", "normalize",
                                        "reserved")] +
                [("packet_off", C.c_longlong), ("snr_lin", C.c_double), ("loud", C.c_double * 5), ("clip_a", C.c_double),
                 ("clip_b", C.c_double), ("dc_offset", C.c_double), ("volume_target", C.c_double)])


class UseHipError(RuntimeError):
    pass


_lib = None

# every symbol declared in include/use_hip.h: (restype, argtypes)
_vp, _i, _i64, _u64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_float
SYMBOLS = {
    "use_set_option": (C.c_int, [C.c_char_p, C.c_longlong]),
    "use_last_error": (C.c_char_p, []),
    "use_version": (C.c_char_p, []),
    "use_create": (_i, [C.POINTER(UseConfig), _i, C.POINTER(_vp)]),
    "use_destroy": (_i, [_vp]),
    "use_set_weight": (_i, [_vp, C.c_char_p, _vp, C.POINTER(_i64), _i]),
    "use_commit_weights": (_i, [_vp]),
    "use_alloc_weight_blob": (_i, [_vp]),
    "use_weight_blob": (_i, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "use_save_weight_blob": (C.c_int, [C.c_void_p, C.c_char_p]),
    "use_load_weight_blob": (C.c_int, [C.c_void_p, C.c_char_p]),
    "use_num_expected_weights": (_i, [_vp]),
    "use_expected_weight": (_i, [_vp, _i, C.POINTER(C.c_char_p), C.POINTER(_i64), C.POINTER(_i)]),
    "use_plan": (_i, [_vp, _i, _i]),
    "use_workspace_bytes": (_i, [_vp, C.POINTER(C.c_size_t)]),
    "use_score": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "use_forward": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "use_forward_items": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "use_score2": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "use_sample_cond2": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "use_sample_items": (_i, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_u64), _vp, _vp]),
    "use_set_sampler": (_i, [_vp, C.POINTER(UseSamplerConfig)]),
    "use_num_noise_draws": (_i, [_vp]),
    "use_get_timesteps": (_i, [_vp, C.POINTER(_f), _i]),
    "use_sample": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "use_sample_cond": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _vp]),
    "use_set_ode": (_i, [_vp, C.POINTER(UseOdeConfig)]),
    "use_sample_ode": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, C.POINTER(_i), C.POINTER(_i), _vp]),
    "use_ode_create": (_i, [_vp, _i, _i64, C.POINTER(UseOdeConfig), C.POINTER(_vp)]),
    "use_ode_start": (_i, [_vp, _vp, _vp, _vp]),
    "use_ode_request": (_i, [_vp, _vp, _vp, _vp]),
    "use_ode_supply": (_i, [_vp, _vp, _i, _vp]),
    "use_ode_result": (_i, [_vp, _vp, C.POINTER(_i), C.POINTER(_i), _vp]),
    "use_ode_state": (_i, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp]),
    "use_ode_num_groups": (_i, [_vp]),
    "use_ode_destroy": (_i, [_vp]),
    "use_spec_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_float, C.c_float, _vp]),
    "use_spec_back": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_float, C.c_float, _vp]),
    "use_stft_fwd": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, C.c_float, C.c_float, _vp]),
    "use_istft_back": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, C.c_float, C.c_float, _vp]),
    "use_stft_fwd_items": (_i, [_vp, _i64, C.POINTER(_i), _vp, _i, _i, _i, _vp, _i, C.c_float, C.c_float, _vp]),
    "use_istft_back_items": (_i, [_vp, _vp, _i64, C.POINTER(_i), _i, _i, _i, _vp, _i, C.c_float, C.c_float, _vp]),
    "use_chunk_count": (_i, [_i, _i, _i]),
    "use_chunk_split": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "use_chunk_merge": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "use_metrics_workspace": (C.c_size_t, [_i, _i]),
    "use_metrics": (_i, [_vp, _vp, _vp, C.POINTER(_i), _i, _i, _vp, C.c_size_t, _vp, _vp]),
    "use_wav_handoff_workspace": (C.c_size_t, [_i, _i64]),
    "use_wav_handoff": (_i, [_vp, _vp, _i64, C.POINTER(_i), _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
    "use_spec_losses_workspace": (C.c_size_t, [_i, _i64, _i]),
    "use_spec_losses": (_i, [_vp, _vp, C.POINTER(_i), _i, _i64, _i, _vp, C.c_size_t, _vp, _vp]),
    "use_stoi_workspace": (C.c_size_t, [_i, _i64, _i]),
    "use_stoi": (_i, [_vp, _vp, C.POINTER(_i), _i, _i64, _i, _vp, C.c_size_t, _vp, _vp]),
    "use_distort_workspace": (C.c_size_t, [_i64, _i64]),
    "use_distort": (_i, [_vp, _vp, _vp, _vp, _i64, C.POINTER(_i), C.POINTER(_i), C.POINTER(UseDistortParams), _i, _i64, _i64, _i64, _i, _vp, _vp,
                         _vp, _vp, _i64, _vp, C.c_size_t, _vp]),
    "use_sde_prior": (_i, [_vp, _vp, _vp, _u64, _vp, _i64, _vp]),
    "use_fill_noise": (_i, [_vp, _u64, _i, _vp, _i64, _vp]),
    "use_fill_noise_items": (_i, [_vp, C.POINTER(_u64), _i, _i, _vp, _i64, _vp]),
    "use_sde_predictor": (_i, [_vp, _i, _f, _i, _vp, _vp, _vp, _vp, _u64, _vp, _vp, _i64, _vp]),
    "use_sde_corrector": (_i, [_vp, _i, _f, _f, _i, _vp, _vp, _vp, _u64, _vp, _vp, _i64, _vp]),
    "use_debug_tensor": (_i, [_vp, C.c_char_p, C.POINTER(_vp), C.POINTER(_i), C.POINTER(_i)]),
    "use_trace_count": (_i, [_vp]),
    "use_trace_entry_get": (_i, [_vp, _i, C.POINTER(UseTraceEntry)]),
    "use_sampler_trace_count": (_i, [_vp]),
    "use_sampler_trace_get": (_i, [_vp, _i, C.POINTER(UseSamplerTraceEntry)]),
    "use_flops_per_score": (C.c_double, [_vp]),
    "use_get_stat": (_i, [_vp, C.c_char_p, C.POINTER(C.c_longlong)]),
    "use_profile_aux": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "use_profile_aux_flops": (_i, [_vp, _i, C.POINTER(C.c_double)]),
    "use_profile_score": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(C.c_double)]),
    "use_timesteps": (_i, [_i, _f, C.POINTER(_f)]),
    "use_conv_bench": (_i, [C.POINTER(UseConvCase), _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "use_op_conv": (_i, [C.POINTER(UseConvOp), _vp]),
    "use_conv_choice": (_i, [C.POINTER(UseConvOp), C.c_char_p, _i, C.POINTER(_i)]),
    "use_op_conv_dev_workspace": (C.c_size_t, [C.POINTER(UseConvOp)]),
    "use_op_conv_dev": (_i, [C.POINTER(UseConvOp), _i, _vp, C.c_size_t, _vp]),
    "use_op_fir": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "use_op_attention": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "use_op_attention_gemm_workspace": (C.c_size_t, [_i, _i, _i, _i]),
    "use_op_attention_gemm": (_i, [_vp, _vp, _vp, _vp, _vp, C.c_size_t, _i, _i, _i, _i, _i, _vp]),
    "use_op_gn_finalize": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _f, _vp, _i, _vp]),
    "use_op_gn_finalize_parts": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _f, _vp, _i, _vp]),
    "use_op_attn_block": (_i, [_vp, _vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "use_op_combine_add": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _i, _i64, _i, _vp]),
    "use_op_temb_mlp": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "use_op_temb_dense": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "use_op_score_out": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i64, _f, _vp]),
    "use_op_pack_input": (_i, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "use_op_softmax_rows": (_i, [_vp, _i, _i64, _i, _vp]),
    "use_op_transpose_nc": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "use_op_wgrad_workspace": (C.c_size_t, [_i, _i, _i, _i, _i, _i, _i]),
    "use_op_wgrad": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, C.c_size_t, _vp]),
    "use_op_gn_workspace": (C.c_size_t, [_i, _i, _i]),
    "use_op_gn_act_bwd": (_i, [_vp, _vp, _i, _vp, _vp, _i, _f, _i, _vp, _f, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "use_op_gn_act_fwd": (_i, [_vp, _i, _vp, _vp, _i, _f, _i, _i, _i, _i, _vp, _vp, _vp]),
    "use_op_colsum": (_i, [_vp, _i, _i, _i, _i, _f, _vp, _vp, _vp]),
    "use_op_attention_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "use_op_dense_bwd": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "use_wav_read": (_i, [C.c_char_p, C.POINTER(C.POINTER(C.c_double)), C.POINTER(_i64), C.POINTER(_i), C.POINTER(_i)]),
    "use_wav_write": (_i, [C.c_char_p, _vp, _i64, _i, _i, _i]),
    "use_resample_fft": (_i, [_vp, _i64, _i64, _vp]),
    "use_load_utterance": (_i, [C.c_char_p, _i, _i, C.POINTER(C.POINTER(C.c_float)), C.POINTER(_i64), C.POINTER(_i)]),
    "use_load_utterance_peak": (_i, [C.c_char_p, _i, _i, C.POINTER(C.POINTER(C.c_float)), C.POINTER(_i64), C.POINTER(_i), C.POINTER(C.c_double)]),
    "use_wav_info": (_i, [C.c_char_p, C.POINTER(_i64), C.POINTER(_i), C.POINTER(_i)]),
    "use_resampled_length": (_i64, [_i64, _i, _i]),
    "use_free": (None, [_vp]),
    "use_resample_workspace": (C.c_size_t, [_i64, _i64]),
    "use_resample_fft_dev": (_i, [_vp, _i64, _i64, _vp, _vp, C.c_size_t, _vp]),
    "use_load_items_dev": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp]),
    "use_load_items_dev_peak": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp, _vp]),
    "use_store_workspace": (C.c_size_t, [_i64, _i64]),
    "use_store_items_dev": (_i, [_vp, _i64, C.POINTER(_i), C.POINTER(_i64), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp]),
    "use_store_items_dev_gain": (_i, [_vp, _i64, C.POINTER(_i), C.POINTER(_i64), C.POINTER(C.c_double), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp]),
    "use_wav_write_pcm16": (_i, [C.c_char_p, _vp, _i64, _i, _i]),
    "use_load_files_workspace": (C.c_size_t, [_i64, _i64, _i]),
    "use_load_files_dev": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp]),
    "use_store_files_dev": (_i, [_vp, _i64, C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i), C.POINTER(_i64), _i, _i, _vp, _vp, C.c_size_t, _vp]),
    "use_load_files_dev_peak": (_i, [C.POINTER(_vp), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i), _i, _i, _vp, _i64, _vp, C.c_size_t, _vp, _vp]),
    "use_store_files_dev_gain": (_i, [_vp, _i64, C.POINTER(_i), C.POINTER(_i64), C.POINTER(_i), C.POINTER(_i64), C.POINTER(C.c_double), _i, _i, _vp, _vp,
                                      C.c_size_t, _vp]),
    "use_wav_handoff_files_workspace": (C.c_size_t, [_i, _i64]),
    "use_wav_handoff_files": (_i, [_vp, _vp, _i64, C.POINTER(_i), C.POINTER(_i), _i, _i, _i, _vp, C.c_size_t, _vp, _vp]),
}


def lib() -> C.CDLL:
    """Load (once) and return the shared library with typed prototypes; raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise UseHipError(
                f"{LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()). "
                "There is no CPU fallback for the sampling path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            if os.environ.get("USE_HIP_LIB") and not hasattr(L, name):
                continue               # an older build under A/B test may lack the newest entry points
            fn = getattr(L, name)  # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        # USE_HIP_OPTS="name=value,...": use_set_option calls at load time (A/B runs of the test suite and the bench with an option flipped);
        # applied BEFORE the library is published: a bad entry fails every lib() call, not only the first
        for kv in filter(None, os.environ.get("USE_HIP_OPTS", "").split(",")):
            k, sep, v = kv.partition("=")
            if not sep or not k.strip():
                raise UseHipError(f"USE_HIP_OPTS: entry {kv!r} is not name=value")
            try:
                iv = int(v)
            except ValueError:
                raise UseHipError(f"USE_HIP_OPTS: {kv!r}: the value must be an integer") from None
            if L.use_set_option(k.strip().encode(), iv) < 0:
                raise UseHipError(f"USE_HIP_OPTS: {kv}: " + L.use_last_error().decode(errors="replace"))
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> int:
    if rc < 0:
        msg = lib().use_last_error().decode(errors="replace")
        raise UseHipError(f"{what or 'libuse_hip'} failed ({rc}): {msg}")
    return rc
