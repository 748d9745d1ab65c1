"""ctypes binding of liboasr.so (include/oasr.h).  The product path has NO fallback: if the HIP library is missing
or cannot be loaded every entry point raises (the driver's "native code not loaded" check must never be fooled)."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# OASR_LIB: A/B a differently built library of the SAME ABI (kernel experiments); never a fallback.
LIB_PATH = os.environ.get("OASR_LIB") or os.path.join(_HERE, "liboasr.so")
_lib = None


class NativeError(RuntimeError):
    pass


class Dims(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                       "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class Operand(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("ld", C.c_int64), ("rpb", C.c_int), ("bstride", C.c_int64), ("lead", C.c_int),
                ("kvalid", C.c_int), ("trail_from", C.c_int)]


class GemmArgs(C.Structure):
    _fields_ = [("A", Operand), ("B", Operand), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("ta", C.c_int),
                ("tb", C.c_int), ("alpha", C.c_float), ("bias", C.c_void_p), ("act", C.c_int), ("pos", C.c_void_p),
                ("pos_period", C.c_int), ("dgelu_u", C.c_void_p), ("ldu", C.c_int64), ("resid", C.c_void_p),
                ("ldr", C.c_int64), ("out", C.c_void_p), ("out_pre", C.c_void_p), ("ldc", C.c_int64),
                ("out_f32", C.c_void_p), ("ldc32", C.c_int64), ("beta", C.c_float), ("colsum", C.c_void_p), ("atomic", C.c_int),
                ("split_k", C.c_int), ("dgelu_deriv", C.c_int)]


class AttnArgs(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("ldq", C.c_int64), ("ldk", C.c_int64),
                ("ldv", C.c_int64), ("bsq", C.c_int64), ("bsk", C.c_int64), ("bsv", C.c_int64), ("o", C.c_void_p),
                ("ldo", C.c_int64), ("bso", C.c_int64), ("lse", C.c_void_p), ("o_lo", C.c_void_p), ("kv_len", C.c_void_p), ("B", C.c_int),
                ("H", C.c_int), ("Tq", C.c_int), ("Tk", C.c_int), ("causal", C.c_int), ("d_o", C.c_void_p),
                ("delta", C.c_void_p), ("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p), ("dq_colsum", C.c_void_p),
                ("dv_colsum", C.c_void_p), ("colsum_scratch", C.c_void_p), ("qtile_flags", C.c_void_p),
                ("q_rows", C.c_void_p), ("k_rows", C.c_void_p), ("q_span", C.c_void_p),
                ("qblk128", C.c_void_p), ("qblk256", C.c_void_p), ("n128", C.c_int), ("n256", C.c_int)]


class AlignArgs(C.Structure):  # include/oasr.h: oasr_align_args
    MAX_LAYERS = 32  # OASR_ALIGN_MAX_LAYERS
    _fields_ = [("qk", C.c_void_p * 32), ("head_mask", C.c_uint32 * 32), ("n_layers", C.c_int32), ("H", C.c_int32), ("n_tok", C.c_int32),
                ("Tk", C.c_int32), ("n_frames", C.c_int32), ("medfilt_width", C.c_int32), ("qk_scale", C.c_float), ("reserved", C.c_int32),
                ("out", C.c_void_p), ("ldo", C.c_int64)]


class SpecAug(C.Structure):  # include/oasr.h: oasr_specaug
    MAX_MASKS = 8  # OASR_SPECAUG_MAX_MASKS
    _fields_ = [("freq_masks", C.c_int32), ("freq_width", C.c_int32), ("time_masks", C.c_int32), ("time_width", C.c_int32), ("fill", C.c_float)]


class EditArgs(C.Structure):  # include/oasr.h: oasr_edit_args
    MAX_LEN = 1023  # OASR_EDIT_MAX_LEN
    _fields_ = [("hyp", C.c_void_p), ("ref", C.c_void_p), ("hyp_len", C.c_void_p), ("ref_len", C.c_void_p), ("out", C.c_void_p),
                ("ld_hyp", C.c_int64), ("ld_ref", C.c_int64), ("B", C.c_int32), ("Lh", C.c_int32), ("Lr", C.c_int32), ("reserved", C.c_int32)]


class ScoreArgs(C.Structure):  # include/oasr.h: oasr_score_args
    _fields_ = [(n, C.c_void_p) for n in ("mel", "xa", "tokens", "targets", "text_len", "span", "row_nll", "pred", "nll_sum", "nll_max", "n_tok",
                                          "n_hit")] + [("B", C.c_int32), ("S", C.c_int32)]


class BeamArgs(C.Structure):  # include/oasr.h: oasr_beam_args
    MAX_BEAM = 15  # OASR_BEAM_MAX
    NOT_FULL = 0x7fffffff  # OASR_BEAM_NOT_FULL
    _fields_ = [(n, C.c_void_p) for n in ("top_logprob", "top_token", "tokens_in", "tokens_out", "sums", "sources", "last_token", "pool_tokens",
                                          "pool_len", "pool_score", "pool_count", "pool_full_len", "short_step")] + \
               [(n, C.c_int32) for n in ("n_audio", "beam", "max_candidates", "n_ctx", "len", "reserved")] + [("eot", C.c_int64)]


class Speed(C.Structure):  # include/oasr.h: oasr_speed
    MAX_FACTORS = 8  # OASR_SPEED_MAX_FACTORS
    _fields_ = [("n_factors", C.c_int32), ("P", C.c_int32 * 8), ("Q", C.c_int32 * 8)]


class SpeedArgs(C.Structure):  # include/oasr.h: oasr_speed_args
    MAX_N = 1 << 26
    _fields_ = [("pcm_in", C.c_void_p), ("pcm_out", C.c_void_p), ("n_valid", C.c_void_p), ("n_out", C.c_void_p), ("factor_out", C.c_void_p),
                ("tokens_a", C.c_void_p), ("tokens_b", C.c_void_p), ("ld_in", C.c_int64), ("ld_out", C.c_int64), ("ld_tokens_a", C.c_int64),
                ("ld_tokens_b", C.c_int64), ("seed", C.c_uint64), ("first_clip", C.c_uint64), ("B", C.c_int32), ("N", C.c_int32),
                ("S", C.c_int32), ("ts_begin", C.c_int32), ("ts_max", C.c_int32), ("policy", Speed)]


class Noise(C.Structure):  # include/oasr.h: oasr_noise
    NONE = -128  # OASR_NOISE_NONE
    SNR_MIN, SNR_MAX = -10, 50
    _fields_ = [("prob_q16", C.c_int32), ("snr_lo_db", C.c_int32), ("snr_hi_db", C.c_int32)]


class NoiseArgs(C.Structure):  # include/oasr.h: oasr_noise_args
    MAX_N, MAX_ROWS = 1 << 26, 65535
    _fields_ = [("pcm_in", C.c_void_p), ("pcm_out", C.c_void_p), ("n_valid", C.c_void_p), ("bank", C.c_void_p), ("row_out", C.c_void_p),
                ("snr_out", C.c_void_p), ("gain_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
                ("ld_in", C.c_int64), ("ld_out", C.c_int64), ("ld_bank", C.c_int64), ("seed", C.c_uint64), ("first_clip", C.c_uint64),
                ("B", C.c_int32), ("N", C.c_int32), ("M", C.c_int32), ("L", C.c_int32), ("policy", Noise), ("reserved", C.c_int32)]


class Reverb(C.Structure):  # include/oasr.h: struct oasr_reverb
    _fields_ = [("prob_q16", C.c_int32)]


class ReverbArgs(C.Structure):  # include/oasr.h: oasr_reverb_args
    MAX_N, MAX_ROWS, MAX_K, TAP_MAX = 1 << 26, 65535, 8192, 32639
    _fields_ = [("pcm_in", C.c_void_p), ("pcm_out", C.c_void_p), ("n_valid", C.c_void_p), ("rir", C.c_void_p), ("delay", C.c_void_p),
                ("row_out", C.c_void_p), ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t), ("ld_in", C.c_int64), ("ld_out", C.c_int64),
                ("ld_rir", C.c_int64), ("seed", C.c_uint64), ("first_clip", C.c_uint64), ("B", C.c_int32), ("N", C.c_int32), ("R", C.c_int32),
                ("K", C.c_int32), ("policy", Reverb), ("reserved", C.c_int32)]


class Telephone(C.Structure):  # include/oasr.h: struct oasr_telephone
    MAX_CODECS = 8  # OASR_TELEPHONE_MAX_CODECS
    LINEAR, MULAW, ALAW = 0, 1, 2  # OASR_TELEPHONE_LINEAR, _MULAW, _ALAW
    BP_TAPS, UP_TAPS = 129, 32  # the tables of oasr_telephone_tables
    _fields_ = [("prob_q16", C.c_int32), ("n_codecs", C.c_int32), ("codecs", C.c_int32 * 8), ("bandpass", C.c_int32)]


class TelephoneArgs(C.Structure):  # include/oasr.h: oasr_telephone_args
    MAX_N, MAX_ROWS = 1 << 26, 65535
    _fields_ = [("pcm_in", C.c_void_p), ("pcm_out", C.c_void_p), ("n_valid", C.c_void_p), ("codec_out", C.c_void_p), ("ld_in", C.c_int64),
                ("ld_out", C.c_int64), ("seed", C.c_uint64), ("first_clip", C.c_uint64), ("B", C.c_int32), ("N", C.c_int32),
                ("policy", Telephone), ("reserved", C.c_int32)]


class TrainStepArgs(C.Structure):  # include/oasr.h: oasr_train_step_args
    _fields_ = [(n, C.c_void_p) for n in ("mel", "xa", "tokens", "targets", "text_len", "span_host", "mel_clip_max", "loss_out", "logits_out",
                                          "pred_out", "seg_events")] + \
               [(n, C.c_int32) for n in ("B", "S", "span_forward", "accumulate_loss")] + [("loss_scale", C.c_float), ("inv_accum", C.c_float)] + \
               [("label_smoothing", C.c_float), ("z_loss", C.c_float), ("loss_parts_out", C.c_void_p), ("loss_parts_rows", C.c_void_p)]


DTW_MAX_N, DTW_MAX_M = 448, 1500  # csrc/dtw_core.h: the model's n_text_ctx / n_audio_ctx
# (sizeof entry, struct) that lib() holds a library to.  Features that only add entry points, or grow a struct at its end, keep
# ABI_VERSION: a library built before them lacks the sizeof entry or answers another size, and is refused all the same.
STRUCT_SIZES = [
    ("oasr_sizeof_attn_args", AttnArgs),  # checked before anything is declared; last grown by the query-block tables (qblk128 .. n256)
    ("oasr_sizeof_align_args", AlignArgs),  # came with the word-timestamp operators (oasr_alignment_matrix, oasr_dtw)
    ("oasr_sizeof_specaug", SpecAug),  # came with oasr_spec_augment
    ("oasr_sizeof_edit_args", EditArgs),  # came with oasr_edit_counts and oasr_test_argmax_rows
    ("oasr_sizeof_beam_args", BeamArgs),  # came with oasr_beam_update and oasr_decode_reorder
    ("oasr_sizeof_speed", Speed),  # came with oasr_speed_perturb
    ("oasr_sizeof_speed_args", SpeedArgs),
    ("oasr_sizeof_noise", Noise),  # came with oasr_noise_mix
    ("oasr_sizeof_noise_args", NoiseArgs),
    ("oasr_sizeof_reverb", Reverb),  # came with oasr_reverb
    ("oasr_sizeof_reverb_args", ReverbArgs),
    ("oasr_sizeof_telephone", Telephone),  # came with oasr_telephone
    ("oasr_sizeof_telephone_args", TelephoneArgs),
    ("oasr_sizeof_train_step_args", TrainStepArgs),  # last grown by label_smoothing / z_loss / loss_parts_*
    ("oasr_sizeof_score_args", ScoreArgs),  # came with oasr_score, oasr_score_rows and oasr_score_reduce
]
ABI_VERSION = 216  # include/oasr.h: OASR_ABI_VERSION (216: one fused training step, oasr_train_step(oasr_train_step_args), in place of the six positional fused-step entries; 215: oasr_test_* unit operators of the glue kernels, include/oasr_testing.h; 214: staged autograd entries, oasr_train_encode / _decode / _dec_fwd_bwd; 213: LoRA adapters, oasr_create_ex3; 212: oasr_set_trainable; 211: the KV cache's control tail is OASR_KV_TAIL_BYTES; 210: OASR_ERETRY from oasr_decode_check)
KV_TAIL_BYTES = 327680  # include/oasr.h: OASR_KV_TAIL_BYTES
# The tail's layout in 32-bit words (csrc/decode_step_core.h; tests/test_native_abi.py holds these mirrors to that header): the control words,
KV_TEAM_COUNTER, KV_ERROR, KV_TEAM_EPOCH, KV_XCC_MASK, KV_WIDE_EPOCH, KV_CTRL_WORDS = 0, 1, 2, 3, 4, 5
# ... and the chip-wide engine's per-workgroup phase flags: replica r (one per XCC) starts at word KV_FLAGS_WORD + r * KV_FLAG_STRIDE
KV_REPLICAS, KV_FLAG_STRIDE, KV_FLAGS_WORD = 8, 1024, 1024
MODE_INFER, MODE_TRAIN, MODE_TRAIN_ENC, MODE_TRAIN_DEC = 0, 1, 2, 3  # include/oasr.h: OASR_MODE_* (oasr_workspace_bytes)
ROWTAB = 16        # include/oasr.h: OASR_ROWTAB (entries per sample of a chunk-row table)
LORA_MAX_RANK = 64  # include/oasr.h: OASR_LORA_MAX_RANK


def _declare(lib):
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
    sig = {
        "oasr_last_error": (C.c_char_p, []),
        "oasr_version": (i32, []),
        "oasr_log_mel_workspace_bytes": (sz, [i32]),
        "oasr_log_mel": (i32, [vp, i32, i32, i32, vp, vp, vp]),
        "oasr_mel_filterbank": (i32, [vp]),
        "oasr_create": (vp, [C.POINTER(Dims)]),
        "oasr_create_ex": (vp, [C.POINTER(Dims), i32]),
        "oasr_create_ex2": (vp, [C.POINTER(Dims), i32, i32]),
        "oasr_compute_dtype": (i32, [vp]),
        "oasr_create_ex3": (vp, [C.POINTER(Dims), i32, i32, vp, i32, i32, f32]),
        "oasr_lora_count": (i32, [vp]),
        "oasr_lora_merge": (i32, [vp, vp]),
        "oasr_lora_merge_op": (i32, [vp, vp, vp, i32, i32, i32, f32, i32, vp, vp]),
        "oasr_lora_grad_scratch_bytes": (sz, [i32, i32, i32]),
        "oasr_lora_grad_op": (i32, [vp, vp, vp, i32, i32, i32, f32, vp, vp, vp, vp]),
        "oasr_encode": (i32, [vp, vp, i32, vp, vp, sz, vp]),
        "oasr_kv_cache_bytes": (sz, [vp, i32]),
        "oasr_decode_step_workspace_bytes": (sz, [vp, i32]),
        "oasr_decode_begin": (i32, [vp, vp, i32, vp, vp]),
        "oasr_decode_step": (i32, [vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        "oasr_decode_check": (i32, [vp, i32, vp, vp]),
        "oasr_decode_logits": (i32, [vp, vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]),
        "oasr_destroy": (None, [vp]),
        "oasr_param_count": (i32, [vp]),
        "oasr_param_info": (i32, [vp, i32, C.c_char_p, i32, C.POINTER(i64), C.POINTER(i64), C.POINTER(i32), C.POINTER(i64)]),
        "oasr_param_numel": (i64, [vp]),
        "oasr_segment_count": (i32, [vp]),
        "oasr_segment_info": (i32, [vp, i32, C.POINTER(i64), C.POINTER(i64)]),
        "oasr_bind": (i32, [vp, vp, vp, vp, vp, vp]),
        "oasr_shadow_bytes": (sz, [vp]),
        "oasr_bind_shadow": (i32, [vp, vp]),
        "oasr_refresh_shadow": (i32, [vp, vp]),
        "oasr_workspace_bytes": (sz, [vp, i32, i32, i32]),
        "oasr_forward": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]),
        "oasr_sizeof_train_step_args": (sz, []),
        "oasr_train_step": (i32, [vp, C.POINTER(TrainStepArgs), vp, sz, vp]),
        "oasr_log_mel_raw": (i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
        "oasr_sizeof_attn_args": (sz, []),
        "oasr_test_span_tables": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp]),
        "oasr_test_span_block_tables": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]),
        "oasr_test_embedding_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, vp]),
        "oasr_test_embedding_bwd": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i64, i64, vp, vp, vp]),
        "oasr_test_colsum": (i32, [vp, i32, i64, i64, i32, vp, vp]),
        "oasr_test_conv2_col2im_dgelu": (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
        "oasr_test_conv1_col2im_mel": (i32, [vp, i32, vp, i32, i32, i32, vp]),
        "oasr_test_mel_to_time_major": (i32, [vp, vp, i32, i32, i32, i32, vp, vp]),
        "oasr_test_pack_conv_weight": (i32, [vp, vp, i32, i32, i32, i32, vp]),
        "oasr_test_unpack_conv_grad": (i32, [vp, vp, i32, i32, i32, vp]),
        "oasr_test_pack_embedding": (i32, [vp, vp, i32, i32, i32, vp]),
        "oasr_test_dgelu_mul": (i32, [vp, vp, vp, i32, i64, vp]),
        "oasr_test_dlogits_from_f32": (i32, [vp, i32, i64, i64, vp, i32, vp]),
        "oasr_test_logits_to_f32": (i32, [vp, i32, i64, i64, i32, vp, vp]),
        "oasr_test_layernorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, vp]),
        "oasr_train_fwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "oasr_train_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "oasr_zero_grad": (i32, [vp, vp]),
        "oasr_train_encode": (i32, [vp, vp, i32, vp, vp, sz, vp]),
        "oasr_train_encode_bwd": (i32, [vp, vp, i32, vp, vp, sz, vp]),
        "oasr_train_decode": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "oasr_train_decode_bwd": (i32, [vp, vp, vp, vp, i32, i32, vp, vp, sz, vp]),
        "oasr_set_trainable": (i32, [vp, vp, i32]),
        "oasr_optim_step": (i32, [vp, f32, f32, f32, f32, f32, f32, f32, i64, vp, vp, vp]),
        "oasr_grad_sumsq_range": (i32, [vp, i64, i64, vp, vp, vp]),
        "oasr_optim_step_range": (i32, [vp, i64, i64, vp, vp, vp, f32, f32, f32, f32, f32, f32, f32, i64, vp]),
        "oasr_gemm": (i32, [C.POINTER(GemmArgs), vp]),
        "oasr_test_gemm": (i32, [C.POINTER(GemmArgs), vp, i32, i32, i32, i32, vp]),
        "oasr_profile_gemm_records": (i32, [C.c_char_p, i32]),
        "oasr_gemm_route_debug": (i32, [i32] * 11 + [i32, C.c_longlong, C.c_longlong, C.c_longlong] + [i32] * 6 + [C.c_char_p, i32, C.POINTER(i32)]),
        "oasr_train_wgrad_plan_debug": (i32, [C.c_longlong, i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "oasr_train_block_needs_debug": (i32, [i32]),
        "oasr_layernorm_fwd": (i32, [vp, vp, vp, vp, vp, vp, i64, i32, vp]),
        "oasr_layernorm_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp]),
        "oasr_attention_fwd": (i32, [C.POINTER(AttnArgs), vp]),
        "oasr_attention_bwd": (i32, [C.POINTER(AttnArgs), vp]),
        "oasr_attention_scores": (i32, [C.POINTER(AttnArgs), i32, vp, vp]),
        "oasr_sizeof_align_args": (sz, []),
        "oasr_alignment_workspace_bytes": (sz, [i32, i32, i32]),
        "oasr_alignment_matrix": (i32, [C.POINTER(AlignArgs), vp, sz, vp]),
        "oasr_dtw_workspace_bytes": (sz, [i32, i32]),
        "oasr_dtw": (i32, [vp, i64, i32, i32, i32, vp, vp, vp, vp, sz, vp]),
        "oasr_test_dtw_host": (i32, [vp, i64, i32, i32, i32, vp, vp, vp, vp]),
        "oasr_sizeof_specaug": (sz, []),
        "oasr_spec_augment": (i32, [vp, i32, i32, i32, C.POINTER(SpecAug), C.c_uint64, C.c_uint64, vp]),
        "oasr_spec_augment_plan": (i32, [C.POINTER(SpecAug), C.c_uint64, C.c_uint64, i32, i32, vp, vp]),
        "oasr_sizeof_edit_args": (sz, []),
        "oasr_edit_counts": (i32, [C.POINTER(EditArgs), vp]),
        "oasr_edit_counts_host": (i32, [C.POINTER(EditArgs)]),
        "oasr_sizeof_score_args": (sz, []),
        "oasr_score": (i32, [vp, C.POINTER(ScoreArgs), vp, sz, vp]),
        "oasr_score_rows": (i32, [vp, i32, i64, i32, vp, vp, i32, i32, i64, vp, vp, vp]),
        "oasr_score_reduce": (i32, [vp, vp, vp, vp, i32, i32, i32, i64, vp, vp, vp, vp, vp]),
        "oasr_score_reduce_host": (i32, [vp, vp, vp, vp, i32, i32, i32, i64, vp, vp, vp, vp]),
        "oasr_sizeof_beam_args": (sz, []),
        "oasr_beam_update": (i32, [C.POINTER(BeamArgs), vp]),
        "oasr_beam_update_host": (i32, [C.POINTER(BeamArgs)]),
        "oasr_decode_reorder": (i32, [vp, vp, i32, i32, i32, vp, vp, vp]),
        "oasr_decode_reorder_host": (i32, [vp, i64, i32, i32, i32, i32, i32, i32, i32, vp]),
        "oasr_sizeof_speed": (sz, []),
        "oasr_sizeof_speed_args": (sz, []),
        "oasr_speed_perturb": (i32, [C.POINTER(SpeedArgs), vp]),
        "oasr_speed_perturb_host": (i32, [C.POINTER(SpeedArgs)]),
        "oasr_speed_plan": (i32, [C.POINTER(Speed), C.c_uint64, C.c_uint64, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "oasr_speed_table": (i32, [i32, i32, vp, C.POINTER(i32)]),
        "oasr_sizeof_noise": (sz, []),
        "oasr_sizeof_noise_args": (sz, []),
        "oasr_noise_workspace_bytes": (sz, [i32, i32]),
        "oasr_noise_mix": (i32, [C.POINTER(NoiseArgs), vp]),
        "oasr_noise_mix_host": (i32, [C.POINTER(NoiseArgs)]),
        "oasr_noise_plan": (i32, [C.POINTER(Noise), C.c_uint64, C.c_uint64, i32, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
        "oasr_sizeof_reverb": (sz, []),
        "oasr_sizeof_reverb_args": (sz, []),
        "oasr_reverb_workspace_bytes": (sz, [i32, i32]),
        "oasr_reverb": (i32, [C.POINTER(ReverbArgs), vp]),
        "oasr_reverb_host": (i32, [C.POINTER(ReverbArgs)]),
        "oasr_reverb_plan": (i32, [C.POINTER(Reverb), C.c_uint64, C.c_uint64, i32, C.POINTER(i32), C.POINTER(i32)]),
        "oasr_sizeof_telephone": (sz, []),
        "oasr_sizeof_telephone_args": (sz, []),
        "oasr_telephone": (i32, [C.POINTER(TelephoneArgs), vp]),
        "oasr_telephone_host": (i32, [C.POINTER(TelephoneArgs)]),
        "oasr_telephone_plan": (i32, [C.POINTER(Telephone), C.c_uint64, C.c_uint64, C.POINTER(i32), C.POINTER(i32)]),
        "oasr_telephone_tables": (i32, [vp, vp]),
        "oasr_telephone_quantize_host": (i32, [vp, vp, i64, i32]),
        "oasr_test_argmax_rows": (i32, [vp, i32, i64, i32, i64, vp, vp, i32, i32, vp, vp]),
        "oasr_cross_entropy": (i32, [vp, i64, i32, vp, i64, i64, f32, vp, vp, vp, i32, vp]),
        "oasr_cross_entropy_ex": (i32, [vp, i64, i32, vp, i64, i64, f32, vp, vp, vp, i32, f32, f32, vp, vp]),
        "oasr_test_cross_entropy": (i32, [vp, i32, i64, i32, vp, i64, i64, f32, vp, vp, vp, i32, f32, f32, vp, vp]),
        "oasr_cast_f32_bf16": (i32, [vp, vp, i64, vp]),
        "oasr_pick_tokens": (i32, [vp, i64, i32, i64, vp, vp, vp, vp, vp]),
        "oasr_pick_tokens_ts": (i32, [vp, i64, i32, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, vp, vp, vp]),
        "oasr_topk_tokens": (i32, [vp, i64, i32, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp, vp]),
        "oasr_sample_tokens": (i32, [vp, i64, i32, i64, vp, vp, vp, i64, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp]),
        "oasr_probe_tr16": (i32, [vp, vp, vp]),
        "oasr_probe_lds_oob": (i32, [vp, vp, vp]),
        "oasr_profile_gemm": (i32, [i32]),
        "oasr_gemm_force_general": (i32, [i32]),
        "oasr_gemm_set_stagger": (i32, [i32, i32]),
        "oasr_gemm_set_variant": (i32, [i32]),
        "oasr_decode_set_ln_fold": (i32, [i32]),
        "oasr_span_set_side_streams": (i32, [i32]),
        "oasr_span_side_streams": (i32, []),
        "oasr_xcd_plan_debug": (i32, [i32, i32, i32, i32, i32, i32, i32, vp, i32]),
        "oasr_xcd_offsets_ok_debug": (i32, [vp, C.c_longlong, C.c_longlong, i32, i32, i32, i32]),
        "oasr_wide_supports_debug": (i32, [i32, i32, i32, i32, i32, i32, i32, i32]),
        "oasr_wide_plan_debug": (i32, [i32, i32, i32, i32, i32, i32, vp, i32]),
        "oasr_attention_set_pingpong": (i32, [i32]),
        "oasr_attention_set_span_grid": (i32, [i32]),
        "oasr_profile_gemm_collect": (i32, [vp, vp, vp, C.c_char_p, i32]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return list(sig)


EXPORTS = None


def _check_struct_size(handle, entry, struct):
    size = getattr(handle, entry, lambda: None)()  # (a library from before the struct was passed lacks the entry)
    if size != C.sizeof(struct):
        raise NativeError(f"{LIB_PATH}: {entry} answers {size} bytes, this binding's {struct.__name__} has {C.sizeof(struct)} "
                          "-- rebuild (__graft_entry__.build())")


def lib():
    """Loads liboasr.so (once).  Raises NativeError when it is missing -- build it with __graft_entry__.build()."""
    global _lib, EXPORTS
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise NativeError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU/PyTorch fallback for this path.")
        try:
            _lib = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise NativeError(f"cannot load {LIB_PATH}: {e}") from e
        handle, _lib = _lib, None  # published only once it has passed every check below (a failed load must not leave a half-declared CDLL behind)
        # a library of another ABI generation reads structs of a different size through the same pointers, and may lack symbols this
        # binding declares: check the version FIRST (oasr_version exists in every generation), then the first struct size, then declare
        ver = getattr(handle, "oasr_version", lambda: None)()
        if ver != ABI_VERSION:
            raise NativeError(f"{LIB_PATH}: ABI version {ver}, this binding is written for version {ABI_VERSION} -- rebuild (__graft_entry__.build())")
        _check_struct_size(handle, *STRUCT_SIZES[0])
        try:
            exports = _declare(handle)
        except AttributeError as e:
            raise NativeError(f"{LIB_PATH} (ABI {ver}) lacks an entry point this binding declares: {e} -- rebuild (__graft_entry__.build())") from e
        for row in STRUCT_SIZES[1:]:
            _check_struct_size(handle, *row)
        _lib, EXPORTS = handle, exports
    return _lib


def enable_testing_hooks():
    """Opt this process in to the kernel-selection setters of include/oasr_testing.h (they are inert otherwise)."""
    os.environ["OASR_TESTING_HOOKS"] = "1"


ERETRY = -4  # include/oasr.h: OASR_ERETRY


def check(rc, what=""):
    if rc != 0:
        msg = lib().oasr_last_error()
        raise NativeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device (or host) address of a tensor; None -> NULL."""
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


STREAM = object()  # call(): stands for the current stream of the call's device
_Tensor = torch.Tensor


def call(name, *args, device=None):
    """``lib().<name>(*args)`` for an entry that returns a status code, checked under the entry's own name.  A tensor argument becomes
    its address (None stays NULL), ``STREAM`` the current stream of the call's device; everything else -- numbers, ctypes values,
    ``C.byref(struct)`` -- passes through.  The call's device is ``device`` (a tensor's ``.device``: entries whose addresses travel inside
    a struct give it) or else the device of the CUDA tensor arguments, which must agree; the entry runs with that device current.  CPU
    tensors pass as addresses and name no device (the ``*_host`` entries, ``span_host``).  No synchronisation and no allocation."""
    fn = getattr(_lib or lib(), name)
    argv, stream_at = [], -1
    for a in args:
        if isinstance(a, _Tensor):
            if a.is_cuda:
                if device is None:
                    device = a.device
                elif a.device != device:
                    raise NativeError(f"{name}: arguments on {device} and on {a.device} -- one call, one device (nothing was launched)")
            a = a.data_ptr()
        elif a is STREAM:
            stream_at = len(argv)
        argv.append(a)
    if device is None:
        if stream_at >= 0:
            raise NativeError(f"{name}: a stream was asked for, but no argument names a device")
        rc = fn(*argv)
    else:
        with torch.cuda.device(device):
            if stream_at >= 0:
                argv[stream_at] = torch.cuda.current_stream().cuda_stream
            rc = fn(*argv)
    if rc != 0:
        check(rc, name)


def require_gpu(t, name="tensor"):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise NativeError(f"{name} must be a CUDA/HIP tensor: the MI355X-native path has no CPU fallback")
