"""ctypes binding of the C ABI in include/ace355.h (csrc/libace355.so).

There is no CPU or PyTorch fallback here: if the library is missing or a call fails, a
``RuntimeError`` carrying ``ace355_last_error()`` is raised (the reference's seam turns backend
exceptions into its PyTorch fallback, handler/service_generate_execute.py:189-191).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_LIB: Optional[C.CDLL] = None
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc", "libace355.so")

OK = 0
DTYPE_F32, DTYPE_BF16 = 0, 1
MAX_BLOCKS = 8
MAX_SLOTS = 32
MAX_SEQS = 64


class DitConfigC(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32), ("num_layers", C.c_int32),
        ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32), ("head_dim", C.c_int32),
        ("sliding_window", C.c_int32), ("patch_size", C.c_int32), ("in_channels", C.c_int32),
        ("out_channels", C.c_int32), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float),
        ("sliding_layer_mask", C.c_uint64),
    ]


class SampleParamsC(C.Structure):
    _fields_ = [
        ("num_steps", C.c_int32), ("t_sched_host", C.POINTER(C.c_float)), ("guidance_scale", C.c_float),
        ("cfg_interval_start", C.c_float), ("cfg_interval_end", C.c_float), ("infer_method", C.c_int32),
        ("use_adg", C.c_int32), ("cond_slot", C.c_int32), ("null_slot", C.c_int32),
        ("cover_switch_step", C.c_int32), ("non_cover_slot", C.c_int32), ("ctx_non_cover_dev", C.c_void_p),
        ("sde_noise_dev", C.c_void_p), ("cond_slots_host", C.POINTER(C.c_int32)), ("non_cover_slots_host", C.POINTER(C.c_int32)),
        ("sde_next_from_sched", C.c_int32),
    ]


class CondConfigC(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("text_hidden_dim", C.c_int32), ("timbre_hidden_dim", C.c_int32),
        ("num_lyric_layers", C.c_int32), ("num_timbre_layers", C.c_int32), ("sliding_window", C.c_int32),
        ("sliding_layer_mask", C.c_uint64), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float),
    ]


class DetokConfigC(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32), ("num_heads", C.c_int32), ("num_kv_heads", C.c_int32),
        ("head_dim", C.c_int32), ("num_layers", C.c_int32), ("pool_window_size", C.c_int32), ("out_dim", C.c_int32),
        ("sliding_window", C.c_int32), ("sliding_layer_mask", C.c_uint64), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float),
    ]


class TextEncConfigC(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int32), ("intermediate_size", C.c_int32), ("num_layers", C.c_int32), ("num_heads", C.c_int32),
        ("num_kv_heads", C.c_int32), ("head_dim", C.c_int32), ("vocab_size", C.c_int32), ("rms_norm_eps", C.c_float),
        ("rope_theta", C.c_float),
    ]


class LmConfigC(C.Structure):
    _fields_ = TextEncConfigC._fields_ + [("tie_word_embeddings", C.c_int32), ("max_seqs", C.c_int32), ("max_positions", C.c_int32)]


LM_MAX_SEQS, LM_MAX_POSITIONS, LM_MAX_TOKENS = 16, 16384, 65536   # ACE355_LM_MAX_*
LM_PICK_MAX_V = 1 << 20   # ace355_lm_pick's largest row


class LmPickParamsC(C.Structure):
    _fields_ = [("top_k", C.c_int32), ("top_p", C.c_float), ("temperature", C.c_float), ("reserved", C.c_int32)]


class LmShapeParamsC(C.Structure):
    _fields_ = [("cfg_scale", C.c_float), ("eos_id", C.c_int32), ("eos_mode", C.c_int32), ("has_temperature", C.c_int32),
                ("temperature", C.c_float), ("penalty", C.c_float), ("mask", C.c_void_p), ("seen", C.c_void_p)]


LM_ALLOW_GQA4 = 1   # ACE355_LM_ALLOW_GQA4: ace355_lm_create_ex takes num_heads == 4 * num_kv_heads too
LM_EOS_NONE, LM_EOS_BLOCK, LM_EOS_FORCE = 0, 1, 2   # ace355_lm_shape_params.eos_mode


class VaeConfigC(C.Structure):
    _fields_ = [
        ("decoder_channels", C.c_int32), ("decoder_input_channels", C.c_int32), ("audio_channels", C.c_int32),
        ("num_blocks", C.c_int32), ("channel_multiples", C.c_int32 * MAX_BLOCKS),
        ("upsampling_ratios", C.c_int32 * MAX_BLOCKS),
    ]


class VaeStageInfoC(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("block", C.c_int32), ("unit", C.c_int32), ("channels", C.c_int32), ("flags", C.c_int32),
        ("src", C.c_int32), ("res", C.c_int32), ("dilation", C.c_int32), ("rows", C.c_int64),
    ]


class GemmRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "M", "N", "K", "mode", "fp8", "cu_slots", "aligned", "counters", "fold_producer", "fold_consumer", "hn_q_cols", "hn_qk_cols",
        "vt_offered", "vt_heads", "pf_x", "placement")]


class GemmPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "mode", "mt", "wnw", "ntw", "pers", "ns", "fp8", "grid_x", "grid_y", "threads", "tiles_n", "nwg", "group_m", "xcd_m",
        "ksplit", "kparts", "sk_ord", "krot", "wide_ok", "pf_x", "head_fused", "vt_epilogue", "next_pf_x", "next_pf_xcd_n")] + [
        ("next_pf_chunk16", C.c_uint32), ("next_pf_len16", C.c_uint32)]


GEMM_PLACEMENT_PROCESS = -2   # ACE355_GEMM_PLACEMENT_PROCESS


class AttnRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("N", "Sq", "Skv", "Hq", "Hkv", "window", "cu_slots", "has_kv_len", "mx_out", "reserved")] + [
        ("part_floats", C.c_int64)]


class AttnPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kernel", "nw", "grid_x", "grid_y", "grid_z", "threads", "kv_split", "merge_grid", "mx_out_ok")]


ATTN_KERNELS = ("attn3", "gqa", "rot")   # ACE355_ATTN_KERNEL_*
ATTN_HOOK_PART_FLOATS = 16 << 20         # the split-KV scratch ace355_attention / ace355_attention_masked lend (csrc/api.hip)


class ConvRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "M", "N", "Cin", "taps", "in_snake", "x_view", "res", "fused", "reserved")]


class ConvPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("bn", "tm", "ws", "grid_x", "grid_y", "grid_z", "threads", "ras_tm", "ras_tn", "reserved")]


class VaeStepInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "weight", "block", "unit", "fused", "in_snake", "in_snake_block", "out_snake", "out_snake_block", "src", "dst", "res", "Cin", "N", "taps",
        "dil", "center", "L_in", "M", "out_mode", "n_real", "ncl_m_lo", "ncl_m_hi", "stage", "reserved")] + [(n, C.c_int64) for n in (
        "src_off", "x_batch_stride", "x_shift", "x_valid", "res_batch_stride", "y_batch_stride", "y_shift", "y_valid", "ncl_ld", "ncl_off")] + [
        ("stage_info", VaeStageInfoC), ("plan", ConvPlanInfoC)]


class VaePlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("items_per_window", "core_frames", "overlap_frames", "n_steps", "n_stages", "reserved")] + [
        (n, C.c_int64) for n in ("window_len", "out_len", "slot_elems", "activation_bytes")]


# ACE355_VAE_W_* / ACE355_VAE_SNAKE_* / ACE355_VAE_BUF_* of include/ace355.h, by name
VAE_WEIGHTS = ("conv_in", "convt", "unit_c1", "unit_c2", "down", "out", "head")
VAE_SNAKES = (None, "unit_s1", "unit_s2", "block", "final")
VAE_BUFS = {-1: None, 0: "slot0", 1: "slot1", 2: "slot2", 3: "in", 4: "out"}

# ACE355_VAE_STAGE_* / ACE355_VAE_FLAG_* of include/ace355.h
VAE_STAGE_INPUT, VAE_STAGE_CONV_IN, VAE_STAGE_CONVT, VAE_STAGE_UNIT, VAE_STAGE_UNIT_K7, VAE_STAGE_UNIT_K1, VAE_STAGE_DOWN, VAE_STAGE_HEAD = range(8)
VAE_FLAG_IN_SNAKE, VAE_FLAG_OUT_SNAKE, VAE_FLAG_FUSED, VAE_FLAG_F32_NCL = 1, 2, 4, 8


class DitPassRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("N", "T", "temb_rows")] + [(n, C.c_int32 * MAX_SEQS) for n in ("seq_slot", "seq_L", "seq_broadcast")] + [
        (n, C.c_int32) for n in ("precision", "mx_min_rows", "mx_copies", "nf_on", "nf_emb_on", "nf_rows", "dup_half", "dedup_on", "prefetch",
                                 "cu_slots", "graph_mode", "zr_M", "map_last")] + [("map_heads", C.c_int32 * 64)] + [
        (n, C.c_int32) for n in ("qkv_vt_epilogue", "qkv_vt_epilogue_half", "self_mx_out_ok", "cross_mx_out_ok")] + [
        ("nf_cap_M", C.c_int64), ("tap_mask", C.c_uint64)]


class DitStepInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "layer", "src", "dst", "M", "seqs", "proj", "path", "N", "K", "lda", "ldw", "ldc", "mode", "rows_per_seq", "bias", "gate", "cvec",
        "cvec_row0", "hn", "hn_q_cols", "hn_qk_cols", "vt_offered", "nf_split", "nf_gA", "nf_gB", "nf_sqA", "nf_sqB", "nc_rowsq", "nc_bias", "a_wrap",
        "a_zero_idx", "mxo", "next_proj", "next_layer", "next_M", "next_N", "next_K", "next_mode", "gs", "Sq", "Skv", "window", "mx_out", "Lpad",
        "n_heads", "pair0", "reserved")] + [("count", C.c_int64), ("flops", C.c_double)]


class DitPassInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("S", "M", "Sp", "Nc", "Mc", "n_sc", "L", "Lpad", "fold", "emb", "dedup0", "zero_rows", "n_steps",
                                         "gemm_launches")] + [("vt_elems", C.c_int64), ("gemm_flops", C.c_double), ("attn_flops", C.c_double)]


# ACE355_DIT_STEP_* / _PROJ_* / _PATH_* / _BUF_* of include/ace355.h, by name
DIT_STEPS = ("mod_gs", "zero_rowsq", "norm_gs", "norm_gs_mx", "norm_w", "norm_w_mx", "gemm", "transpose_v", "attn_self", "attn_cross", "xattn_probs",
             "tap", "norm_out")
DIT_PROJS = ("patchify", "qkv", "o", "cross_q", "cross_o", "gate_up", "down", "out")
DIT_PATHS = ("bf16", "mx_quant", "mx")
DIT_BUFS = {-1: None, 0: "xin", 1: "h", 2: "xn", 3: "qkv", 4: "ao", 5: "act", 6: "aq", 7: "xq", 8: "vt", 9: "vpad", 10: "slot_kv", 11: "tap", 12: "maps"}


class EncoderPassRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("hidden_size", "intermediate_size", "num_heads", "num_kv_heads", "num_layers", "sliding_window", "causal",
                                         "N", "S", "has_kv_len", "has_cache", "pos0", "max_pos", "max_seqs", "has_first", "reserved")] + [
        ("sliding_layer_mask", C.c_uint64)]


class EncoderStepInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "kind", "layer", "src", "dst", "M", "N", "K", "norm", "proj", "lda", "ldw", "ldc", "mode", "rows_per_seq", "hn_q_cols", "hn_qk_cols",
        "rope_row0", "sk_cnt", "seqs", "Sq", "Skv", "Hq", "Hkv", "ld", "k_col0", "v_col0", "o_ld", "Sp", "window", "kv_len", "first", "pos0", "len",
        "chunk", "splits", "reserved")] + [("flops", C.c_double)]


# ACE355_ENC_STEP_* / _PROJ_* / _BUF_* of include/ace355.h, by name
ENC_STEPS = ("rmsnorm", "gemm", "kv_store", "causal_attn", "decode_attn", "transpose_v", "vmean", "attn")
ENC_PROJS = ("qkv", "o", "gate_up", "down")
ENC_NORMS = ("input", "post_attention", "final")
ENC_BUFS = {-1: None, 0: "h", 1: "xn", 2: "qkv", 3: "ao", 4: "act", 5: "vt", 6: "vmean", 7: "cache", 8: "out"}
# the fields of a step that each kind's launcher takes.  (The two causal launchers also take the step's Hq, 2 or 4 x Hkv; it is the
# request's num_heads and is left out here so that the recorded plan tables keep their hashes.)
ENC_STEP_FIELDS = {
    "rmsnorm": ("M", "N", "norm", "rows_per_seq"),
    "gemm": ("M", "N", "K", "proj", "lda", "ldw", "ldc", "mode", "rows_per_seq", "hn_q_cols", "hn_qk_cols", "rope_row0", "sk_cnt", "flops"),
    "kv_store": ("seqs", "Sq", "Hkv", "ld", "k_col0", "v_col0", "pos0"),
    "causal_attn": ("seqs", "Sq", "Hkv", "ld", "k_col0", "v_col0", "o_ld", "first"),
    "decode_attn": ("seqs", "Hkv", "ld", "len", "chunk", "splits", "first"),
    "transpose_v": ("seqs", "Sq", "Hkv", "ld", "v_col0", "Sp"),
    "vmean": ("seqs", "Sq", "Hkv", "ld", "v_col0"),
    "attn": ("seqs", "Sq", "Skv", "Hq", "Hkv", "ld", "k_col0", "Sp", "window", "kv_len"),
}


class EncoderPassInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("M", "Sp", "QKV", "rope_rows", "n_steps")] + [("calls", C.c_int32 * len(ENC_STEPS)), ("reserved", C.c_int32),
                                                                                        ("gemm_flops", C.c_double)]


class LoraTermC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("A_dev", C.c_void_p), ("B_dev", C.c_void_p), ("rank", C.c_int32), ("scale", C.c_float)]


class KronTermC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("w1_dev", C.c_void_p), ("w1a_dev", C.c_void_p), ("w1b_dev", C.c_void_p),
                ("w2_dev", C.c_void_p), ("w2a_dev", C.c_void_p), ("w2b_dev", C.c_void_p),
                ("out_l", C.c_int32), ("out_k", C.c_int32), ("in_m", C.c_int32), ("in_n", C.c_int32), ("r1", C.c_int32), ("r2", C.c_int32),
                ("scale", C.c_float)]


class DoraTermC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("g_dev", C.c_void_p), ("per_input", C.c_int32), ("eps", C.c_float), ("multiplier", C.c_float)]


ADAPTER_CLASSES = ("lora", "kron", "dora_lora", "dora_kron")                    # ACE355_ADAPTER_CLASS_*
ADAPTER_KERNELS = ("lora_merge", "kron_factors", "kron_merge", "dora_factors")  # ACE355_ADAPTER_KERNEL_*
ADAPTER_SECTIONS = ("lora_targets", "lora_terms", "kron_targets", "kron_terms", "kron_factors", "dora_lora_targets", "dora_lora_rows",
                    "dora_kron_targets", "dora_kron_rows")


class AdapterTargetInfoC(C.Structure):
    _fields_ = [("name", C.c_char_p)] + [(n, C.c_int32) for n in (
        "cls", "row", "rows", "cols", "tile0", "tiles_n", "term0", "nterms", "restored")]


class AdapterLaunchInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kernel", "pass", "entries", "grid_x", "grid_y", "lds_bytes")] + [("sections", C.c_int32 * 3)]


class AdapterKronInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("out_l", "out_k", "in_m", "in_n", "wide", "w1_f32", "w2_f32")] + [
        ("scale", C.c_float), ("w1_offset", C.c_int64), ("w2_offset", C.c_int64)]


class AdapterFactorInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("rows", "cols", "rank", "tile0", "tiles_n", "reserved")] + [("offset", C.c_int64)]


class AdapterDoraInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("cls", "per_input", "n", "ntiles")] + [
        ("eps", C.c_float), ("multiplier", C.c_float), ("part_offset", C.c_int64), ("f_offset", C.c_int64)]


class AdapterPlanRowsC(C.Structure):
    _fields_ = [("targets", C.POINTER(AdapterTargetInfoC)), ("cap_targets", C.c_int32),
                ("launches", C.POINTER(AdapterLaunchInfoC)), ("cap_launches", C.c_int32),
                ("kron", C.POINTER(AdapterKronInfoC)), ("cap_kron", C.c_int32),
                ("factors", C.POINTER(AdapterFactorInfoC)), ("cap_factors", C.c_int32),
                ("dora", C.POINTER(AdapterDoraInfoC)), ("cap_dora", C.c_int32)]


class AdapterPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_targets", "n_merged", "n_launches", "n_lora_terms", "n_kron_terms", "n_factors", "n_dora",
                                         "stale_kv", "stale_o", "reserved")] + [
        ("table_bytes", C.c_int64), ("kscratch_floats", C.c_int64), ("dscratch_bytes", C.c_int64),
        ("section_at", C.c_int64 * len(ADAPTER_SECTIONS)), ("section_bytes", C.c_int64 * len(ADAPTER_SECTIONS))]


PCM_FORMATS = ("u8", "s16", "s24", "s32", "f32")   # ACE355_PCM_*
PCM_BYTES = (1, 2, 3, 4, 4)
AUDIO_IN_MAX_DENSE_TAPS = 1 << 22   # csrc/audio_in_plan.h: the largest dense tap table n x (2 width + o) the input stage takes


class AudioInRequestC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("format", "channels", "o", "n", "K", "width")] + [("frames", C.c_int64)]


class AudioInPlanInfoC(C.Structure):
    _fields_ = [("out_frames", C.c_int64), ("grid", C.c_int64)] + [(n, C.c_int32) for n in (
        "tile", "threads", "span", "table_in_lds", "lds_bytes", "passthrough")]


FLAC_STATUS = ("ok", "header mismatch", "reserved code", "ran past its byte range", "sample count", "CRC-16 mismatch")   # ACE355_FLAC_*


class FlacStreamInfoC(C.Structure):
    _fields_ = [("total_samples", C.c_int64), ("first_frame", C.c_int64)] + [(n, C.c_int32) for n in (
        "channels", "bits_per_sample", "sample_rate", "min_block", "max_block", "variable_blocks")]


class FlacInPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("entropy_grid", "restore_grid", "finish_grid", "desc_at", "frame_at", "scratch_bytes", "out_bytes")] + [
        (n, C.c_int32) for n in ("launches", "entropy_threads", "entropy_lanes", "restore_threads", "restore_lanes", "finish_threads",
                                 "finish_tiles", "status_threads", "out_format", "reserved")]


class FlacOutPlanInfoC(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("blocks", "units", "frame_grid", "offsets_grid", "gather_grid", "item_stride", "sizes_at", "offsets_at",
                                         "scratch_bytes", "out_bytes", "records_bytes")] + [
        (n, C.c_int32) for n in ("launches", "frame_threads", "offsets_threads", "gather_threads", "frame_lds_bytes", "offsets_lds_bytes",
                                 "slot_stride", "reserved")]


SAVE_FLAC_GPU, SAVE_FLAC_NO_MD5 = 1, 2   # ACE355_SAVE_*


# name -> (restype, argtypes); every symbol include/ace355.h declares
SIGNATURES = {
    "ace355_last_error": (C.c_char_p, []),
    "ace355_version": (C.c_int, []),
    "ace355_dit_create": (C.c_int, [C.POINTER(DitConfigC), C.POINTER(C.c_void_p)]),
    "ace355_dit_destroy": (None, [C.c_void_p]),
    "ace355_dit_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_dit_finalize": (C.c_int, [C.c_void_p]),
    "ace355_dit_set_condition": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ace355_dit_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                     C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_dit_cross_attention_maps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                                  C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p,
                                                  C.c_void_p]),
    "ace355_dit_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(SampleParamsC),
                                    C.c_void_p, C.POINTER(C.c_float), C.c_void_p]),
    "ace355_dit_set_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "ace355_dit_set_adapters": (C.c_int, [C.c_void_p, C.POINTER(LoraTermC), C.c_int, C.c_void_p]),
    "ace355_dit_set_adapters_mixed": (C.c_int, [C.c_void_p, C.POINTER(LoraTermC), C.c_int, C.POINTER(KronTermC), C.c_int, C.c_void_p]),
    "ace355_dit_set_adapters_dora": (C.c_int, [C.c_void_p, C.POINTER(LoraTermC), C.c_int, C.POINTER(KronTermC), C.c_int,
                                               C.POINTER(DoraTermC), C.c_int, C.c_void_p]),
    "ace355_dit_read_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ace355_dit_set_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_set_graph": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_set_norm_fold": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_box_probe_mfma": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "ace355_gemm_set_k_rotation": (C.c_int, [C.c_int]),
    "ace355_gemm_plan": (C.c_int, [C.POINTER(GemmRequestC), C.POINTER(GemmPlanInfoC)]),
    "ace355_attn_plan": (C.c_int, [C.POINTER(AttnRequestC), C.POINTER(AttnPlanInfoC)]),
    "ace355_conv_plan": (C.c_int, [C.POINTER(ConvRequestC), C.POINTER(ConvPlanInfoC)]),
    "ace355_vae_plan": (C.c_int, [C.POINTER(VaeConfigC), C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.POINTER(VaeStepInfoC), C.c_int,
                                  C.POINTER(C.c_int32), C.POINTER(VaePlanInfoC)]),
    "ace355_dit_pass_plan": (C.c_int, [C.POINTER(DitConfigC), C.POINTER(DitPassRequestC), C.POINTER(DitStepInfoC), C.c_int, C.POINTER(C.c_int32),
                                       C.POINTER(DitPassInfoC)]),
    "ace355_adapter_plan": (C.c_int, [C.POINTER(DitConfigC), C.POINTER(LoraTermC), C.c_int, C.POINTER(KronTermC), C.c_int,
                                      C.POINTER(DoraTermC), C.c_int, C.POINTER(C.c_char_p), C.c_int, C.POINTER(AdapterPlanRowsC),
                                      C.POINTER(AdapterPlanInfoC)]),
    "ace355_dit_set_dual": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_dual_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ace355_dit_set_dedup": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_dedup_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "ace355_dit_graph_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "ace355_dit_poll_errors": (C.c_int, [C.c_void_p, C.c_void_p]),
    "ace355_dit_trim_slots": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_set_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_dit_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ace355_vae_create": (C.c_int, [C.POINTER(VaeConfigC), C.POINTER(C.c_void_p)]),
    "ace355_vae_destroy": (None, [C.c_void_p]),
    "ace355_vae_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_vae_finalize": (C.c_int, [C.c_void_p]),
    "ace355_vae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_vae_hop": (C.c_int, [C.c_void_p]),
    "ace355_vae_set_decode_budget": (C.c_int, [C.c_void_p, C.c_int64, C.c_int]),
    "ace355_vae_decode_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int64)]),
    "ace355_vae_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "ace355_vae_latent_frames": (C.c_int, [C.c_void_p, C.c_int64]),
    "ace355_vae_set_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_vae_get_profile": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "ace355_vae_num_stages": (C.c_int, [C.c_void_p, C.c_int]),
    "ace355_vae_get_stage": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.POINTER(VaeStageInfoC)]),
    "ace355_vae_set_tap": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    "ace355_cond_create": (C.c_int, [C.POINTER(CondConfigC), C.POINTER(C.c_void_p)]),
    "ace355_cond_destroy": (None, [C.c_void_p]),
    "ace355_cond_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_cond_finalize": (C.c_int, [C.c_void_p]),
    "ace355_cond_out_len": (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int]),
    "ace355_cond_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p, C.POINTER(C.c_int32), C.c_int,
                                     C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int32),
                                     C.c_void_p]),
    "ace355_tok_create": (C.c_int, [C.POINTER(DetokConfigC), C.POINTER(C.c_void_p)]),
    "ace355_tok_destroy": (None, [C.c_void_p]),
    "ace355_tok_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_tok_finalize": (C.c_int, [C.c_void_p]),
    "ace355_tok_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_detok_create": (C.c_int, [C.POINTER(DetokConfigC), C.POINTER(C.c_void_p)]),
    "ace355_detok_destroy": (None, [C.c_void_p]),
    "ace355_detok_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_detok_finalize": (C.c_int, [C.c_void_p]),
    "ace355_detok_run": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_textenc_create": (C.c_int, [C.POINTER(TextEncConfigC), C.POINTER(C.c_void_p)]),
    "ace355_textenc_destroy": (None, [C.c_void_p]),
    "ace355_textenc_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_textenc_finalize": (C.c_int, [C.c_void_p]),
    "ace355_textenc_encode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_textenc_embed": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int64, C.c_void_p, C.c_void_p]),
    "ace355_lm_create": (C.c_int, [C.POINTER(LmConfigC), C.POINTER(C.c_void_p)]),
    "ace355_lm_create_ex": (C.c_int, [C.POINTER(LmConfigC), C.c_uint32, C.POINTER(C.c_void_p)]),
    "ace355_lm_destroy": (None, [C.c_void_p]),
    "ace355_lm_load_tensor": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    "ace355_lm_finalize": (C.c_int, [C.c_void_p]),
    "ace355_lm_prefill": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_lm_decode": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "ace355_lm_length": (C.c_int, [C.c_void_p]),
    "ace355_lm_decode_plan": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ace355_lm_score_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ace355_lm_score_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ace355_lm_score_plan": (C.c_int, [C.c_int, C.c_int, C.c_int] + [C.POINTER(C.c_int32)] * 5),
    "ace355_lm_score": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int, C.c_int,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "ace355_encoder_pass_plan": (C.c_int, [C.POINTER(EncoderPassRequestC), C.POINTER(EncoderStepInfoC), C.c_int, C.POINTER(C.c_int32),
                                           C.POINTER(EncoderPassInfoC)]),
    "ace355_lm_pick_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ace355_lm_pick_plan": (C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ace355_lm_pick": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.POINTER(LmPickParamsC), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ace355_lm_shape": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                  C.POINTER(LmShapeParamsC), C.c_void_p]),
    "ace355_lm_shape_as": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                     C.POINTER(LmShapeParamsC), C.c_int, C.c_void_p]),
    "ace355_lm_seen_mark": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_lm_decode_tokens": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_lm_bad_tokens": (C.c_int64, [C.c_void_p]),
    "ace355_lm_fan_out": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "ace355_lm_fan_out_plan": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ace355_peak_normalize": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "ace355_latent_check": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.c_void_p]),
    "ace355_normalize_audio": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "ace355_audio_interleave": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "ace355_flac_bound": (C.c_int64, [C.c_int64, C.c_int]),
    "ace355_flac_encode_pcm16": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "ace355_flac_info": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ace355_flac_decode_pcm16": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int]),
    "ace355_wav_bound": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "ace355_wav_encode": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "ace355_save_audio_batch": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_void_p]),
    "ace355_audio_in_plan": (C.c_int, [C.POINTER(AudioInRequestC), C.POINTER(AudioInPlanInfoC)]),
    "ace355_audio_in_run": (C.c_int, [C.POINTER(AudioInRequestC), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "ace355_flac_index": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(FlacStreamInfoC), C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "ace355_flac_in_plan": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(FlacInPlanInfoC)]),
    "ace355_flac_in_decode": (C.c_int, [C.POINTER(FlacStreamInfoC), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "ace355_flac_out_plan": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.POINTER(FlacOutPlanInfoC)]),
    "ace355_flac_out_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p]),
    "ace355_flac_streaminfo": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "ace355_save_audio_batch_ex": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_uint32,
                                             C.c_void_p]),
    "ace355_gemm_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_gemm_bf16_fused": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ace355_gemm_bf16_residual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "ace355_gemm_bf16_headnorm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_float, C.c_void_p]),
    "ace355_mx_quantize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "ace355_mx_rows_pad": (C.c_int, [C.c_int]),
    "ace355_gemm_mxfp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int, C.c_int, C.c_void_p]),
    "ace355_rmsnorm_mod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ace355_headnorm_rope": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_float, C.c_int, C.c_int,
                                       C.c_float, C.c_void_p]),
    "ace355_attention": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_int, C.c_float, C.c_void_p]),
    "ace355_cross_attention_probs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                               C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_float, C.c_void_p]),
    "ace355_align_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "ace355_align_timestamp_matrix": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int,
                                                C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ace355_align_score_matrix": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ace355_align_dtw": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_size_t, C.c_void_p]),
    "ace355_align_score_metrics": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double,
                                             C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "ace355_align_median": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "ace355_attention_masked": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_int, C.c_float, C.POINTER(C.c_int32), C.c_void_p]),
    "ace355_linear_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "ace355_apg_euler_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                        C.c_int, C.c_void_p]),
    "ace355_conv1d_nlc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
}


def lib() -> C.CDLL:
    """Load csrc/libace355.so (once).  Raises RuntimeError if it has not been built."""
    global _LIB
    if _LIB is None:
        # torch bundles its own libamdhip64.so.7; device pointers and streams are shared with torch, so both must
        # run on ONE HIP runtime instance: load torch's first (same SONAME -> our NEEDED entry resolves to it).
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"ace355 native library not found at {LIB_PATH}. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). There is no CPU fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the header and the library drift apart
            fn.restype = res
            fn.argtypes = args
        _LIB = handle
    return _LIB


def last_error() -> str:
    msg = lib().ace355_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc: int, what: str = "") -> None:
    if rc != OK:
        raise RuntimeError(f"ace355 native call failed ({what}, code {rc}): {last_error()}")


def gemm_set_k_rotation(mode: int) -> int:
    """`ace355_gemm_set_k_rotation` (include/ace355.h): 0 off, 1 launches with N <= 2048 (default), 2 every one-round launch; returns the
    previous mode.  Process-wide."""
    return int(lib().ace355_gemm_set_k_rotation(int(mode)))


def gemm_plan(M: int, N: int, K: int, mode: int, **fields) -> dict:
    """`ace355_gemm_plan` (include/ace355.h): the launch the GEMM entry points would make for a request, as a dict of the plan's fields.
    Fields not given are 0, except aligned operands and this process's placement state."""
    rq = GemmRequestC(M=M, N=N, K=K, mode=mode, aligned=1, placement=GEMM_PLACEMENT_PROCESS)
    for k, v in fields.items():
        assert hasattr(rq, k), k
        setattr(rq, k, int(v))
    out = GemmPlanInfoC()
    check(lib().ace355_gemm_plan(C.byref(rq), C.byref(out)), "gemm_plan")
    return {n: int(getattr(out, n)) for n, _t in GemmPlanInfoC._fields_}


def attn_plan(N: int, Sq: int, Skv: int, Hq: int, Hkv: int, window: int = -1, **fields) -> dict:
    """`ace355_attn_plan` (include/ace355.h): the launch the attention launcher would make for a request, as a dict of the plan's fields
    with `kernel` as its name in ATTN_KERNELS.  Fields not given are 0: no scratch, no mask, the whole chip."""
    rq = AttnRequestC(N=N, Sq=Sq, Skv=Skv, Hq=Hq, Hkv=Hkv, window=window)
    for k, v in fields.items():
        assert hasattr(rq, k), k
        setattr(rq, k, int(v))
    out = AttnPlanInfoC()
    check(lib().ace355_attn_plan(C.byref(rq), C.byref(out)), "attn_plan")
    return {**{n: int(getattr(out, n)) for n, _t in AttnPlanInfoC._fields_}, "kernel": ATTN_KERNELS[out.kernel]}


def lm_decode_plan(length: int) -> dict:
    """`ace355_lm_decode_plan` (include/ace355.h): how the LM's decode attention cuts a cache of ``length`` keys - keys per workgroup
    (``chunk``) and chunks per sequence (``splits``).  A function of the length alone; no GPU, no handle."""
    chunk, splits = C.c_int32(), C.c_int32()
    check(lib().ace355_lm_decode_plan(int(length), C.byref(chunk), C.byref(splits)), "lm_decode_plan")
    return {"chunk": chunk.value, "splits": splits.value}


def lm_fan_out_plan(src, n_old: int) -> list:
    """`ace355_lm_fan_out_plan` (include/ace355.h): the launches of ``ace355_lm_fan_out`` for ``src`` on a handle that holds ``n_old``
    sequences, as a list of waves, each a list of ``(dst, src)`` copies in ascending ``dst``.  No wave reads a sequence that the same or
    an earlier wave writes; a sequence that stays (``src[n] == n``) is in no wave.  A refusal raises.  No GPU, no handle."""
    src = [int(v) for v in src]
    n = len(src)
    arr, waves, n_waves = (C.c_int32 * max(n, 1))(*src), (C.c_int32 * max(n, 1))(), C.c_int32()
    check(lib().ace355_lm_fan_out_plan(arr, n, int(n_old), waves, C.byref(n_waves)), "lm_fan_out_plan")
    return [[(d, src[d]) for d in range(n) if waves[d] == w] for w in range(n_waves.value)]


def encoder_pass_plan(hidden_size: int, intermediate_size: int, num_heads: int, num_kv_heads: int, num_layers: int, N: int, S: int, **fields) -> dict:
    """`ace355_encoder_pass_plan` (include/ace355.h): the launcher calls of one pass of the encoder stack over ``N`` sequences of ``S`` rows,
    in launch order, as the cond / detok / tok / textenc / lm handles would make them.  ``fields``: the other ace355_encoder_pass_request
    fields (causal, sliding_window, sliding_layer_mask, has_kv_len, has_cache with pos0 / max_pos / max_seqs / has_first); left out, they are
    0: a bidirectional stack without windows, key counts or cache.  A refusal raises with the stack's or the launcher's text.  Steps: kinds,
    projections, norms and buffers by name, each with the fields its launcher takes; ``calls``: launcher calls per kind."""
    rq = EncoderPassRequestC(hidden_size=hidden_size, intermediate_size=intermediate_size, num_heads=num_heads, num_kv_heads=num_kv_heads,
                             num_layers=num_layers, N=N, S=S)
    for k, v in fields.items():
        assert hasattr(rq, k), k
        setattr(rq, k, int(v))
    n, info = C.c_int32(), EncoderPassInfoC()
    check(lib().ace355_encoder_pass_plan(C.byref(rq), None, 0, C.byref(n), C.byref(info)), "encoder_pass_plan")
    steps = (EncoderStepInfoC * n.value)()
    check(lib().ace355_encoder_pass_plan(C.byref(rq), steps, n.value, C.byref(n), C.byref(info)), "encoder_pass_plan")
    out = {k: getattr(info, k) for k in ("M", "Sp", "QKV", "rope_rows", "n_steps", "gemm_flops")}
    out["calls"] = {ENC_STEPS[i]: int(c) for i, c in enumerate(info.calls)}
    out["steps"] = []
    for st in steps:
        kind = ENC_STEPS[st.kind]
        r = {"kind": kind, "layer": st.layer, "src": ENC_BUFS[st.src], "dst": ENC_BUFS[st.dst], **{k: getattr(st, k) for k in ENC_STEP_FIELDS[kind]}}
        if kind == "gemm":
            r["proj"] = ENC_PROJS[st.proj]
        if kind == "rmsnorm":
            r["norm"] = ENC_NORMS[st.norm]
        out["steps"].append(r)
    return out


def lm_pick_plan(V: int) -> dict:
    """`ace355_lm_pick_plan` (include/ace355.h): how the token selection cuts a row of ``V`` logits - ids per workgroup (``chunk``) and
    chunks per row (``chunks``).  A function of V alone; no GPU."""
    chunk, chunks = C.c_int32(), C.c_int32()
    check(lib().ace355_lm_pick_plan(int(V), C.byref(chunk), C.byref(chunks)), "lm_pick_plan")
    return {"chunk": chunk.value, "chunks": chunks.value}


def lm_score_plan(R: int, V: int, D: int) -> dict:
    """`ace355_lm_score_plan` (include/ace355.h): what the scoring head launches for ``R`` rows against a ``[V, D]`` head - rows per
    workgroup (``tile_rows``), ids per workgroup (``chunk``, a function of V alone), ``chunks`` and the grid.  No GPU."""
    o = [C.c_int32() for _ in range(5)]
    check(lib().ace355_lm_score_plan(int(R), int(V), int(D), *[C.byref(v) for v in o]), "lm_score_plan")
    return dict(zip(("tile_rows", "chunk", "chunks", "grid_x", "grid_y"), (v.value for v in o)))


def lm_score_workspace_bytes(R: int, V: int) -> int:
    """`ace355_lm_score_workspace_bytes`: bytes `ace355_lm_score_rows` needs for ``R`` rows of ``V`` ids (0: outside the limits)."""
    return int(lib().ace355_lm_score_workspace_bytes(int(R), int(V)))


def audio_in_request(format: str, channels: int, frames: int, o: int, n: int, K: int, width: int) -> AudioInRequestC:
    """An ace355_audio_in_request with the format by name (PCM_FORMATS)."""
    if format not in PCM_FORMATS:
        raise ValueError(f"unknown PCM format '{format}'")
    return AudioInRequestC(format=PCM_FORMATS.index(format), channels=int(channels), o=int(o), n=int(n), K=int(K), width=int(width),
                           frames=int(frames))


def audio_in_plan(format: str, channels: int, frames: int, o: int, n: int, K: int, width: int) -> dict:
    """`ace355_audio_in_plan` (include/ace355.h): the launch of the audio input stage for a clip of ``frames`` frames at rate
    ``o / n x 48000`` - output frames, tile, grid, the input span a tile stages, whether the tap table sits in LDS.  A refusal raises with
    the plan's text.  A function of the request alone; no GPU."""
    rq, out = audio_in_request(format, channels, frames, o, n, K, width), AudioInPlanInfoC()
    check(lib().ace355_audio_in_plan(C.byref(rq), C.byref(out)), "audio_in_plan")
    return {k: int(getattr(out, k)) for k, _t in AudioInPlanInfoC._fields_}


def flac_in_plan(frames: int, channels: int, bps: int, max_block: int, total_samples: int) -> dict:
    """`ace355_flac_in_plan` (include/ace355.h): the launches of the GPU FLAC decode for a table of ``frames`` frames - grids, workgroup
    sizes, live lanes per wave, scratch layout and bytes, output format (by name) and bytes.  A refusal raises with the plan's text.  A
    function of its arguments alone; no GPU."""
    out = FlacInPlanInfoC()
    check(lib().ace355_flac_in_plan(int(frames), int(channels), int(bps), int(max_block), int(total_samples), C.byref(out)), "flac_in_plan")
    d = {k: int(getattr(out, k)) for k, _t in FlacInPlanInfoC._fields_ if k != "reserved"}
    d["out_format"] = PCM_FORMATS[d["out_format"]]
    return d


def flac_out_plan(n_items: int, frames: int, channels: int) -> dict:
    """`ace355_flac_out_plan` (include/ace355.h): the launches of the GPU FLAC encode for ``n_items`` items of ``frames`` frames - grids,
    workgroup sizes, LDS bytes, the slot and item strides, scratch layout and bytes, output and record bytes.  A refusal raises with the
    plan's text.  A function of its arguments alone; no GPU."""
    out = FlacOutPlanInfoC()
    check(lib().ace355_flac_out_plan(int(n_items), int(frames), int(channels), C.byref(out)), "flac_out_plan")
    return {k: int(getattr(out, k)) for k, _t in FlacOutPlanInfoC._fields_ if k != "reserved"}


def flac_streaminfo(frames: int, channels: int, sample_rate: int, min_frame: int, max_frame: int, md5: bytes = None) -> bytes:
    """`ace355_flac_streaminfo`: "fLaC" and the STREAMINFO block, 42 bytes; ``md5`` None leaves the 16 MD5 bytes zero."""
    out = (C.c_uint8 * 42)()
    assert md5 is None or len(md5) == 16
    check(lib().ace355_flac_streaminfo(out, int(frames), int(channels), int(sample_rate), int(min_frame), int(max_frame),
                                       C.c_char_p(md5) if md5 is not None else None), "flac_streaminfo")
    return bytes(out)


def conv_plan(B: int, M: int, N: int, Cin: int, taps: int, **bits) -> dict:
    """`ace355_conv_plan` (include/ace355.h): the conv_kernel instantiation and grid a conv launch would get, as a dict of the plan's
    fields.  ``bits``: in_snake, x_view, res, fused (0 when left out)."""
    rq = ConvRequestC(B=B, M=M, N=N, Cin=Cin, taps=taps)
    for k, v in bits.items():
        assert hasattr(rq, k), k
        setattr(rq, k, int(v))
    out = ConvPlanInfoC()
    check(lib().ace355_conv_plan(C.byref(rq), C.byref(out)), "conv_plan")
    return {n: int(getattr(out, n)) for n, _t in ConvPlanInfoC._fields_ if n != "reserved"}


def vae_plan(cfg, encoder: bool, B: int, T: int, budget_bytes: int = 0, overlap_frames: int = 0) -> dict:
    """`ace355_vae_plan` (include/ace355.h): the conv launches of the first window of a decode of (B, T latent frames) / the first group
    of an encode of (B, T samples) on configuration ``cfg`` (a config.VaeConfig), in launch order, with weights, Snakes and buffers by
    name, each step's public stage (or None) and its conv plan; plus the window plan and the buffer size.  No GPU, no handle."""
    ups, cm = list(cfg.upsampling_ratios), list(cfg.channel_multiples)
    c = VaeConfigC(cfg.decoder_channels, cfg.decoder_input_channels, cfg.audio_channels, len(ups), (C.c_int32 * MAX_BLOCKS)(*cm),
                   (C.c_int32 * MAX_BLOCKS)(*ups))
    cap = 2 + 7 * MAX_BLOCKS
    steps, n, info = (VaeStepInfoC * cap)(), C.c_int32(), VaePlanInfoC()
    check(lib().ace355_vae_plan(C.byref(c), 1 if encoder else 0, B, T, budget_bytes, overlap_frames, steps, cap, C.byref(n), C.byref(info)), "vae_plan")
    assert n.value <= cap
    out = {k: int(getattr(info, k)) for k, _t in VaePlanInfoC._fields_ if k != "reserved"}
    out["steps"] = []
    for st in steps[:n.value]:
        r = {k: int(getattr(st, k)) for k, t in VaeStepInfoC._fields_ if t in (C.c_int32, C.c_int64) and k != "reserved"}
        r.update(weight=VAE_WEIGHTS[st.weight], in_snake=VAE_SNAKES[st.in_snake], out_snake=VAE_SNAKES[st.out_snake],
                 src=VAE_BUFS[st.src], dst=VAE_BUFS[st.dst], res=VAE_BUFS[st.res],
                 stage_info={k: int(getattr(st.stage_info, k)) for k, _t in VaeStageInfoC._fields_} if st.stage >= 0 else None,
                 plan={k: int(getattr(st.plan, k)) for k, _t in ConvPlanInfoC._fields_ if k != "reserved"})
        out["steps"].append(r)
    return out


def dit_config_c(cfg) -> DitConfigC:
    """A config.DitConfig as the C struct."""
    return DitConfigC(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.num_key_value_heads,
                      cfg.head_dim, int(cfg.sliding_window or 0), cfg.patch_size, cfg.in_channels, cfg.audio_acoustic_hidden_dim,
                      cfg.rms_norm_eps, cfg.rope_theta, sliding_mask(cfg.layer_types, len(cfg.layer_types)))


def dit_pass_plan(cfg, T: int, seqs, **fields) -> dict:
    """`ace355_dit_pass_plan` (include/ace355.h): the launches of one decoder pass on configuration ``cfg`` (a config.DitConfig) in launch
    order, as the handle would make them.  ``seqs``: per sequence (condition slot, that slot's key count L, set from one row?).  ``fields``:
    further ace355_dit_pass_request fields; left out, they are a fresh bf16 handle's plain forward (temb_rows = N, MXFP8 copies as
    set_precision would make them, dedup and prefetch allowed, no fold, no taps, no maps).  ``map_heads`` is a list per layer.  A refusal
    raises with forward's text.  Steps: kinds, projections, paths and buffers by name; fields a step kind does not use are dropped."""
    seqs = list(seqs)
    rq = DitPassRequestC(N=len(seqs), T=T, temb_rows=len(seqs), mx_min_rows=1536, mx_copies=-1, dedup_on=1, prefetch=1, zr_M=-1, map_last=-1)
    for i, (slot, L, bc) in enumerate(seqs):
        rq.seq_slot[i], rq.seq_L[i], rq.seq_broadcast[i] = int(slot), int(L), int(bc)
    for k, v in fields.items():
        assert hasattr(rq, k), k
        if k == "map_heads":
            for l, n in enumerate(v):
                rq.map_heads[l] = int(n)
        else:
            setattr(rq, k, int(v))
    c = cfg if isinstance(cfg, DitConfigC) else dit_config_c(cfg)
    n, info = C.c_int32(), DitPassInfoC()
    check(lib().ace355_dit_pass_plan(C.byref(c), C.byref(rq), None, 0, C.byref(n), C.byref(info)), "dit_pass_plan")
    steps = (DitStepInfoC * n.value)()
    check(lib().ace355_dit_pass_plan(C.byref(c), C.byref(rq), steps, n.value, C.byref(n), C.byref(info)), "dit_pass_plan")
    out = {k: getattr(info, k) for k, _t in DitPassInfoC._fields_}
    gemm_only = ("proj", "path", "N", "K", "lda", "ldw", "ldc", "mode", "rows_per_seq", "bias", "gate", "cvec", "cvec_row0", "hn", "hn_q_cols",
                 "hn_qk_cols", "vt_offered", "nf_split", "nf_gA", "nf_gB", "nf_sqA", "nf_sqB", "nc_rowsq", "nc_bias", "a_wrap", "a_zero_idx", "mxo",
                 "next_proj", "next_layer", "next_M", "next_N", "next_K", "next_mode")
    attn_only = ("Sq", "Skv", "window", "mx_out", "Lpad", "n_heads", "pair0")
    out["steps"] = []
    for st in steps:
        kind = DIT_STEPS[st.kind]
        r = {k: getattr(st, k) for k, _t in DitStepInfoC._fields_ if k != "reserved"}
        r.update(kind=kind, src=DIT_BUFS[st.src], dst=DIT_BUFS[st.dst])
        if kind == "gemm":
            r.update(proj=DIT_PROJS[st.proj], path=DIT_PATHS[st.path], next_proj=DIT_PROJS[st.next_proj] if st.next_proj >= 0 else None)
        for k in (() if kind == "gemm" else gemm_only) + (() if kind in ("attn_self", "attn_cross", "xattn_probs") else attn_only):
            del r[k]
        out["steps"].append(r)
    return out


def _rows(arr, n):
    out = []
    for i in range(n):
        r = {}
        for f, _t in arr[i]._fields_:
            v = getattr(arr[i], f)
            r[f] = v.decode() if isinstance(v, bytes) else list(v) if hasattr(v, "_length_") else v
        r.pop("reserved", None)
        out.append(r)
    return out


def adapter_plan(cfg: DitConfigC, lora=(), kron=(), dora=(), applied=()) -> dict:
    """`ace355_adapter_plan` (include/ace355.h): what a set_adapters call with these terms comes to on a decoder of configuration ``cfg``
    whose targets ``applied`` hold a merge now - targets, Kronecker term rows, factor jobs, DoRA rows, launches, table sections and
    scratch sizes, as dicts with classes, kernels and sections by name.  ``lora`` / ``kron`` / ``dora`` are tuples of the fields of
    LoraTermC / KronTermC / DoraTermC (names as bytes; device pointers are any numbers, only tested).  No GPU, no handle."""
    la = (LoraTermC * max(len(lora), 1))(*[LoraTermC(*r) for r in lora])
    ka = (KronTermC * max(len(kron), 1))(*[KronTermC(*r) for r in kron])
    da = (DoraTermC * max(len(dora), 1))(*[DoraTermC(*r) for r in dora])
    names = (C.c_char_p * max(len(applied), 1))(*[n.encode() if isinstance(n, str) else n for n in applied])
    nt, nk = len(lora) + len(kron) + len(dora) + len(applied) + 1, len(kron) + 1
    tg, ln, kr, fa, dr = (AdapterTargetInfoC * nt)(), (AdapterLaunchInfoC * 9)(), (AdapterKronInfoC * nk)(), (AdapterFactorInfoC * (2 * nk))(), \
        (AdapterDoraInfoC * (len(dora) + 1))()
    rows = AdapterPlanRowsC(tg, nt, ln, 9, kr, nk, fa, 2 * nk, dr, len(dora) + 1)
    info = AdapterPlanInfoC()
    check(lib().ace355_adapter_plan(C.byref(cfg), la, len(lora), ka, len(kron), da, len(dora), names, len(applied), C.byref(rows),
                                    C.byref(info)), "adapter_plan")
    assert info.n_targets <= nt and info.n_launches <= 9 and info.n_kron_terms <= nk and info.n_factors <= 2 * nk and info.n_dora <= len(dora) + 1
    out = {n: int(getattr(info, n)) for n, _t in AdapterPlanInfoC._fields_[:13] if n != "reserved"}
    out["sections"] = {s: (int(info.section_at[i]), int(info.section_bytes[i])) for i, s in enumerate(ADAPTER_SECTIONS)}
    out["targets"] = [{**r, "cls": ADAPTER_CLASSES[r["cls"]]} for r in _rows(tg, info.n_targets)]
    out["launches"] = [{**r, "kernel": ADAPTER_KERNELS[r["kernel"]], "sections": [ADAPTER_SECTIONS[s] if s >= 0 else None for s in r["sections"]]}
                       for r in _rows(ln, info.n_launches)]
    out["kron"] = _rows(kr, info.n_kron_terms)
    out["factors"] = _rows(fa, info.n_factors)
    out["dora"] = [{**r, "cls": ADAPTER_CLASSES[r["cls"]]} for r in _rows(dr, info.n_dora)]
    return out


def current_stream_ptr() -> int:
    """The caller's current HIP stream as an integer handle (use the caller's stream)."""
    import torch
    return int(torch.cuda.current_stream().cuda_stream)


def ptr(t) -> int:
    """Device/host address of a contiguous torch tensor (0 for None)."""
    if t is None:
        return 0
    assert t.is_contiguous(), "ace355: tensors crossing the C ABI must be contiguous"
    return int(t.data_ptr())


def sliding_mask(layer_types, n: int) -> int:
    """Bit i set when layer i < n is a ``sliding_attention`` layer (the ``sliding_layer_mask`` of the C configs)."""
    return sum(1 << i for i in range(n) if layer_types[i] == "sliding_attention")


def load_state_dict(load_fn, finalize_fn, handle, sd, what: str, device, skip=None) -> None:
    """Feed a state dict to ``<what>_load_tensor`` and seal it with ``<what>_finalize``: fp32 / bf16 as they are, other dtypes as
    fp32, CPU or GPU.  Rotary ``inv_freq`` buffers are skipped, and so is every entry for which ``skip(name, tensor)`` is true."""
    import torch
    with torch.cuda.device(device):
        for name, t in sd.items():
            if "rotary_emb" in name:
                continue
            t = t.detach()
            if skip is not None and skip(name, t):
                continue
            if t.dtype not in (torch.float32, torch.bfloat16):
                t = t.float()
            t = t.contiguous()
            dt = DTYPE_F32 if t.dtype == torch.float32 else DTYPE_BF16
            check(load_fn(handle, name.encode(), ptr(t), dt, t.numel(), 1 if t.is_cuda else 0), f"{what}_load_tensor({name})")
        check(finalize_fn(handle), f"{what}_finalize")


class Owner:
    """Base of the classes that own a native handle: ``_destroy`` names the library's destroy function."""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None):
            import torch
            with torch.cuda.device(self.device):
                getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
