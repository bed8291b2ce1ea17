"""ctypes binding of libmusic2midi_amd.so (the C ABI in include/music2midi_amd.h).

There is NO fallback: if the library is missing or a call fails, this module
raises.  The product never routes through ``oracle/`` or a torch CPU path.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path
from typing import Optional

_LIB_PATH = Path(__file__).resolve().parent / "lib" / "libmusic2midi_amd.so"
_lib: Optional[C.CDLL] = None
_lock = threading.Lock()

PREC_FP32 = 0
PREC_BF16 = 1
PREC_FP8 = 2
KERNEL_DEC_CROSS_ATTN = 0
KERNEL_DEC_SELF_ATTN = 1
KERNEL_DEC_STEP = 2


class NativeError(RuntimeError):
    pass


class FrontendDesc(C.Structure):
    _fields_ = [("n_fft", C.c_int), ("hop_length", C.c_int), ("n_freqs", C.c_int), ("n_mels", C.c_int),
                ("window_host", C.c_void_p), ("fb_host", C.c_void_p)]


class FrontendPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("form", "grid_x", "grid_y", "chunks", "frames_per_chunk", "frames", "n_wpad", "lds_bytes")]


FE_FORMS = ("v2_nj6", "v2_nj8", "v1_taps_lds", "v1_taps_global")   # FrontendPlan.form -> name (M2M_FE_FORM_*)


class AugmentPlan(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("frames", "stretched_frames", "stretched_len", "up", "down", "taps", "cap_frames", "cap_len")]


class AugmentStages(C.Structure):
    _fields_ = [("stft", C.c_void_p), ("stretched_stft", C.c_void_p), ("stretched_wave", C.c_void_p)]


class DatasetClip(C.Structure):
    """m2m_dataset_clip: one clip of m2m_dataset_crop_f32."""
    _fields_ = [("bytes_dev", C.c_void_p), ("h_phase_dev", C.c_void_p), ("n_frames", C.c_int64), ("channels", C.c_int32),
                ("format", C.c_int32), ("up", C.c_int32), ("down", C.c_int32), ("half", C.c_int32), ("reserved", C.c_int32)]


class RenderNote(C.Structure):
    """m2m_render_note: one packed note of m2m_render_notes_f32 (six 32-bit words)."""
    _fields_ = [("on", C.c_int32), ("off", C.c_int32), ("inc", C.c_uint32), ("dec", C.c_uint32), ("table", C.c_int32), ("gain", C.c_float)]


class RenderVoice(C.Structure):
    """m2m_render_voice: the device tables and integer constants of a render.Voice."""
    _fields_ = [("wave_dev", C.c_void_p), ("decay_dev", C.c_void_p), ("table_size", C.c_int32), ("n_tables", C.c_int32),
                ("decay_steps", C.c_int32), ("attack", C.c_int32), ("release", C.c_int32), ("reserved", C.c_int32)]


class AlignProblem(C.Structure):
    """m2m_align_problem: one DTW problem of m2m_align_dtw (six 32-bit words)."""
    _fields_ = [(n, C.c_int32) for n in ("a_offset", "n", "b_offset", "m", "shift", "path_offset")]


class BeatClip(C.Structure):
    """m2m_beat_clip: one clip of m2m_beat_track (four 32-bit words)."""
    _fields_ = [(n, C.c_int32) for n in ("env_offset", "frames", "period", "beat_offset")]


class T5GeometryC(C.Structure):
    _fields_ = [(n, C.c_int) for n in
                ("d_model", "d_ff", "num_layers", "num_decoder_layers", "num_heads", "d_kv", "vocab_size",
                 "num_buckets", "max_distance", "pad_token_id", "eos_token_id", "decoder_start_token_id")] + \
               [("layer_norm_eps", C.c_float)]


class EncLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("ln0", "q", "k", "v", "o", "ln1", "wi0", "wi1", "wo")]


class DecLayerWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("ln0", "q", "k", "v", "o", "ln1", "cq", "ck", "cv", "co", "ln2", "wi0", "wi1", "wo")]


class T5Weights(C.Structure):
    _fields_ = [("shared", C.c_void_p), ("lm_head", C.c_void_p), ("enc_rel_bias", C.c_void_p),
                ("dec_rel_bias", C.c_void_p), ("enc_final_ln", C.c_void_p), ("dec_final_ln", C.c_void_p),
                ("enc", C.POINTER(EncLayerWeights)), ("dec", C.POINTER(DecLayerWeights))]


class SampleParams(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("seed", C.c_uint64)]


class ProcessParams(C.Structure):
    _fields_ = [("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int), ("min_length", C.c_int),
                ("min_new_tokens", C.c_int), ("forced_bos_token_id", C.c_int), ("forced_eos_token_id", C.c_int),
                ("suppress_tokens", C.POINTER(C.c_int32)), ("n_suppress_tokens", C.c_int),
                ("begin_suppress_tokens", C.POINTER(C.c_int32)), ("n_begin_suppress_tokens", C.c_int),
                ("bad_words_ids", C.POINTER(C.c_int32)), ("bad_words_lengths", C.POINTER(C.c_int32)), ("n_bad_words", C.c_int)]


class GrammarParams(C.Structure):
    _fields_ = [("pitch_offset", C.c_int), ("n_pitch", C.c_int), ("n_time", C.c_int)]


class BeamParams(C.Structure):
    _fields_ = [("num_beams", C.c_int), ("length_penalty", C.c_float), ("early_stopping", C.c_int),
                ("num_return_sequences", C.c_int)]


class TensorInfo(C.Structure):
    _fields_ = [("name", C.c_char * 160), ("offset", C.c_int64), ("rows", C.c_int), ("cols", C.c_int)]


# name -> (restype, argtypes); every symbol include/music2midi_amd.h declares.
_SIGNATURES = {
    "m2m_abi_version": (C.c_int, []),
    "m2m_last_error": (C.c_char_p, []),
    "m2m_device_count": (C.c_int, []),
    "m2m_frontend_create": (C.c_int, [C.POINTER(FrontendDesc), C.POINTER(C.c_void_p)]),
    "m2m_frontend_destroy": (None, [C.c_void_p]),
    "m2m_frontend_num_frames": (C.c_int, [C.c_void_p, C.c_int]),
    "m2m_frontend_fb_nnz": (C.c_int, [C.c_void_p]),
    "m2m_logmel_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                 C.c_void_p]),
    "m2m_frontend_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(FrontendPlan)]),
    "m2m_cond_rows_f32": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "m2m_augment_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "m2m_augment_destroy": (None, [C.c_void_p]),
    "m2m_augment_plan": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(AugmentPlan)]),
    "m2m_augment_filter": (C.c_int, [C.c_int, C.c_void_p, C.c_int]),
    "m2m_augment_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "m2m_pitch_shift_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(AugmentStages), C.c_void_p]),
    "m2m_score_frame_count": (C.c_int64, [C.c_double]),
    "m2m_score_detokenize": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "m2m_score_detokenize_scored": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                              C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_score_chroma_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_score_note_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "m2m_score_note_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "m2m_score_frame_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_score_error_notes_capacity": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "m2m_score_error_notes_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "m2m_score_error_notes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_consensus_workspace_bytes": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "m2m_consensus_pairwise_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double,
                                                C.c_double, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_consensus_select": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_ingest_resampled_length": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "m2m_ingest_phase_taps": (C.c_int, [C.c_int, C.c_int]),
    "m2m_ingest_pcm": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_ingest_resample_f32": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                          C.c_void_p]),
    "m2m_dataset_crop_window": (C.c_int, [C.c_int, C.c_int]),
    "m2m_dataset_crop_f32": (C.c_int, [C.POINTER(DatasetClip), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "m2m_render_tile": (C.c_int, []),
    "m2m_render_notes_f32": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(RenderVoice), C.c_void_p, C.c_int64,
                                       C.c_int64, C.c_int, C.c_void_p]),
    "m2m_align_features": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_align_coarse": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p]),
    "m2m_align_dtw_strip": (C.c_int, []),
    "m2m_align_dtw_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_void_p, C.c_int]),
    "m2m_align_dtw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "m2m_beat_envelope": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "m2m_beat_track_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int]),
    "m2m_beat_track": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "m2m_tokenize_quantize": (C.c_int, [C.c_double, C.c_double, C.c_int]),
    "m2m_tokenize_row_bound": (C.c_int64, [C.c_int, C.c_int]),
    "m2m_tokenize_notes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.c_double, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "m2m_model_create": (C.c_int, [C.POINTER(T5GeometryC), C.POINTER(T5Weights), C.c_int, C.c_void_p,
                                   C.POINTER(C.c_void_p)]),
    "m2m_model_destroy": (None, [C.c_void_p]),
    "m2m_model_precision": (C.c_int, [C.c_void_p]),
    "m2m_model_param_bytes": (C.c_int64, [C.c_void_p]),
    "m2m_model_checksum": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]),
    "m2m_rel_bucket": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "m2m_session_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "m2m_session_create": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                     C.POINTER(C.c_void_p)]),
    "m2m_session_destroy": (None, [C.c_void_p]),
    "m2m_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_generate_greedy": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "m2m_generate_sample": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(SampleParams), C.c_void_p, C.POINTER(C.c_int),
                                      C.c_void_p]),
    "m2m_generate_processed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ProcessParams), C.POINTER(SampleParams), C.c_void_p,
                                         C.POINTER(C.c_int), C.c_void_p]),
    "m2m_generate_scored": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ProcessParams), C.POINTER(SampleParams), C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "m2m_generate_grammar": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(GrammarParams), C.POINTER(ProcessParams), C.POINTER(SampleParams),
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "m2m_generate_beam": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BeamParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_int),
                                    C.c_void_p]),
    "m2m_generate_beam_processed": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(BeamParams), C.POINTER(GrammarParams),
                                              C.POINTER(ProcessParams), C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p]),
    "m2m_session_repack_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "m2m_decode_forced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_trainer_create": (C.c_int, [C.POINTER(T5GeometryC), C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int,
                                     C.POINTER(C.c_void_p)]),
    "m2m_trainer_destroy": (None, [C.c_void_p]),
    "m2m_trainer_num_params": (C.c_int64, [C.c_void_p]),
    "m2m_trainer_num_tensors": (C.c_int, [C.c_void_p]),
    "m2m_trainer_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(TensorInfo)]),
    "m2m_trainer_workspace_bytes": (C.c_int64, [C.c_void_p]),
    "m2m_train_forward_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                             C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_train_forward_backward_acc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                 C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p]),
    "m2m_trainer_set_dropout": (C.c_int, [C.c_void_p, C.c_float, C.c_uint64]),
    "m2m_trainer_set_sync_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "m2m_trainer_early_grad_ranges": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "m2m_trainer_graph_nodes": (C.c_int, [C.c_void_p]),
    "m2m_adafactor_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_adafactor_get_step": (C.c_int, [C.c_void_p]),
    "m2m_adafactor_state_floats": (C.c_int64, [C.c_void_p]),
    "m2m_adafactor_state_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_adafactor_state_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "m2m_trainer_set_grad_clip": (C.c_int, [C.c_void_p, C.c_int, C.c_float]),
    "m2m_trainer_grad_norm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_mx8_matmul_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_mx8_matmul_bf16a": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "m2m_mx8_quantize_cols": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_mx8_quantize_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_mx8_quantize_weight": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_mx8_step_product": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_float, C.c_uint64, C.c_uint64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "m2m_attn_head_fwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float,
                                         C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_attn_head_bwd_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "m2m_bench_kernel": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float),
                                   C.POINTER(C.c_int64), C.c_void_p]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)


def library_path() -> Path:
    return Path(os.environ.get("M2M_LIBRARY", str(_LIB_PATH)))


def load() -> C.CDLL:
    """Load the shared library once; raise NativeError if it is not there."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = library_path()
        if not path.exists():
            raise NativeError(
                f"{path} not found: the HIP library has not been built. Run "
                "`python -m music2midi_amd.csrc.build` (needs hipcc). There is no CPU fallback.")
        try:
            lib = C.CDLL(str(path))
        except OSError as e:
            raise NativeError(f"cannot load {path}: {e}") from e
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise NativeError(f"{path} does not export {name} (stale build?)") from e
            fn.restype = res
            fn.argtypes = args
        if lib.m2m_abi_version() != 1:
            raise NativeError(f"ABI version mismatch: library {lib.m2m_abi_version()}, binding 1")
        _lib = lib
        return lib


def check(status: int, what: str) -> None:
    if status != 0:
        msg = load().m2m_last_error().decode("utf-8", "replace")
        raise NativeError(f"{what} failed (status {status}): {msg}")


def stream_handle(device=None) -> int:
    """hipStream_t of torch's current stream on `device` as an integer."""
    import torch
    return int(torch.cuda.current_stream(device).cuda_stream)


def require_gpu() -> None:
    import torch
    if not torch.cuda.is_available() or load().m2m_device_count() < 1:
        raise NativeError("no HIP device visible: the Music2MIDI MI355X path has no CPU fallback")
