"""ctypes binding of csrc/libwhispermi.so (include/whisper_mi.h).  Fails loudly when the HIP library is missing:
there is no CPU fallback in this package."""
from __future__ import annotations

import ctypes as C
import os

from .config import WmDims

_HERE = os.path.dirname(os.path.abspath(__file__))
# WM_USE_DEV_LIB=1 (developer tools only) selects the -DWM_DEV build with the A/B switches and debug chains
LIB_PATH = os.path.join(_HERE, "csrc", "libwhispermi_dev.so" if os.environ.get("WM_USE_DEV_LIB") else "libwhispermi.so")
if os.environ.get("WM_USE_DEV_LIB") and os.environ.get("WM_DEV_LIB_PATH"):  # a developer A/B build kept under another name
    LIB_PATH = os.environ["WM_DEV_LIB_PATH"]

# every symbol include/whisper_mi.h declares (tests/test_cabi_symbols.py checks the .so exports all of them)
SYMBOLS = [
    "wm_last_error", "wm_abi_version", "wm_model_load", "wm_model_load_memory", "wm_model_free", "wm_weight_count", "wm_weights_convert_v2", "wm_weights_read", "wm_state_new",
    "wm_state_reset", "wm_state_free", "wm_state_len", "wm_encode", "wm_state_set_encoder_output", "wm_decode_step",
    "wm_transcribe", "wm_transcribe_submit", "wm_transcribe_wait", "wm_transcribe_wait_device", "wm_transcribe_steps", "wm_log_mel", "wm_transcribe_pcm", "wm_op_matmul_nt", "wm_op_ln_matmul_nt", "wm_op_mlp_block", "wm_op_attention", "wm_op_attention_cached", "wm_op_layer_norm", "wm_op_gelu", "wm_op_softmax_rows", "wm_op_conv1d_k3",
    "wm_op_argmax", "wm_op_logits", "wm_op_xattn", "wm_op_dec_linear", "wm_bench_kernel", "wm_bench_bytes", "wm_synth_weights", "wm_synth_mel_host",
    "wm_set_alignment_heads", "wm_transcribe_tt", "wm_transcribe_submit_tt", "wm_transcribe_wait_tt", "wm_transcribe_pcm_tt",
    "wm_alignment_weights", "wm_op_token_times",
    "wm_log_mel_long", "wm_transcribe_long", "wm_transcribe_long_pcm", "wm_long_result_sizes", "wm_long_result_get",
    "wm_long_result_stats", "wm_long_result_free", "wm_op_long_segments",
    "wm_transcribe_rows", "wm_transcribe_submit_rows", "wm_transcribe_long_ex", "wm_transcribe_long_pcm_ex", "wm_op_long_prompt",
    "wm_op_attention_cached_lo", "wm_long_result_prompt_stats",
    "wm_transcribe_lp", "wm_transcribe_submit_lp", "wm_transcribe_wait_lp", "wm_op_logits_lp",
    "wm_transcribe_lp_ns", "wm_transcribe_submit_lp_ns", "wm_transcribe_wait_lp_ns", "wm_op_no_speech",
    "wm_long_result_quality", "wm_long_result_windows", "wm_long_result_skip_stats",
    "wm_detect_language", "wm_transcribe_lang", "wm_transcribe_submit_lang", "wm_transcribe_wait_lang", "wm_op_lang_detect",
    "wm_transcribe_long_lang", "wm_transcribe_long_pcm_lang",
    "wm_score", "wm_score_submit", "wm_score_wait", "wm_score_pcm", "wm_op_score_logits", "wm_score_phases",
    "wm_align", "wm_align_submit", "wm_align_wait", "wm_align_pcm", "wm_align_phases", "wm_op_dec_linear_capmap", "wm_op_token_times_rows",
    "wm_op_align_probs", "wm_op_align_norm",
    "wm_op_attention_batch", "wm_op_layer_norm_t",
    "wm_op_xattn_absorb",
    "wm_op_dec_linear_long",
    "wm_transcribe_long_tt", "wm_transcribe_long_pcm_tt", "wm_long_result_token_times", "wm_op_long_token_times",
    "wm_set_repeat_options", "wm_op_logits_processed", "wm_op_repeat_sets",
    "wm_set_sequence_bias", "wm_op_logits_seq_bias", "wm_op_seq_bias_hits",
    "wm_chunk_table", "wm_transcribe_chunked", "wm_op_chunk_gather", "wm_op_chunk_merge",
    "wm_transcribe_chunked_ts", "wm_op_chunk_segments",
    "wm_op_gemm_nt_epi", "wm_op_gemm_nt_ring",
    "wm_resample_len", "wm_resample_pcm", "wm_op_resample", "wm_op_resample_taps",
    "wm_set_top_k", "wm_transcribe_top_k", "wm_op_logits_topk",
    "wm_set_constraint", "wm_transcribe_constraint_match", "wm_op_constraint_states",
    "wm_op_fe_tables", "wm_op_fe_frames", "wm_op_fe_mel_log", "wm_op_fe_mel_norm", "wm_op_window_gather",
    "wm_score_nbest", "wm_score_nbest_submit", "wm_score_nbest_wait", "wm_score_nbest_pcm",
    "wm_op_attention_cached_map", "wm_op_xattn_map", "wm_op_score_rank",
    "wm_op_ts_states", "wm_op_init_tokens", "wm_op_set_rows_step", "wm_op_set_step", "wm_op_pack_tokens", "wm_op_dec_embed", "wm_op_rows_copy",
    "wm_op_mel_transpose_pad",
]

ABI_VERSION = 5  # include/whisper_mi.h WM_ABI_VERSION: the struct layouts below are this version's
KERNEL_CROSS_ATTN, KERNEL_DECODE_STEP, KERNEL_ENCODER, KERNEL_DECODE_STEP_SHARED = 0, 1, 2, 3


class WmConfig(C.Structure):
    _fields_ = [("dims", WmDims), ("gelu_mode", C.c_int), ("compute_dtype", C.c_int), ("kv_dtype", C.c_int),
                ("max_batch", C.c_int), ("decoder_fp32", C.c_int), ("coalesce", C.c_int)]


class WmDecodeOpts(C.Structure):
    _fields_ = [("prompt", C.POINTER(C.c_int32)), ("n_prompt", C.c_int), ("eot", C.c_int), ("max_loop", C.c_int),
                ("pos_mode", C.c_int), ("ignore_eot", C.c_int),
                ("suppress_tokens", C.POINTER(C.c_int32)), ("n_suppress", C.c_int),
                ("begin_suppress_tokens", C.POINTER(C.c_int32)), ("n_begin_suppress", C.c_int),
                ("timestamp_begin", C.c_int), ("no_timestamps_token", C.c_int), ("max_initial_timestamp_index", C.c_int)]


class WmSegment(C.Structure):
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("start", C.c_double), ("end", C.c_double)]


class WmLongOpts(C.Structure):
    _fields_ = [("condition_on_prev_tokens", C.c_int), ("prev_sot_token", C.c_int), ("prompt_ids", C.POINTER(C.c_int32)),
                ("n_prompt_ids", C.c_int), ("prompt_condition_type", C.c_int),
                ("use_logprob_threshold", C.c_int), ("logprob_threshold", C.c_float),
                ("use_no_speech_threshold", C.c_int), ("no_speech_threshold", C.c_float), ("no_speech_token", C.c_int)]


PROMPT_CONDITION_TYPES = {"first-segment": 0, "all-segments": 1}


def long_opts(prompt_ids=None, condition_on_prev_tokens=False, prompt_condition_type="first-segment", prev_sot_token=50361,
              logprob_threshold=None, no_speech_threshold=None, no_speech_token=None):
    """-> (WmLongOpts, keep-alive array).  prompt_condition_type: a name of PROMPT_CONDITION_TYPES.
    logprob_threshold / no_speech_threshold / no_speech_token: HF generate's thresholds; ValueError for a
    no_speech_threshold without logprob_threshold (HF dereferences it) or without the <|nospeech|> id."""
    import numpy as np
    if no_speech_threshold is not None:
        if logprob_threshold is None:
            raise ValueError("no_speech_threshold needs logprob_threshold")
        if no_speech_token is None:
            raise ValueError("no_speech_threshold needs no_speech_token (the <|nospeech|> id, HF: no_timestamps_token_id - 1)")
    if no_speech_token is not None and int(no_speech_token) < 0:
        raise ValueError("no_speech_token must be a vocabulary id")
    if (prompt_condition_type or "first-segment") not in PROMPT_CONDITION_TYPES:
        raise ValueError(f"prompt_condition_type must be one of {sorted(PROMPT_CONDITION_TYPES)}")
    p = np.ascontiguousarray(np.asarray([] if prompt_ids is None else prompt_ids, np.int32).reshape(-1))
    o = WmLongOpts(int(bool(condition_on_prev_tokens)), int(prev_sot_token), p.ctypes.data_as(C.POINTER(C.c_int32)) if p.size else None,
                   int(p.size), PROMPT_CONDITION_TYPES[prompt_condition_type or "first-segment"],
                   int(logprob_threshold is not None), float(logprob_threshold or 0.0),
                   int(no_speech_threshold is not None), float(no_speech_threshold or 0.0),
                   -1 if no_speech_token is None else int(no_speech_token))
    return o, p


def no_speech_args(no_speech_token, n_init, prompt_lens, vocab):
    """Checks the no-speech probe's arguments on the host (the library refuses the same with WM_E_ARG) -> (token, n_init).
    n_init None: the shared prompt's length (prompt_lens one number); required with per-row prompts (a list of lengths)."""
    shared = isinstance(prompt_lens, int)
    if n_init is None:
        if not shared:
            raise ValueError("n_init is required with per-row prompts (the number of initial ids, <|startoftranscript|> first)")
        n_init = prompt_lens
    token, n_init = int(no_speech_token), int(n_init)
    if token < 0 or token >= vocab:
        raise ValueError(f"no_speech_token {token} is not a vocabulary id")
    shortest = prompt_lens if shared else min(int(v) for v in prompt_lens)
    if n_init < 1 or n_init > shortest:
        raise ValueError(f"n_init {n_init} outside [1, shortest prompt = {shortest}]")
    return token, n_init


LANG_DETECT_MAX = 128  # csrc/wm_kernels.h LANG_DETECT_MAX


def lang_args(lang_ids, vocab):
    """Checks a language list on the host (the library refuses the same with WM_E_ARG) -> contiguous int32 array."""
    import numpy as np
    ids = np.ascontiguousarray(np.asarray(lang_ids, np.int64).reshape(-1))
    if ids.size < 1 or ids.size > LANG_DETECT_MAX:
        raise ValueError(f"the language list needs 1..{LANG_DETECT_MAX} ids, got {ids.size}")
    if ids.min() < 0 or ids.max() >= vocab:
        raise ValueError(f"language ids must be vocabulary ids [0, {vocab})")
    if np.unique(ids).size != ids.size:
        raise ValueError("a language id is listed twice")
    return ids.astype(np.int32)


def score_args(ids, context_len, B, vocab, n_text_ctx, max_batch):
    """Checks a score call's arguments on the host (the library refuses the same with WM_E_ARG) -> (table [B, stride] int32,
    lengths [B], context lengths [B]).  ids: one id list per row (the decoder prompt followed by the hypothesis); context_len: None
    (= 1), one number, or one per row."""
    import numpy as np
    rows = [np.asarray(r, np.int64).reshape(-1) for r in ids]
    if len(rows) != B:
        raise ValueError(f"{len(rows)} id rows for {B} clips")
    if B < 1 or B > max_batch:
        raise ValueError(f"batch {B} outside [1, max_batch = {max_batch}]")
    lens = np.asarray([r.size for r in rows], np.int32)
    if lens.min() < 2 or lens.max() > n_text_ctx:
        raise ValueError(f"every row needs 2..{n_text_ctx} ids")
    ctx = np.full(B, 1, np.int32) if context_len is None else np.broadcast_to(np.asarray(context_len, np.int32), (B,)).copy()
    if (ctx < 1).any() or (ctx > lens - 1).any():
        raise ValueError("context_len must lie in [1, len - 1] for every row")
    tab = np.zeros((B, int(lens.max())), np.int32)
    for b, r in enumerate(rows):
        if r.min() < 0 or r.max() >= vocab:
            raise ValueError(f"row {b} holds an id outside the vocabulary [0, {vocab})")
        tab[b, :r.size] = r
    return tab, lens, ctx


def nbest_args(candidates, context_len, U, vocab, n_text_ctx, max_batch):
    """Checks an n-best score call's arguments on the host (the library refuses the same with WM_E_ARG) -> (table
    [R, stride] int32, lengths [R], context lengths [R], n_cand [U], utt_of [R], row0 [U]).  candidates: per clip a non-empty list of
    id lists (each as a row of score_args); the R = sum n_cand rows are flattened clip by clip in the caller's order.  context_len:
    None (= 1), one number, one per row (flat, [R]), or per clip a list with one entry per candidate."""
    import numpy as np
    try:
        clips = [list(c) for c in candidates]
    except TypeError:
        raise ValueError("candidates: one list of id lists per clip")
    if U < 1 or len(clips) != U:
        raise ValueError(f"{len(clips)} candidate lists for {U} clips (at least one clip)")
    n_cand = np.asarray([len(c) for c in clips], np.int32)
    if n_cand.min() < 1:
        raise ValueError("every clip needs at least one candidate")
    R = int(n_cand.sum())
    if R > max_batch:
        raise ValueError(f"{R} candidates in all exceed max_batch = {max_batch}")
    if context_len is not None and not np.isscalar(context_len):
        cl = list(context_len)
        if len(cl) == U and all(not np.isscalar(c) for c in cl):  # per clip, one entry per candidate
            if any(len(c) != n for c, n in zip(cl, n_cand)):
                raise ValueError("context_len per clip needs one entry per candidate")
            cl = [v for c in cl for v in c]
        if len(cl) != R:
            raise ValueError(f"context_len needs one entry per candidate row ({R}), got {len(cl)}")
        context_len = cl
    tab, lens, ctx = score_args([r for c in clips for r in c], context_len, R, vocab, n_text_ctx, max_batch)
    row0 = (np.cumsum(n_cand) - n_cand).astype(np.int32)
    utt_of = np.repeat(np.arange(U, dtype=np.int32), n_cand)
    return tab, lens, ctx, n_cand, utt_of, row0


def align_args(ids, context_len, n_frames, B, vocab, n_text_ctx, max_batch, n_audio_ctx):
    """Checks an align call's arguments on the host (the library refuses the same with WM_E_ARG) -> (table, lengths, context
    lengths, n_frames [B] int32 or None).  ids / context_len: as score_args; n_frames: None (every column) or one count of real mel
    frames per row in [2, 2 * n_audio_ctx].  (Missing alignment heads are the library's to refuse: WM_E_STATE.)"""
    import numpy as np
    tab, lens, ctx = score_args(ids, context_len, B, vocab, n_text_ctx, max_batch)
    nf = None
    if n_frames is not None:
        nf = np.ascontiguousarray(np.asarray(n_frames, np.int64).reshape(-1))
        if nf.size != B:
            raise ValueError(f"n_frames needs one entry per row ({B}), got {nf.size}")
        if nf.min() < 2 or nf.max() > 2 * n_audio_ctx:
            raise ValueError(f"n_frames must lie in [2, {2 * n_audio_ctx}]")
        nf = nf.astype(np.int32)
    return tab, lens, ctx, nf


class WhisperMiError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WhisperMiError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py build` "
                             "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_void_p
    L.wm_last_error.restype = C.c_char_p
    if not hasattr(L, "wm_abi_version") or L.wm_abi_version() != ABI_VERSION:
        got = L.wm_abi_version() if hasattr(L, "wm_abi_version") else "none"
        raise WhisperMiError(f"{LIB_PATH} speaks ABI version {got}, this binding {ABI_VERSION}: rebuild the library "
                             "(python __graft_entry__.py build)")
    L.wm_model_load.argtypes = [C.c_char_p, C.POINTER(WmConfig), C.c_int, C.POINTER(vp)]
    L.wm_model_load_memory.argtypes = [fp, C.c_size_t, C.POINTER(WmConfig), C.c_int, C.POINTER(vp)]
    L.wm_model_free.argtypes = [vp]
    L.wm_model_free.restype = None
    L.wm_weight_count.argtypes = [C.POINTER(WmDims)]
    L.wm_weight_count.restype = C.c_size_t
    L.wm_weights_convert_v2.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(WmDims), C.c_int, C.c_int]
    L.wm_weights_read.argtypes = [C.c_char_p, C.POINTER(WmDims), fp]
    L.wm_state_new.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.wm_state_reset.argtypes = [vp]
    L.wm_state_free.argtypes = [vp]
    L.wm_state_free.restype = None
    L.wm_state_len.argtypes = [vp]
    L.wm_encode.argtypes = [vp, vp, vp, C.c_int, C.c_int, fp]
    L.wm_state_set_encoder_output.argtypes = [vp, vp, fp, C.c_int]
    L.wm_decode_step.argtypes = [vp, vp, ip, C.c_int, ip, fp, ip]
    L.wm_transcribe.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip]
    L.wm_transcribe_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts)]
    L.wm_transcribe_wait.argtypes = [vp, C.c_int, ip, ip]
    L.wm_transcribe_steps.argtypes = [vp, C.c_int]
    L.wm_transcribe_wait_device.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int]
    L.wm_log_mel.argtypes = [vp, fp, ip, C.c_int, C.c_int, fp]
    L.wm_transcribe_pcm.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip]
    L.wm_set_alignment_heads.argtypes = [vp, ip, C.c_int]
    L.wm_transcribe_tt.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, ip, fp]
    L.wm_transcribe_submit_tt.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip]
    L.wm_transcribe_wait_tt.argtypes = [vp, C.c_int, ip, ip, fp]
    L.wm_transcribe_pcm_tt.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, fp]
    L.wm_alignment_weights.argtypes = [vp, C.c_int, fp]
    L.wm_op_token_times.argtypes = [fp, fp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wm_log_mel_long.argtypes = [vp, fp, ip, C.c_int, C.c_int, fp, ip]
    L.wm_transcribe_long.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.POINTER(WmDecodeOpts), C.POINTER(vp)]
    L.wm_transcribe_long_pcm.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), C.POINTER(vp)]
    L.wm_long_result_sizes.argtypes = [vp, C.c_int, ip, ip]
    L.wm_long_result_get.argtypes = [vp, C.c_int, ip, C.POINTER(WmSegment)]
    L.wm_long_result_stats.argtypes = [vp, ip, ip, ip, ip]
    L.wm_long_result_prompt_stats.argtypes = [vp, ip, ip]
    L.wm_long_result_free.argtypes = [vp]
    L.wm_long_result_free.restype = None
    L.wm_op_long_segments.argtypes = [ip, C.c_int, C.c_int, C.c_int64, C.c_int, C.POINTER(WmSegment), ip, ip]
    L.wm_transcribe_rows.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, ip, ip]
    L.wm_transcribe_submit_rows.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int]
    L.wm_transcribe_long_ex.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), C.POINTER(vp)]
    L.wm_transcribe_long_pcm_ex.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), C.POINTER(vp)]
    L.wm_op_long_prompt.argtypes = [ip, C.POINTER(WmSegment), C.c_int, ip, C.c_int, C.POINTER(WmLongOpts), C.c_int, C.c_int, ip, ip]
    L.wm_op_attention_cached_lo.argtypes = [fp] * 4 + [C.c_int] * 9 + [ip]
    L.wm_op_matmul_nt.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wm_op_mlp_block.argtypes = [fp] * 10 + [C.c_int] * 5
    L.wm_op_ln_matmul_nt.argtypes = [fp] * 6 + [C.c_int] * 5
    L.wm_op_attention.argtypes = [fp] * 4 + [C.c_int] * 3
    L.wm_op_attention_cached.argtypes = [fp] * 4 + [C.c_int] * 9
    L.wm_op_attention_cached_map.argtypes = [fp] * 4 + [C.c_int] * 9 + [ip, C.c_int]
    L.wm_op_dec_linear.argtypes = [fp] * 7 + [C.c_int] * 8 + [fp, fp] + [C.c_int] * 5 + [fp, C.POINTER(C.c_int8)] + [C.c_int] * 3
    L.wm_op_dec_linear_long.argtypes = L.wm_op_dec_linear.argtypes
    L.wm_op_layer_norm.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.c_float]
    L.wm_op_layer_norm_t.argtypes = [fp] * 5 + [C.c_int, C.c_int, C.c_float, C.c_int]
    L.wm_op_attention_batch.argtypes = [fp] * 4 + [C.c_int] * 4
    L.wm_op_gemm_nt_epi.argtypes = ([fp, C.c_size_t, fp, C.c_size_t, fp, fp, fp, fp, C.c_size_t] + [C.c_int] * 4 + [C.c_longlong] * 6 +
                                    [C.c_int] * 4 + [C.c_longlong, C.c_int, C.c_int, ip])
    L.wm_op_gemm_nt_ring.argtypes = L.wm_op_gemm_nt_epi.argtypes[:-1] + [fp] * 5 + [C.c_size_t, ip]
    L.wm_op_gelu.argtypes = [fp, C.c_size_t, C.c_int]
    L.wm_op_softmax_rows.argtypes = [fp, C.c_int, C.c_int]
    L.wm_op_conv1d_k3.argtypes = [fp, fp, fp, fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]
    L.wm_op_argmax.argtypes = [fp, C.c_int, ip]
    L.wm_op_logits.argtypes = [fp, ip, fp, fp, fp, fp, fp, ip] + [C.c_int] * 5
    L.wm_op_logits_lp.argtypes = [fp, ip, fp, fp, fp, fp, fp, fp, ip] + [C.c_int] * 5
    L.wm_transcribe_lp.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, ip, ip, fp, fp]
    L.wm_transcribe_submit_lp.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int]
    L.wm_transcribe_wait_lp.argtypes = [vp, C.c_int, ip, ip, fp, fp]
    L.wm_transcribe_lp_ns.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, C.c_int, C.c_int, ip, ip, fp, fp, fp]
    L.wm_transcribe_submit_lp_ns.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, C.c_int, C.c_int]
    L.wm_transcribe_wait_lp_ns.argtypes = [vp, C.c_int, ip, ip, fp, fp, fp]
    L.wm_op_no_speech.argtypes = [fp] * 6 + [C.c_int] * 5
    L.wm_detect_language.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, fp]
    L.wm_transcribe_lang.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, C.c_int, C.c_int, ip, C.c_int,
                                     ip, ip, fp, fp, fp, ip, fp]
    L.wm_transcribe_submit_lang.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), ip, ip, C.c_int, C.c_int, C.c_int,
                                            ip, C.c_int, C.c_int]
    L.wm_transcribe_wait_lang.argtypes = [vp, C.c_int, ip, ip, fp, fp, fp, ip, fp]
    L.wm_transcribe_long_lang.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), ip, C.c_int, ip,
                                          C.POINTER(vp)]
    L.wm_transcribe_long_pcm_lang.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), ip, C.c_int, ip,
                                              C.POINTER(vp)]
    L.wm_transcribe_long_tt.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), ip, C.c_int, ip,
                                        C.c_int, C.POINTER(vp)]
    L.wm_transcribe_long_pcm_tt.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.POINTER(WmDecodeOpts), C.POINTER(WmLongOpts), ip, C.c_int, ip,
                                            C.c_int, C.POINTER(vp)]
    L.wm_long_result_token_times.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    L.wm_op_long_token_times.argtypes = [fp, C.c_int, C.c_int64, C.POINTER(WmSegment), C.c_int, C.POINTER(C.c_double), ip]
    L.wm_op_lang_detect.argtypes = [ip, fp, fp, fp, fp, fp, ip] + [C.c_int] * 5
    L.wm_score.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, fp, ip, fp, fp]
    L.wm_score_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip]
    L.wm_score_wait.argtypes = [vp, C.c_int, fp, ip, fp, fp]
    L.wm_score_pcm.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, fp, ip, fp, fp]
    L.wm_score_phases.argtypes = [vp, C.c_int, fp]
    L.wm_score_nbest.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, ip, ip, C.c_int, ip, fp, ip, fp, fp, ip, ip, fp]
    L.wm_score_nbest_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, ip, C.c_int, C.c_int, ip, ip, C.c_int, ip]
    L.wm_score_nbest_wait.argtypes = [vp, C.c_int, fp, ip, fp, fp, ip, ip, fp]
    L.wm_score_nbest_pcm.argtypes = [vp, fp, ip, C.c_int, C.c_int, ip, C.c_int, C.c_int, ip, ip, C.c_int, ip, fp, ip, fp, fp, ip, ip, fp]
    L.wm_op_score_rank.argtypes = [ip, ip, fp, fp, ip, C.c_int]
    L.wm_op_score_logits.argtypes = [fp, ip, fp, fp, fp, fp, ip] + [C.c_int] * 4
    L.wm_align.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, ip, fp, fp, fp, fp]
    L.wm_align_submit.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, ip, C.c_int]
    L.wm_align_wait.argtypes = [vp, C.c_int, fp, fp, fp, fp]
    L.wm_align_pcm.argtypes = [vp, fp, ip, C.c_int, C.c_int, C.c_int, ip, ip, C.c_int, ip, fp, fp, fp, fp]
    L.wm_align_phases.argtypes = [vp, C.c_int, fp]
    L.wm_op_dec_linear_capmap.argtypes = [fp] * 7 + [C.c_int] * 4 + [C.POINTER(C.c_int8), C.c_int, ip, C.c_int]
    L.wm_op_token_times_rows.argtypes = [fp, fp] + [C.c_int] * 4 + [ip, ip, ip, C.c_int]
    L.wm_op_align_probs.argtypes = [fp, fp, fp, C.c_int, fp, fp, ip, C.c_int, ip] + [C.c_int] * 5
    L.wm_op_align_norm.argtypes = [fp, fp] + [C.c_int] * 4 + [ip, ip]
    L.wm_long_result_quality.argtypes = [vp, C.c_int, fp, fp]
    L.wm_long_result_windows.argtypes = [vp, C.c_int, ip, C.POINTER(C.c_int64), fp, fp, ip]
    L.wm_long_result_skip_stats.argtypes = [vp, ip]
    L.wm_op_xattn.argtypes = [fp] * 6 + [C.c_int] * 7
    L.wm_op_xattn_map.argtypes = [fp] * 6 + [C.c_int] * 7 + [ip]
    L.wm_op_xattn_absorb.argtypes = [fp] * 3 + [C.c_int] * 3
    L.wm_bench_kernel.argtypes = [vp, vp, C.c_int, C.c_int, fp]
    L.wm_bench_bytes.argtypes = [vp, vp, C.c_int, C.POINTER(C.c_double)]
    L.wm_synth_weights.argtypes = [C.POINTER(WmDims), C.c_uint64, fp]
    L.wm_synth_weights.restype = C.c_size_t
    L.wm_synth_mel_host.argtypes = [C.c_uint64, C.c_int, C.c_int, fp]
    L.wm_synth_mel_host.restype = None
    up = C.POINTER(C.c_uint32)
    L.wm_set_repeat_options.argtypes = [vp, C.c_float, C.c_int]
    L.wm_op_logits_processed.argtypes = [fp, ip, fp, fp, fp, fp, fp, fp, ip, C.c_int, up, up, C.c_float] + [C.c_int] * 4
    L.wm_op_repeat_sets.argtypes = [up, up, ip, ip, ip] + [C.c_int] * 5
    L.wm_set_constraint.argtypes = [vp, ip, ip, C.c_int, C.c_int]
    L.wm_transcribe_constraint_match.argtypes = [vp, C.c_int, ip, C.c_int]
    L.wm_op_constraint_states.argtypes = [ip, up, ip, ip, ip] + [C.c_int] * 5 + [ip, ip] + [C.c_int] * 3
    L.wm_set_top_k.argtypes = [vp, C.c_int]
    L.wm_transcribe_top_k.argtypes = [vp, C.c_int, ip, fp]
    L.wm_op_logits_topk.argtypes = [fp, ip, fp, ip, fp, C.c_int, fp, fp, fp, fp, fp, ip, C.c_int, up, up, C.c_float] + [C.c_int] * 4
    L.wm_set_sequence_bias.argtypes = [vp, ip, ip, fp, C.c_int, ip, ip, C.c_int]
    L.wm_op_logits_seq_bias.argtypes = [fp, ip, fp, fp, fp, fp, fp, fp, ip, C.c_int, up, up, C.c_float, up, ip, C.c_int, fp, ip] + [C.c_int] * 4
    L.wm_op_seq_bias_hits.argtypes = [up, fp, ip, ip, ip, ip, ip, ip] + [C.c_int] * 4 + [ip, ip, fp, C.c_int, ip, ip, C.c_int, C.c_int]
    L.wm_chunk_table.argtypes = [ip] + [C.c_int] * 5 + [ip, C.c_int, ip]
    L.wm_transcribe_chunked.argtypes = [vp, vp, C.c_int, ip] + [C.c_int] * 5 + [C.POINTER(WmDecodeOpts), ip, C.c_int, C.c_int, ip, ip, C.c_int,
                                                                               ip, ip, ip]
    L.wm_op_chunk_gather.argtypes = [fp, fp, C.c_int, C.c_int64, ip, C.c_int, C.c_int]
    L.wm_op_chunk_merge.argtypes = [ip] * 5 + [C.c_int] * 5
    dp = C.POINTER(C.c_double)
    L.wm_transcribe_chunked_ts.argtypes = [vp, vp, C.c_int, ip] + [C.c_int] * 5 + [C.POINTER(WmDecodeOpts), ip, C.c_int, C.c_int, C.c_int, C.c_double,
                                                                                  ip, ip, C.c_int, ip, dp, ip, C.c_int, dp, ip, ip, fp, ip]
    L.wm_op_chunk_segments.argtypes = [ip, ip, ip, fp, ip] + [C.c_int] * 5 + [C.c_double, C.c_int, ip, ip, C.c_int, ip, dp, ip, C.c_int, dp]
    i64 = C.c_int64
    L.wm_resample_len.argtypes = [i64, C.c_int, C.POINTER(i64)]
    L.wm_resample_pcm.argtypes = [vp, vp, C.c_int, C.c_int, ip, C.c_int, i64, C.c_int, vp, C.c_int, i64, ip]
    L.wm_op_resample.argtypes = [fp, vp, C.c_int, ip, C.c_int, i64, C.c_int, i64, ip]
    L.wm_op_resample_taps.argtypes = [C.c_int, fp, i64, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.wm_op_fe_tables.argtypes = [C.c_int, fp, fp, fp, ip]
    L.wm_op_fe_frames.argtypes = [fp, fp, ip] + [C.c_int] * 4
    L.wm_op_fe_mel_log.argtypes = [fp, fp] + [C.c_int] * 5
    L.wm_op_fe_mel_norm.argtypes = [fp, fp, C.c_int, i64, C.c_int]
    L.wm_op_window_gather.argtypes = [fp, fp, ip] + [C.c_int] * 5
    L.wm_op_ts_states.argtypes = [ip] * 12 + [C.c_int] * 8
    L.wm_op_init_tokens.argtypes = [ip] * 7 + [fp, fp, ip, ip, C.c_int, ip] + [C.c_int] * 10
    L.wm_op_set_rows_step.argtypes = [ip, ip, ip] + [C.c_int] * 4
    L.wm_op_set_step.argtypes = [ip, ip, ip] + [C.c_int] * 6
    L.wm_op_pack_tokens.argtypes = [ip, ip, ip] + [C.c_int] * 5
    L.wm_op_dec_embed.argtypes = [fp, fp, fp, ip, ip] + [C.c_int] * 5
    L.wm_op_rows_copy.argtypes = [fp, fp, ip] + [C.c_int] * 3
    L.wm_op_mel_transpose_pad.argtypes = [fp, fp] + [C.c_int] * 5
    _lib = L
    return L


FIRST_SPECIAL = 50257  # the multilingual vocabulary's first special id (<|endoftext|>): what the chunked stitch strips from
CHUNK_MERGE_MAX_IDS = 2048  # wm_kernels.h CHUNK_MERGE_MAX_IDS


def chunk_strides(chunk_length_s, stride_length_s, sampling_rate=16000):
    """HF AutomaticSpeechRecognitionPipeline.preprocess' seconds -> samples (Whisper: align_to = 1): (chunk_len, stride_left,
    stride_right).  stride_length_s: None (chunk_length_s / 6 on both sides), one number, or (left, right)."""
    if stride_length_s is None:
        stride_length_s = chunk_length_s / 6
    if isinstance(stride_length_s, (int, float)):
        stride_length_s = [stride_length_s, stride_length_s]
    if len(stride_length_s) != 2:
        raise ValueError("stride_length_s is None, one number or (left, right)")
    return (int(round(chunk_length_s * sampling_rate)), int(round(stride_length_s[0] * sampling_rate)),
            int(round(stride_length_s[1] * sampling_rate)))


def chunk_table(n_samples, chunk_len=480000, stride_left=None, stride_right=None, window=0):
    """wm_chunk_table (host only): HF chunk_iter's chunks of recordings of n_samples[r] samples -> int32 array [n, 6] of
    (recording, start, len, stride_left_eff, stride_right_eff, is_last).  The strides default to chunk_len // 6.  window > 0: the
    model's window in samples, chunk_len beyond it is refused.  WhisperMiError (WM_E_ARG) where HF raises."""
    import numpy as np
    ns = np.ascontiguousarray(np.asarray(n_samples, np.int64).reshape(-1))
    if ns.size < 1 or ns.min() < 0 or ns.max() >= 2 ** 31:
        raise ValueError("n_samples needs one length in [0, 2^31) per recording")
    ns = ns.astype(np.int32)
    sl = chunk_len // 6 if stride_left is None else int(stride_left)
    sr = chunk_len // 6 if stride_right is None else int(stride_right)
    ip = C.POINTER(C.c_int32)
    n = C.c_int32()
    check(lib().wm_chunk_table(ns.ctypes.data_as(ip), ns.size, int(chunk_len), sl, sr, int(window), None, 0, C.byref(n)))
    tab = np.zeros((max(1, n.value), 6), np.int32)
    check(lib().wm_chunk_table(ns.ctypes.data_as(ip), ns.size, int(chunk_len), sl, sr, int(window), tab.ctypes.data_as(ip), n.value, C.byref(n)))
    return tab[:n.value]


def op_chunk_gather(pcm, items, N, fill=0.0):
    """wm_op_chunk_gather: pcm [R, T_max] float32, items [(recording, start, len)] -> [n, N]; the output starts as `fill` everywhere, so
    a cell the kernel does not store shows."""
    import numpy as np
    p = np.ascontiguousarray(pcm, np.float32)
    it = np.ascontiguousarray(np.asarray(items, np.int32).reshape(-1, 3))
    out = np.full((it.shape[0], int(N)), fill, np.float32)
    check(lib().wm_op_chunk_gather(out.ctypes.data_as(C.POINTER(C.c_float)), p.ctypes.data_as(C.POINTER(C.c_float)), p.shape[0], p.shape[1],
                                   it.ctypes.data_as(C.POINTER(C.c_int32)), it.shape[0], int(N)))
    return out


def op_chunk_merge(recordings, first_special=FIRST_SPECIAL, fill=-7):
    """wm_op_chunk_merge: recordings = one list of id lists (chunks, in order) per recording -> one merged id list per recording, all
    recordings in one launch.  Cells of the output past each length must still hold `fill` (AssertionError)."""
    import numpy as np
    rows = [np.asarray(ch, np.int32).reshape(-1) for rec in recordings for ch in rec]
    off = np.zeros(len(recordings) + 1, np.int32)
    off[1:] = np.cumsum([len(rec) for rec in recordings])
    if not rows:
        rows = [np.zeros(0, np.int32)]  # (the library wants one row; no recording owns it)
    stride = max(1, max(r.size for r in rows))
    ids = np.zeros((len(rows), stride), np.int32)
    lens = np.asarray([r.size for r in rows], np.int32)
    for k, r in enumerate(rows):
        ids[k, :r.size] = r
    cap = max(1, max([sum(len(ch) for ch in rec) for rec in recordings] + [1]))
    merged = np.full((len(recordings), cap + 8), fill, np.int32)
    mlen = np.zeros(len(recordings), np.int32)
    ip = C.POINTER(C.c_int32)
    check(lib().wm_op_chunk_merge(merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), ids.ctypes.data_as(ip), lens.ctypes.data_as(ip),
                                  off.ctypes.data_as(ip), len(rows), len(recordings), stride, cap + 8, int(first_special)))
    for r in range(len(recordings)):
        assert (merged[r, mlen[r]:] == fill).all(), f"recording {r}: the kernel stored past its length"
    return [merged[r, :mlen[r]].tolist() for r in range(len(recordings))]


def op_chunk_segments(recordings, word, timestamp_begin, first_special, time_precision, segment_size, cap_extra=8, seg_cap=None, cap=None,
                      fill=-7):
    """wm_op_chunk_segments: recordings = per recording a list of chunks (ids, (len, stride_left, stride_right) in samples, token times
    or None), all recordings in one launch -> per recording the segments [{"timestamp": (start, end | None), "ids", "token_timestamps"
    (word)}].  Every output starts as a sentinel; cells past what a recording produced must still hold it (AssertionError).
    cap / seg_cap: capacities to force (default: what the recording can need + cap_extra)."""
    import numpy as np
    chunks = [ch for rec in recordings for ch in rec]
    off = np.zeros(len(recordings) + 1, np.int32)
    off[1:] = np.cumsum([len(rec) for rec in recordings])
    n_rows = max(1, len(chunks))
    stride = max([1] + [len(ch[0]) for ch in chunks])
    ids, lens = np.zeros((n_rows, stride), np.int32), np.zeros(n_rows, np.int32)
    strides, times = np.zeros((n_rows, 3), np.int32), np.zeros((n_rows, stride), np.float32)
    for k, (i, st, tt) in enumerate(chunks):
        lens[k] = len(i)
        ids[k, :len(i)] = i
        strides[k] = st
        if word:
            times[k, :len(i)] = np.asarray(tt, np.float32)
    R = len(recordings)
    need = max([1] + [sum(len(ch[0]) for ch in rec) for rec in recordings])
    cap = need + cap_extra if cap is None else int(cap)
    seg_cap = need + 1 + cap_extra if seg_cap is None else int(seg_cap)
    NAN_FILL = np.float64(-12345.5)
    GUARD = 64  # cells behind every output that the library never hears of: a store past a capacity lands there
    merged_g, segt_g = np.full(R * cap + GUARD, fill, np.int32), np.full(R * seg_cap * 2 + GUARD, NAN_FILL, np.float64)
    segr_g, pairs_g = np.full(R * seg_cap * 2 + GUARD, fill, np.int32), np.full(R * cap * 2 + GUARD, NAN_FILL, np.float64)
    merged, segt = merged_g[:R * cap].reshape(R, cap), segt_g[:R * seg_cap * 2].reshape(R, seg_cap, 2)
    segr, pairs = segr_g[:R * seg_cap * 2].reshape(R, seg_cap, 2), pairs_g[:R * cap * 2].reshape(R, cap, 2)
    mlen, nseg = np.zeros(R, np.int32), np.zeros(R, np.int32)
    ip, dp, fp = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_float)
    rc = lib().wm_op_chunk_segments(ids.ctypes.data_as(ip), lens.ctypes.data_as(ip), strides.ctypes.data_as(ip), times.ctypes.data_as(fp) if word else None,
                                    off.ctypes.data_as(ip), n_rows, R, stride, int(first_special), int(timestamp_begin), float(time_precision),
                                    int(segment_size), merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), cap, nseg.ctypes.data_as(ip),
                                    segt.ctypes.data_as(dp), segr.ctypes.data_as(ip), seg_cap, pairs.ctypes.data_as(dp) if word else None)
    assert (merged_g[R * cap:] == fill).all() and (segr_g[R * seg_cap * 2:] == fill).all(), "a store past an output's capacity"
    assert (segt_g[R * seg_cap * 2:] == NAN_FILL).all() and (pairs_g[R * cap * 2:] == NAN_FILL).all(), "a store past an output's capacity"
    for r in range(R):  # also on a refusal: nothing was stored past what was produced
        assert (merged[r, min(mlen[r], cap):] == fill).all(), f"recording {r}: ids stored past the length"
        k = min(max(nseg[r], 0), seg_cap)
        assert (segr[r, k:] == fill).all() and (segt[r, k:] == NAN_FILL).all(), f"recording {r}: segments stored past the count"
        assert (pairs[r, min(mlen[r], cap) if word else 0:] == NAN_FILL).all(), f"recording {r}: pairs stored past the length"
    check(rc)
    out = []
    for r in range(R):
        m, segs = merged[r, :mlen[r]].tolist(), []
        for k in range(nseg[r]):
            (s, e), (b0, b1) = segt[r, k].tolist(), segr[r, k].tolist()
            seg = {"timestamp": (None if s != s else s, None if e != e else e), "ids": m[b0:b1]}
            if word:
                seg["token_timestamps"] = [tuple(p) for p in pairs[r, b0:b1].tolist()]
            segs.append(seg)
        assert not segs or (segs and segr[r, nseg[r] - 1, 1] == mlen[r] and segr[r, 0, 0] == 0)
        out.append(segs)
    return out


WM_F32, WM_I16 = 0, 3  # include/whisper_mi.h: the input dtypes of the resampling entries


def resample_len(n_in, sr_in):
    """wm_resample_len (host only): samples at 16 kHz of a row of n_in samples at sr_in."""
    n = C.c_int64()
    check(lib().wm_resample_len(int(n_in), int(sr_in), C.byref(n)))
    return n.value


def resample_taps(sr_in):
    """wm_op_resample_taps (host only): (h [new, 2 * width + orig] float32, orig, new, width) of the sinc table for sr_in -> 16 kHz."""
    import numpy as np
    o, n, w = C.c_int(), C.c_int(), C.c_int()
    check(lib().wm_op_resample_taps(int(sr_in), None, 0, C.byref(o), C.byref(n), C.byref(w)))
    h = np.zeros((n.value, 2 * w.value + o.value), np.float32)
    check(lib().wm_op_resample_taps(int(sr_in), h.ctypes.data_as(C.POINTER(C.c_float)), h.size, C.byref(o), C.byref(n), C.byref(w)))
    return h, o.value, n.value, w.value


def pack_pcm(rows):
    """Rows of PCM -> ([B, stride] buffer, lengths [B] int32, dtype code): int16 when every row is np.int16, else float32 (an int16 row
    among float rows is scaled by 1 / 32768 here, which is exact)."""
    import numpy as np
    rows = [np.asarray(r).reshape(-1) for r in rows]
    if not rows:
        raise ValueError("no recording")
    i16 = all(r.dtype == np.int16 for r in rows)
    n = np.asarray([r.size for r in rows], np.int64)
    if n.max() >= 2 ** 31:
        raise ValueError("a row has 2^31 samples or more")
    buf = np.zeros((len(rows), max(1, int(n.max()))), np.int16 if i16 else np.float32)
    for b, r in enumerate(rows):
        buf[b, :r.size] = r if i16 or r.dtype != np.int16 else r.astype(np.float32) / 32768.0
    return buf, n.astype(np.int32), WM_I16 if i16 else WM_F32


def op_resample(rows, sr_in, fill=-7.0, stride_out=None, in_dtype=None):
    """wm_op_resample: resample_kernel alone on rows of float32 or int16 PCM -> (out [B, stride_out] float32, n_out [B]); out starts as
    `fill` everywhere, so a cell the kernel does not store shows.  stride_out: None = the longest row's output + 8."""
    import numpy as np
    buf, n, dt = pack_pcm(rows)
    if stride_out is None:
        stride_out = max(resample_len(int(v), sr_in) for v in n) + 8
    out = np.full((len(rows), int(stride_out)), fill, np.float32)
    n_out = np.full(len(rows), -1, np.int32)
    ip = C.POINTER(C.c_int32)
    check(lib().wm_op_resample(out.ctypes.data_as(C.POINTER(C.c_float)), buf.ctypes.data_as(C.c_void_p), dt if in_dtype is None else int(in_dtype),
                               n.ctypes.data_as(ip), len(rows), buf.shape[1], int(sr_in), int(stride_out), n_out.ctypes.data_as(ip)))
    return out, n_out


REPEAT_NGRAM_MAX = 64  # wm_kernels.h REPEAT_NGRAM_MAX


def repeat_args(repetition_penalty, no_repeat_ngram_size):
    """Checks HF generate's repetition_penalty / no_repeat_ngram_size on the host (the library refuses the same with WM_E_ARG) ->
    (penalty, n) as wm_set_repeat_options takes them: None means off (1.0 / 0)."""
    p = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not (p > 0.0) or p != p or p == float("inf"):
        raise ValueError(f"repetition_penalty must be a finite float > 0 (got {repetition_penalty!r})")
    n = 0 if no_repeat_ngram_size is None else no_repeat_ngram_size
    if isinstance(n, bool) or int(n) != n:
        raise ValueError(f"no_repeat_ngram_size must be an integer (got {no_repeat_ngram_size!r})")
    n = int(n)
    if n < 0 or n > REPEAT_NGRAM_MAX:
        raise ValueError(f"no_repeat_ngram_size must lie in [0, {REPEAT_NGRAM_MAX}] (got {n})")
    return p, n


TOPK_MAX = 8  # wm_kernels.h TOPK_MAX


def top_k_arg(top_k, return_logprobs):
    """Checks top_k on the host (the library refuses the same with WM_E_ARG) -> k as wm_set_top_k takes it: None means off (0).
    ValueError: not an integer of [1, 8], or without return_logprobs (the alternatives' log-probs share the chosen id's normaliser)."""
    if top_k is None:
        return 0
    if isinstance(top_k, bool) or int(top_k) != top_k:
        raise ValueError(f"top_k must be an integer (got {top_k!r})")
    k = int(top_k)
    if k < 1 or k > TOPK_MAX:
        raise ValueError(f"top_k must lie in [1, {TOPK_MAX}] (got {k})")
    if not return_logprobs:
        raise ValueError("top_k needs return_logprobs=True")
    return k


CONSTRAINT_PHRASES_MAX, CONSTRAINT_LEN_MAX, CONSTRAINT_NODES_MAX = 4096, 64, 65536  # wm_kernels.h


def constraint_trie(phrases):
    """The trie of a list of phrases (id tuples), flattened as wm_set_constraint flattens it -> (edge_off [n + 1],
    edge_id, edge_next, terminal [n]) int32: node v's child edges are edge_id / edge_next [edge_off[v] : edge_off[v + 1]], ids
    ascending; terminal[v] = the index of the phrase that ends at v, or -1.  Node 0 is the root, nodes are numbered in the order the
    phrases, taken in the caller's order and id by id, first reach them, and the last node is the dead node: no edges, no phrase.
    ValueError: a duplicate phrase, more than CONSTRAINT_NODES_MAX nodes."""
    import numpy as np
    kids, term = [{}], [-1]
    for q, ph in enumerate(phrases):
        v = 0
        for t in ph:
            nxt = kids[v].get(t)
            if nxt is None:
                if len(kids) + 2 > CONSTRAINT_NODES_MAX:
                    raise ValueError(f"constraint: more than {CONSTRAINT_NODES_MAX} trie nodes")
                nxt = kids[v][t] = len(kids)
                kids.append({})
                term.append(-1)
            v = nxt
        if term[v] >= 0:
            raise ValueError(f"constraint: phrase {list(ph)} is given twice")
        term[v] = q
    kids.append({})
    term.append(-1)
    off, eid, enx = [0], [], []
    for k in kids:
        for t in sorted(k):
            eid.append(t)
            enx.append(k[t])
        off.append(len(eid))
    return np.asarray(off, np.int32), np.asarray(eid, np.int32), np.asarray(enx, np.int32), np.asarray(term, np.int32)


def constraint_args(constraint, free_from, vocab, eot, timestamps=None):
    """Checks constraint= (a list of phrases, each a non-empty list of ids) and free_from= on the host (the library refuses the same
    with WM_E_ARG) -> None when constraint is None, else (key, [ids, offsets, n_phrases, free_from]) as wm_set_constraint takes them;
    key is hashable and equal for equal phrases in equal order under an equal free_from.  free_from None: the first timestamp id
    when the timestamp rules are on, else no free ids (-1)."""
    import numpy as np
    if constraint is None:
        if free_from is not None:
            raise ValueError("free_from without constraint")
        return None
    try:
        items = list(constraint)
    except TypeError:
        raise ValueError(f"constraint: a list of phrases, each a list of ids (got {constraint!r})")
    if not items:
        raise ValueError("constraint: an empty list of phrases (use None for off)")
    if len(items) > CONSTRAINT_PHRASES_MAX:
        raise ValueError(f"constraint: at most {CONSTRAINT_PHRASES_MAX} phrases (got {len(items)})")
    if free_from is None:
        ff = int(timestamps[0]) if timestamps is not None else -1
    else:
        if isinstance(free_from, bool) or not isinstance(free_from, (int, np.integer)):
            raise ValueError(f"free_from must be an id (got {free_from!r})")
        ff = int(free_from)
    if ff < 0 or ff > vocab:
        ff = vocab
    out = []
    for s in items:
        try:
            t = tuple(s)
        except TypeError:
            raise ValueError(f"constraint: every phrase is a list of ids (got {s!r})")
        if not 1 <= len(t) <= CONSTRAINT_LEN_MAX:
            raise ValueError(f"constraint: a phrase has 1..{CONSTRAINT_LEN_MAX} ids (got {len(t)})")
        for i in t:
            if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < vocab:
                raise ValueError(f"constraint: id {i!r} is not an integer inside the vocabulary of {vocab}")
            if int(i) == int(eot):
                raise ValueError(f"constraint: a phrase holds the eot {eot}")
            if int(i) >= ff:
                raise ValueError(f"constraint: a phrase holds the free id {int(i)} (free_from {ff})")
        out.append(tuple(int(i) for i in t))
    constraint_trie(out)  # a duplicate phrase, too many nodes
    ids = np.asarray([i for t in out for i in t], np.int32)
    off = np.concatenate([[0], np.cumsum([len(t) for t in out])]).astype(np.int32)
    return (tuple(out), ff), [ids, off, len(out), ff]


SEQ_BIAS_MAX, SEQ_BIAS_LEN_MAX = 1024, 32  # wm_kernels.h


def seq_bias_args(sequence_bias, bad_words_ids, vocab):
    """Checks HF generate's sequence_bias ({(ids...): bias} or [[[ids...], bias], ...]) and bad_words_ids ([[ids...], ...]) on the
    host (the library refuses the same with WM_E_ARG) -> None when both are empty, else (key, [ids, offsets, bias, n_seq, bad_ids,
    bad_offsets, n_bad]) as wm_set_sequence_bias takes them; key is hashable and equal for equal lists in equal order."""
    import numpy as np
    if sequence_bias is None:
        seqs = []
    elif isinstance(sequence_bias, dict):
        seqs = list(sequence_bias.items())
    else:
        seqs = [(s[0], s[1]) for s in sequence_bias]
    bad = [] if bad_words_ids is None else list(bad_words_ids)
    out = []
    for what, items in (("sequence_bias", [s for s, _ in seqs]), ("bad_words_ids", bad)):
        had = set()
        for s in items:
            try:
                t = tuple(s)
            except TypeError:
                raise ValueError(f"{what}: every sequence is a list of ids (got {s!r})")
            if not 1 <= len(t) <= SEQ_BIAS_LEN_MAX:
                raise ValueError(f"{what}: a sequence has 1..{SEQ_BIAS_LEN_MAX} ids (got {len(t)})")
            for i in t:
                if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= int(i) < vocab:
                    raise ValueError(f"{what}: id {i!r} is not an integer inside the vocabulary of {vocab}")
            t = tuple(int(i) for i in t)
            if t in had:
                raise ValueError(f"{what}: sequence {list(t)} is given twice")
            had.add(t)
            out.append(t)
    n_seq, n_bad = len(seqs), len(bad)
    if n_seq + n_bad > SEQ_BIAS_MAX:
        raise ValueError(f"at most {SEQ_BIAS_MAX} sequences over sequence_bias and bad_words_ids together (got {n_seq + n_bad})")
    bias = []
    for _, b in seqs:
        if isinstance(b, bool) or not isinstance(b, (int, float, np.integer, np.floating)):
            raise ValueError(f"sequence_bias: a bias is a float (got {b!r})")
        b = float(np.float32(b))
        if b != b or b == float("inf"):
            raise ValueError("sequence_bias: a bias is a finite float or -inf")
        bias.append(b)
    if n_seq + n_bad == 0:
        return None

    def pack(ts):
        ids = np.asarray([i for t in ts for i in t], np.int32)
        off = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int32)
        return ids, off

    ids, off = pack(out[:n_seq])
    bids, boff = pack(out[n_seq:])
    key = (tuple(out[:n_seq]), tuple(np.float32(b).tobytes() for b in bias), tuple(out[n_seq:]))
    return key, [ids if n_seq else None, off if n_seq else None, np.asarray(bias, np.float32) if n_seq else None, n_seq,
                 bids if n_bad else None, boff if n_bad else None, n_bad]


def long_tt_args(return_token_timestamps, logprob_threshold, no_speech_threshold):
    """Checks the long-form token-timestamp flag on the host (the library refuses the same with WM_E_ARG) -> bool."""
    tt = bool(return_token_timestamps)
    if tt and (logprob_threshold is not None or no_speech_threshold is not None):
        raise ValueError("return_token_timestamps does not combine with logprob_threshold / no_speech_threshold")
    return tt


def long_token_times(rel, seek: int, segs):
    """wm_op_long_token_times (host only): rel = the window-relative float32 times of a window's generated ids (eot
    dropped), segs = long_segments' (first, count, start, end) of those ids -> float64 array, one time per id a segment keeps."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(rel, np.float32).reshape(-1))
    sg = (WmSegment * max(1, len(segs)))(*[WmSegment(int(s[0]), int(s[1]), float(s[2]), float(s[3])) for s in segs])
    out = np.zeros(max(1, a.size), np.float64)
    n = C.c_int32()
    check(lib().wm_op_long_token_times(a.ctypes.data_as(C.POINTER(C.c_float)) if a.size else None, a.size, int(seek), sg, len(segs),
                                       out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
    return out[:n.value].copy()


def long_result(h, B: int, quality: bool = False, token_times: bool = False):
    """Reads and frees a wm_long_result handle of B utterances -> (per utterance {"sequence": [...], "segments": [{"start",
    "end", "tokens"}]}, {"windows", "stalled", "passes", "rows"}: windows decoded, windows that did not advance seek, passes
    run and rows those passes decoded; "longest_prompt", "row_passes": the longest decoder prompt a pass carried and how many
    passes went out as per-row passes).
    quality (a run with thresholds): every segment also carries its window's "avg_logprob" / "no_speech_prob", every
    utterance its window log "windows": [{"seek", "avg_logprob", "no_speech_prob", "skipped"}] in decode order, and the stats
    "skipped_windows".
    token_times (a run with token timestamps): every utterance also carries "token_times", a float64 array parallel to
    "sequence", and every segment "token_timestamps", its slice of that array."""
    import numpy as np
    L = lib()
    try:
        out = []
        n_tok, n_seg = C.c_int32(), C.c_int32()
        for b in range(B):
            check(L.wm_long_result_sizes(h, b, C.byref(n_tok), C.byref(n_seg)))
            toks = (C.c_int32 * max(1, n_tok.value))()
            segs = (WmSegment * max(1, n_seg.value))()
            check(L.wm_long_result_get(h, b, toks, segs))
            seq = list(toks[:n_tok.value])
            out.append({"sequence": seq, "segments": [{"start": s.start, "end": s.end, "tokens": seq[s.first:s.first + s.count]}
                                                      for s in segs[:n_seg.value]]})
            if token_times:
                tt = np.zeros(max(1, n_tok.value), np.float64)
                check(L.wm_long_result_token_times(h, b, tt.ctypes.data_as(C.POINTER(C.c_double))))
                out[-1]["token_times"] = tt[:n_tok.value]
                for sg, s in zip(out[-1]["segments"], segs[:n_seg.value]):
                    sg["token_timestamps"] = out[-1]["token_times"][s.first:s.first + s.count]
            if quality:
                qa, qn = (C.c_float * max(1, n_seg.value))(), (C.c_float * max(1, n_seg.value))()
                check(L.wm_long_result_quality(h, b, qa, qn))
                for i, sg in enumerate(out[-1]["segments"]):
                    sg["avg_logprob"], sg["no_speech_prob"] = float(qa[i]), float(qn[i])
                nw = C.c_int32()
                check(L.wm_long_result_windows(h, b, C.byref(nw), None, None, None, None))
                k = max(1, nw.value)
                ws, wa, wn, wk = (C.c_int64 * k)(), (C.c_float * k)(), (C.c_float * k)(), (C.c_int32 * k)()
                check(L.wm_long_result_windows(h, b, C.byref(nw), ws, wa, wn, wk))
                out[-1]["windows"] = [{"seek": int(ws[i]), "avg_logprob": float(wa[i]), "no_speech_prob": float(wn[i]),
                                       "skipped": bool(wk[i])} for i in range(nw.value)]
        st = [C.c_int32() for _ in range(4)]
        check(L.wm_long_result_stats(h, *[C.byref(v) for v in st]))
        stats = dict(zip(("windows", "stalled", "passes", "rows"), (v.value for v in st)))
        lp, rp = C.c_int32(), C.c_int32()
        check(L.wm_long_result_prompt_stats(h, C.byref(lp), C.byref(rp)))
        stats.update(longest_prompt=lp.value, row_passes=rp.value)
        if quality:
            sk = C.c_int32()
            check(L.wm_long_result_skip_stats(h, C.byref(sk)))
            stats["skipped_windows"] = sk.value
        return out, stats
    finally:
        L.wm_long_result_free(h)


def long_segments(ids, timestamp_begin: int, seek: int, seek_num_frames: int):
    """wm_op_long_segments (host-only HF _retrieve_segment): ([(first, count, start, end)], advance)."""
    import numpy as np
    a = np.ascontiguousarray(np.asarray(ids, np.int32).reshape(-1))
    segs = (WmSegment * max(1, a.size))()
    n, adv = C.c_int32(), C.c_int32()
    check(lib().wm_op_long_segments(a.ctypes.data_as(C.POINTER(C.c_int32)), a.size, timestamp_begin, seek, seek_num_frames, segs,
                                    C.byref(n), C.byref(adv)))
    return [(s.first, s.count, s.start, s.end) for s in segs[:n.value]], adv.value


def long_prompt(segments, init, timestamp_begin: int, n_text_ctx: int, prompt_ids=None, condition_on_prev_tokens=False,
                prompt_condition_type="first-segment", prev_sot_token=50361):
    """wm_op_long_prompt (host-only HF _prepare_decoder_input_ids for one utterance): segments = the utterance's segments so
    far (a list of id lists) -> the decoder prompt of its next window."""
    import numpy as np
    ip = C.POINTER(C.c_int32)
    seq = np.ascontiguousarray(np.asarray([t for sg in segments for t in sg], np.int32))
    segs = (WmSegment * max(1, len(segments)))()
    first = 0
    for i, sg in enumerate(segments):
        segs[i] = WmSegment(first, len(sg), 0.0, 0.0)
        first += len(sg)
    ini = np.ascontiguousarray(np.asarray(init, np.int32).reshape(-1))
    lo, _keep = long_opts(prompt_ids, condition_on_prev_tokens, prompt_condition_type, prev_sot_token)
    out = np.zeros(max(1, n_text_ctx), np.int32)
    n = C.c_int32()
    check(lib().wm_op_long_prompt(seq.ctypes.data_as(ip) if seq.size else None, segs, len(segments), ini.ctypes.data_as(ip), ini.size,
                                  C.byref(lo), timestamp_begin, n_text_ctx, out.ctypes.data_as(ip), C.byref(n)))
    return out[:n.value].tolist()


def check(rc: int):
    if rc != 0:
        raise WhisperMiError(f"libwhispermi error {rc}: {lib().wm_last_error().decode()}")
