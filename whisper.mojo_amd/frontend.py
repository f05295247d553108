"""Log-mel front end: the host-side equivalent of the reference's
`processor(audio, sampling_rate=16000, return_tensors="pt").input_features` (export_weights.py:116), computed on the GPU
through the C-ABI (wm_log_mel / wm_transcribe_pcm)."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib
from .config import EOT, MAX_LOOP, PROMPT

SAMPLING_RATE = 16000


def _pack(audios: Sequence[np.ndarray]):
    n = np.asarray([len(a) for a in audios], np.int32)
    stride = max(1, int(n.max()))
    buf = np.zeros((len(audios), stride), np.float32)
    for i, a in enumerate(audios):
        buf[i, :len(a)] = np.asarray(a, np.float32)
    return buf, n, stride


def _is_16k_f32(audios, sampling_rate) -> bool:
    """True for what every entry took before resampling existed: 16 kHz and no int16 row.  That input takes the old path untouched."""
    if isinstance(sampling_rate, bool) or int(sampling_rate) != sampling_rate:
        raise ValueError(f"sampling_rate must be an integer (got {sampling_rate!r})")
    if int(sampling_rate) <= 0:
        raise ValueError(f"sampling_rate must be positive (got {sampling_rate})")
    return int(sampling_rate) == SAMPLING_RATE and not any(isinstance(a, np.ndarray) and a.dtype == np.int16 for a in audios)


def _resample(model, audios, sampling_rate, on_device: bool):
    """wm_resample_pcm: rows of float32 or int16 PCM at sampling_rate -> 16 kHz float32 [B, stride] with lengths [B];
    on_device: a torch CUDA tensor on the model's GPU (the samples stay there), else a numpy array."""
    if model._h is None:
        raise _lib.WhisperMiError("model not loaded")
    buf, n, dt = _lib.pack_pcm(audios)
    stride = max(1, max(_lib.resample_len(int(v), sampling_rate) for v in n))
    n_out = np.zeros(len(n), np.int32)
    if on_device:
        import torch
        out = torch.empty((len(n), stride), dtype=torch.float32, device=f"cuda:{model.device}")
        torch.cuda.current_stream(out.device).synchronize()
        ptr = C.c_void_p(out.data_ptr())
    else:
        out = np.empty((len(n), stride), np.float32)
        ptr = out.ctypes.data_as(C.c_void_p)
    ip = C.POINTER(C.c_int32)
    _lib.check(_lib.lib().wm_resample_pcm(model._h, buf.ctypes.data_as(C.c_void_p), dt, 0, n.ctypes.data_as(ip), len(n), buf.shape[1],
                                          int(sampling_rate), ptr, int(on_device), stride, n_out.ctypes.data_as(ip)))
    return out, n_out


def resample(model, audios: Sequence[np.ndarray], sampling_rate: int) -> List[np.ndarray]:
    """PCM at any sample rate, float32 or np.int16 (scaled by 1 / 32768), -> a list of float32 arrays at 16 kHz, resampled on the GPU
    by band-limited sinc interpolation as torchaudio.functional.resample(x, sampling_rate, 16000) defines it.  What every
    audio entry does with sampling_rate= / int16 input before anything else."""
    _is_16k_f32(audios, sampling_rate)
    out, n = _resample(model, audios, sampling_rate, False)
    return [out[b, :n[b]].copy() for b in range(len(n))]


def _at_16k(model, audios, sampling_rate):
    return audios if _is_16k_f32(audios, sampling_rate) else resample(model, audios, sampling_rate)


def log_mel(model, audios: Sequence[np.ndarray], sampling_rate: int = SAMPLING_RATE) -> np.ndarray:
    """audios: list of 1-D float arrays at 16 kHz (any lengths; padded / trimmed to 30 s like WhisperProcessor) ->
    [B, n_mels, 2*n_audio_ctx] float32.  sampling_rate / np.int16 rows: resampled on the GPU first (resample)."""
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    cfg = model.config
    out = np.empty((len(audios), cfg.n_mels, cfg.n_frames), np.float32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(_lib.lib().wm_log_mel(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride, out.ctypes.data_as(fp)))
    return out


def transcribe_audio(model, audios: Sequence[np.ndarray], prompt: Sequence[int] = PROMPT, eot: int = EOT,
                     max_loop: int = MAX_LOOP, ignore_eot: bool = False, return_token_timestamps: bool = False,
                     repetition_penalty=None, no_repeat_ngram_size=None, sampling_rate: int = SAMPLING_RATE, sequence_bias=None,
                     bad_words_ids=None, return_logprobs: bool = False, top_k=None, constraint=None, free_from=None):
    """PCM in, token ids out (the mel never leaves the GPU).  return_logprobs / top_k / constraint / free_from: as
    Whisper.transcribe_batch, whose result this then is (constraint_match last); the log-mel of such a call is made on the
    GPU by log_mel and handed to transcribe_batch from host memory.  sampling_rate / np.int16 rows: resampled on the GPU first (resample).  return_token_timestamps: (ids, times) with the time in seconds
    each id was spoken (needs model.set_alignment_heads); the attention columns are cropped to each clip's real audio.
    repetition_penalty / no_repeat_ngram_size: as Whisper.transcribe_batch."""
    k = _lib.top_k_arg(top_k, return_logprobs)
    _lib.constraint_args(constraint, free_from, model.config.vocab_size, eot)  # (refused before any GPU work)
    if return_logprobs or constraint is not None:
        return model.transcribe_batch(log_mel(model, audios, sampling_rate), prompt, eot, max_loop, ignore_eot,
                                      return_token_timestamps=return_token_timestamps, return_logprobs=return_logprobs,
                                      repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                      sequence_bias=sequence_bias, bad_words_ids=bad_words_ids, top_k=k or None, constraint=constraint,
                                      free_from=free_from)
    model._set_repeat(_lib.repeat_args(repetition_penalty, no_repeat_ngram_size),
                      _lib.seq_bias_args(sequence_bias, bad_words_ids, model.config.vocab_size))  # (as Whisper.transcribe_batch)
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    p = np.asarray(prompt, np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    opts = _lib.WmDecodeOpts(p.ctypes.data_as(ip), len(p), eot, max_loop, model.pos_mode, int(ignore_eot), None, 0, None, 0)
    total = len(p) + 1 + max_loop
    toks = np.zeros((len(audios), total), np.int32)
    cnt = np.zeros(len(audios), np.int32)
    if return_token_timestamps:
        times = np.zeros((len(audios), total), np.float32)
        _lib.check(_lib.lib().wm_transcribe_pcm_tt(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                                   C.byref(opts), toks.ctypes.data_as(ip), cnt.ctypes.data_as(ip), times.ctypes.data_as(fp)))
        return ([toks[b, :cnt[b]].tolist() for b in range(len(audios))], [times[b, :cnt[b]].tolist() for b in range(len(audios))])
    _lib.check(_lib.lib().wm_transcribe_pcm(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                            C.byref(opts), toks.ctypes.data_as(ip), cnt.ctypes.data_as(ip)))
    return [toks[b, :cnt[b]].tolist() for b in range(len(audios))]


def score_audio(model, audios: Sequence[np.ndarray], ids, context_len=None, return_top_ids: bool = False,
                sampling_rate: int = SAMPLING_RATE):
    """PCM in, Whisper.score out (wm_score_pcm: the mel never leaves the GPU).  Arguments and result as Whisper.score.
    sampling_rate / np.int16 rows: resampled on the GPU first (resample)."""
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    B = len(audios)
    tab, lens, ctx = _lib.score_args(ids, context_len, B, model.config.vocab_size, model.config.n_text_ctx, model.max_batch)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lps, top = np.zeros(tab.shape, np.float32), np.full(tab.shape, -1, np.int32)
    sm, avg = np.zeros(B, np.float32), np.zeros(B, np.float32)
    _lib.check(_lib.lib().wm_score_pcm(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), B, stride, model.pos_mode,
                                       tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), tab.shape[1], ctx.ctypes.data_as(ip),
                                       lps.ctypes.data_as(fp), top.ctypes.data_as(ip) if return_top_ids else None,
                                       sm.ctypes.data_as(fp), avg.ctypes.data_as(fp)))
    return model._score_out(tab, lens, lps, top, sm, avg, return_top_ids)


def score_audio_candidates(model, audios: Sequence[np.ndarray], candidates, context_len=None, normalize: bool = False,
                           return_top_ids: bool = False, sampling_rate: int = SAMPLING_RATE):
    """PCM in, Whisper.score_candidates out (wm_score_nbest_pcm: the mel never leaves the GPU).  Arguments and result as
    Whisper.score_candidates.  sampling_rate / np.int16 rows: resampled on the GPU first (resample)."""
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    U = len(audios)
    args = _lib.nbest_args(candidates, context_len, U, model.config.vocab_size, model.config.n_text_ctx, model.max_batch)
    tab, lens, ctx, n_cand = args[:4]
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    bufs = model._nbest_bufs(tab, U)
    lps, top, sm, avg, order, best, post = bufs
    _lib.check(_lib.lib().wm_score_nbest_pcm(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), U, stride, n_cand.ctypes.data_as(ip),
                                             int(bool(normalize)), model.pos_mode, tab.ctypes.data_as(ip), lens.ctypes.data_as(ip),
                                             tab.shape[1], ctx.ctypes.data_as(ip), lps.ctypes.data_as(fp),
                                             top.ctypes.data_as(ip) if return_top_ids else None, sm.ctypes.data_as(fp),
                                             avg.ctypes.data_as(fp), order.ctypes.data_as(ip), best.ctypes.data_as(ip),
                                             post.ctypes.data_as(fp)))
    return model._nbest_out(args, bufs, return_top_ids)


def align_audio(model, audios: Sequence[np.ndarray], ids, context_len=None, return_logprobs: bool = False,
                sampling_rate: int = SAMPLING_RATE):
    """PCM in, Whisper.align out (wm_align_pcm: the mel never leaves the GPU; n_frames from the clip lengths, as
    transcribe_audio(return_token_timestamps=True)).  Arguments and result as Whisper.align.
    sampling_rate / np.int16 rows: resampled on the GPU first (resample); the frame counts are those of the 16 kHz samples."""
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    B = len(audios)
    tab, lens, ctx, _ = _lib.align_args(ids, context_len, None, B, model.config.vocab_size, model.config.n_text_ctx, model.max_batch,
                                        model.config.n_audio_ctx)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    times = np.zeros(tab.shape, np.float32)
    lp = (np.zeros(tab.shape, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)) if return_logprobs else None
    _lib.check(_lib.lib().wm_align_pcm(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), B, stride, model.pos_mode,
                                       tab.ctypes.data_as(ip), lens.ctypes.data_as(ip), tab.shape[1], ctx.ctypes.data_as(ip),
                                       times.ctypes.data_as(fp), *([a.ctypes.data_as(fp) for a in lp] if lp else [None] * 3)))
    return model._align_out(0, tab, lens, ctx, times, lp)


def log_mel_long(model, audios: Sequence[np.ndarray], sampling_rate: int = SAMPLING_RATE):
    """Log-mel of audio of any length, HF WhisperFeatureExtractor(truncation=False, padding="longest",
    return_attention_mask=True): (features [B, n_mels, longest // 160] float32, n_frames [B] = the mask's ones).
    sampling_rate / np.int16 rows: resampled on the GPU first (resample); longest counts 16 kHz samples."""
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    stride = max(stride, 201)
    if buf.shape[1] < stride:
        buf = np.pad(buf, ((0, 0), (0, stride - buf.shape[1])))
    out = np.empty((len(audios), model.config.n_mels, stride // HOP), np.float32)
    nf = np.zeros(len(audios), np.int32)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _lib.check(_lib.lib().wm_log_mel_long(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                          out.ctypes.data_as(fp), nf.ctypes.data_as(ip)))
    return out, nf


def transcribe_audio_long_form(model, audios: Sequence[np.ndarray], prompt: Sequence[int] = PROMPT, eot: int = EOT,
                               max_loop: int = MAX_LOOP, suppress_tokens: Sequence[int] = (), begin_suppress_tokens: Sequence[int] = (),
                               timestamps=(50364, 50363, 50), return_stats: bool = False, prompt_ids=None,
                               condition_on_prev_tokens: bool = False, prompt_condition_type: str = "first-segment",
                               prev_sot_token: int = 50361, logprob_threshold=None, no_speech_threshold=None, no_speech_token=None,
                               detect_language=None, return_token_timestamps: bool = False, repetition_penalty=None,
                               no_repeat_ngram_size=None, sampling_rate: int = SAMPLING_RATE, sequence_bias=None, bad_words_ids=None,
                               top_k=None, constraint=None, free_from=None):
    """top_k, constraint / free_from: refused here (ValueError), as in Whisper.transcribe_long_form.
    Sequential long-form transcription of 16 kHz PCM of any length (HF generate's long-form path), the long
    log-mel never leaving the GPU.  sampling_rate / np.int16 rows: resampled on the GPU first (resample; the 16 kHz samples pass
    through host memory); all times are seconds of audio.  repetition_penalty / no_repeat_ngram_size: as Whisper.transcribe_long_form.
    return_token_timestamps: as Whisper.transcribe_long_form ("token_times" per recording, "token_timestamps" per segment; not with
    the thresholds).  prompt_ids / condition_on_prev_tokens / prompt_condition_type / logprob_threshold /
    no_speech_threshold / no_speech_token / detect_language (then the detected ids [B] are returned as the last element): as
    Whisper.transcribe_long_form.  Returns per recording {"sequence": ids, "segments": [{"start", "end", "tokens"}]}."""
    if top_k is not None:
        raise ValueError("top_k is not available in long-form transcription (use transcribe_batch on 30 s windows)")
    if constraint is not None or free_from is not None:
        raise ValueError("constraint is not available in long-form transcription (use transcribe_batch on 30 s windows)")
    rp = _lib.repeat_args(repetition_penalty, no_repeat_ngram_size)
    sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, model.config.vocab_size)  # (as Whisper.transcribe_batch)
    lo, _keep2 = _lib.long_opts(prompt_ids, condition_on_prev_tokens, prompt_condition_type, prev_sot_token, logprob_threshold,
                                no_speech_threshold, no_speech_token)
    if no_speech_token is not None and int(no_speech_token) >= model.config.vocab_size:
        raise ValueError(f"no_speech_token {no_speech_token} is not a vocabulary id")
    if timestamps is None:
        raise ValueError("long-form transcription needs the timestamp rules")
    tt = _lib.long_tt_args(return_token_timestamps, logprob_threshold, no_speech_threshold)
    lang_list = None
    if detect_language is not None:
        lang_list = _lib.lang_args(detect_language, model.config.vocab_size)
        if len(prompt) < 2:
            raise ValueError("detect_language needs at least two initial ids (<|startoftranscript|> and the language slot)")
    audios = _at_16k(model, audios, sampling_rate)
    buf, n, stride = _pack(audios)
    stride = max(stride, 201)
    if buf.shape[1] < stride:
        buf = np.pad(buf, ((0, 0), (0, stride - buf.shape[1])))
    opts, _keep = model._opts(prompt, eot, max_loop, False, suppress_tokens, begin_suppress_tokens, timestamps)
    model._set_repeat(rp, sb)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    h = C.c_void_p()
    if tt:
        lang = np.zeros(len(audios), np.int32)
        _lib.check(_lib.lib().wm_transcribe_long_pcm_tt(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                                        C.byref(opts), C.byref(lo),
                                                        lang_list.ctypes.data_as(ip) if lang_list is not None else None,
                                                        lang_list.size if lang_list is not None else 0, lang.ctypes.data_as(ip), 1,
                                                        C.byref(h)))
        out, stats = _lib.long_result(h, len(audios), False, True)
        res = (out, stats) if return_stats else (out,)
        res = res + (lang,) if lang_list is not None else res
        return res if len(res) > 1 else out
    if lang_list is not None:
        lang = np.zeros(len(audios), np.int32)
        _lib.check(_lib.lib().wm_transcribe_long_pcm_lang(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                                          C.byref(opts), C.byref(lo), lang_list.ctypes.data_as(ip), lang_list.size,
                                                          lang.ctypes.data_as(ip), C.byref(h)))
        out, stats = _lib.long_result(h, len(audios), logprob_threshold is not None or no_speech_threshold is not None)
        return (out, stats, lang) if return_stats else (out, lang)
    _lib.check(_lib.lib().wm_transcribe_long_pcm_ex(model._h, buf.ctypes.data_as(fp), n.ctypes.data_as(ip), len(audios), stride,
                                                    C.byref(opts), C.byref(lo), C.byref(h)))
    out, stats = _lib.long_result(h, len(audios), logprob_threshold is not None or no_speech_threshold is not None)
    return (out, stats) if return_stats else out


def transcribe_audio_chunked(model, audios, chunk_length_s: float = 30.0, stride_length_s=None, return_chunks: bool = False,
                             prompt: Sequence[int] = PROMPT, eot: int = EOT, max_loop: int = MAX_LOOP, suppress_tokens: Sequence[int] = (),
                             begin_suppress_tokens: Sequence[int] = (), timestamps=None, detect_language=None, repetition_penalty=None,
                             no_repeat_ngram_size=None, first_special: int = _lib.FIRST_SPECIAL, return_stats: bool = False, n_samples=None,
                             return_timestamps=False, time_precision=None, tokenizer=None, sampling_rate: int = SAMPLING_RATE,
                             sequence_bias=None, bad_words_ids=None, top_k=None, constraint=None, free_from=None):
    """constraint / free_from: refused here (ValueError) — the chunk scheduler does not carry Whisper.transcribe_batch's phrase-list
    constraint yet.
    top_k: refused here (ValueError) — the top-k alternatives of Whisper.transcribe_batch have no place in the stitched
    result yet.
    Chunked long-form transcription of 16 kHz PCM of any length (HF's ASR pipeline with chunk_length_s / stride_length_s /
    batch_size = max_batch): every recording is cut into overlapping chunks (HF chunk_iter), the chunks of all recordings
    are decoded on their own in passes of up to max_batch rows, two passes in flight, and each recording's id lists are stitched on
    the GPU (HF _find_longest_common_sequence after the strip of every id >= first_special).  One recording fills whole batches,
    which transcribe_audio_long_form's sequential algorithm cannot.
    audios: one 1-D float array or a list of them, or PCM that already is on the model's GPU: a torch float32 CUDA tensor [R, stride]
    (or [stride]) with n_samples, the valid samples per row (None: the whole row) — it is not copied.  stride_length_s: None (chunk_length_s / 6), seconds, or (left, right).
    prompt / eot / max_loop / suppress_tokens / begin_suppress_tokens / timestamps / detect_language / repetition_penalty /
    no_repeat_ngram_size: as Whisper.transcribe_batch, applied to every chunk (HF's generate_kwargs); with detect_language the
    detected id sits in each chunk's ids.  The no-timestamps prompt is the caller's choice; timestamp ids a chunk does emit are dropped
    with the other specials.
    Returns per recording {"sequence": merged ids} and, with return_chunks, "chunks": [(start_s, len_s, stride_left_s,
    stride_right_s, ids)] with the ids exactly as transcribe_audio gives them for that chunk's samples alone.  A single array in, a
    single dict out.  return_stats: also {"chunks", "passes"}.  tokenizer.decode_text(sequence) gives the text.
    return_timestamps (needs timestamps=, the timestamp rule, and a prompt without the no-timestamps id): True — HF's
    return_timestamps=True: every recording also carries "segments": [{"timestamp": (start_s, end_s | None), "ids": [...]}], cut at
    the timestamp ids as _decode_asr cuts them (those inside a stride are skipped), each segment's ids merged over the chunks it
    spans; "sequence" is then the segments' ids concatenated.  "word" — HF's return_timestamps="word" (needs set_alignment_heads; not
    with detect_language): every pass also computes token times with n_frames = chunk samples // 160, every segment carries
    "token_timestamps": [(start_s, end_s)] per id, the merge counts a position only when the left pair <= the right pair, and with
    tokenizer= also "words" (tokenizer.collate_words); with return_chunks every chunk tuple ends with its token times.  "word" needs
    two mel frames of audio in every chunk: a chunk shorter than 320 samples (the tail of a recording under stride_length_s=0, or a
    recording shorter than 20 ms) makes the library refuse the whole call, where the other two modes accept it.
    time_precision: seconds per timestamp id (None: window seconds / n_audio_ctx).
    sampling_rate / np.int16 host arrays: the raw samples go up once, are resampled to 16 kHz on the GPU and stay there
    (the device-PCM path below); chunk_length_s, stride_length_s and every returned time are seconds of audio.  Device PCM is 16 kHz
    float32 already."""
    if top_k is not None:
        raise ValueError("top_k is not available in chunked transcription (use transcribe_batch on the chunks)")
    if constraint is not None or free_from is not None:
        raise ValueError("constraint is not available in chunked transcription (use transcribe_batch on the chunks)")
    if not isinstance(return_timestamps, (bool, np.bool_)) and not (isinstance(return_timestamps, str) and return_timestamps == "word"):
        raise ValueError('return_timestamps is False, True or "word"')  # 0 / 1 would pass an `in` test by equality: bools only
    ts_mode = 2 if isinstance(return_timestamps, str) else 1 if return_timestamps else 0
    if ts_mode and timestamps is None:
        raise ValueError("return_timestamps needs timestamps=(timestamp_begin, no_timestamps_id, max_initial_timestamp_index)")
    if ts_mode == 2 and detect_language is not None:
        raise ValueError('return_timestamps="word" does not combine with detect_language')
    dev, was_single = None, None
    if not isinstance(audios, (np.ndarray, list, tuple)):
        import torch
        if isinstance(audios, torch.Tensor) and audios.is_cuda:
            dev = audios
    if dev is not None and int(sampling_rate) != SAMPLING_RATE:
        raise ValueError("device PCM is 16 kHz float32; sampling_rate goes with host arrays")
    if dev is None:
        if n_samples is not None:
            raise ValueError("n_samples goes with device PCM; host arrays carry their own lengths")
        single = isinstance(audios, np.ndarray) and audios.ndim == 1
        if single:
            audios = [audios]
        if not len(audios):
            raise ValueError("no recording")
        if not _is_16k_f32(audios, sampling_rate):
            dev, n_samples = _resample(model, audios, sampling_rate, True)
            was_single = single
    if dev is not None:
        single = dev.dim() == 1
        dev = (dev[None] if single else dev).contiguous().float()
        if dev.dim() != 2 or dev.shape[0] < 1 or dev.shape[1] < 1:
            raise ValueError("device PCM must be [R, stride] or [stride]")
        n = np.full(dev.shape[0], dev.shape[1], np.int64) if n_samples is None else np.asarray(n_samples, np.int64).reshape(-1)
        if n.size != dev.shape[0] or n.min() < 0 or n.max() > dev.shape[1]:
            raise ValueError(f"n_samples needs one length in [0, {dev.shape[1]}] per row ({dev.shape[0]})")
        n, stride, n_rec = n.astype(np.int32), int(dev.shape[1]), int(dev.shape[0])
        import torch
        torch.cuda.current_stream(dev.device).synchronize()  # the library reads it on its own HIP stream
        pcm_ptr, on_dev = C.c_void_p(dev.data_ptr()), 1
        single = was_single if was_single is not None else single
    else:
        audios = [np.asarray(a, np.float32).reshape(-1) for a in audios]
        buf, n, stride = _pack(audios)
        n_rec = len(audios)
        pcm_ptr, on_dev = buf.ctypes.data_as(C.c_void_p), 0
    rp = _lib.repeat_args(repetition_penalty, no_repeat_ngram_size)
    sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, model.config.vocab_size)  # (as Whisper.transcribe_batch)
    lang_list = None
    if detect_language is not None:
        lang_list = _lib.lang_args(detect_language, model.config.vocab_size)
        if len(prompt) < 2:
            raise ValueError("detect_language needs at least two initial ids (<|startoftranscript|> and the language slot)")
    if not 0 < int(first_special) <= model.config.vocab_size:
        raise ValueError(f"first_special must lie in (0, vocab = {model.config.vocab_size}]")
    chunk_len, sl, sr = _lib.chunk_strides(chunk_length_s, stride_length_s, SAMPLING_RATE)
    tab = _lib.chunk_table(n, chunk_len, sl, sr, window=model.config.n_frames * HOP)
    if model._h is None:
        raise _lib.WhisperMiError("model not loaded")
    opts, _keep = model._opts(prompt, eot, max_loop, False, suppress_tokens, begin_suppress_tokens, timestamps)
    model._set_repeat(rp, sb)
    R, total = n_rec, len(prompt) + 1 + max_loop
    per_rec = np.bincount(tab[:, 0], minlength=R) if len(tab) else np.zeros(R, np.int64)
    cap = max(1, int(per_rec.max()) * total)
    merged, mlen = np.zeros((R, cap), np.int32), np.zeros(R, np.int32)
    cids = np.zeros((max(1, len(tab)), total), np.int32) if return_chunks else None
    cn = np.zeros(max(1, len(tab)), np.int32) if return_chunks else None
    passes = C.c_int32()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    lang_ptr = lang_list.ctypes.data_as(ip) if lang_list is not None else None
    n_lang = lang_list.size if lang_list is not None else 0
    ctimes = None
    if not ts_mode:
        _lib.check(_lib.lib().wm_transcribe_chunked(
            model._h, pcm_ptr, on_dev, n.ctypes.data_as(ip), R, stride, chunk_len, sl, sr, C.byref(opts), lang_ptr, n_lang, int(first_special),
            merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), cap, cids.ctypes.data_as(ip) if return_chunks else None,
            cn.ctypes.data_as(ip) if return_chunks else None, C.byref(passes)))
        out = [{"sequence": merged[r, :mlen[r]].tolist()} for r in range(R)]
    else:
        dp = C.POINTER(C.c_double)
        seg_cap = cap + 1  # a segment closes at a timestamp id, and one more may stay open
        nseg, segt, segr = np.zeros(R, np.int32), np.zeros((R, seg_cap, 2), np.float64), np.zeros((R, seg_cap, 2), np.int32)
        pairs = np.zeros((R, cap, 2), np.float64) if ts_mode == 2 else None
        ctimes = np.zeros((max(1, len(tab)), total), np.float32) if return_chunks and ts_mode == 2 else None
        _lib.check(_lib.lib().wm_transcribe_chunked_ts(
            model._h, pcm_ptr, on_dev, n.ctypes.data_as(ip), R, stride, chunk_len, sl, sr, C.byref(opts), lang_ptr, n_lang, int(first_special),
            ts_mode, 0.0 if time_precision is None else float(time_precision), merged.ctypes.data_as(ip), mlen.ctypes.data_as(ip), cap,
            nseg.ctypes.data_as(ip), segt.ctypes.data_as(dp), segr.ctypes.data_as(ip), seg_cap, pairs.ctypes.data_as(dp) if pairs is not None else None,
            cids.ctypes.data_as(ip) if return_chunks else None, cn.ctypes.data_as(ip) if return_chunks else None,
            ctimes.ctypes.data_as(fp) if ctimes is not None else None, C.byref(passes)))
        out = []
        for r in range(R):
            ids = merged[r, :mlen[r]].tolist()
            segs = []
            for k in range(nseg[r]):
                (s, e), (b0, b1) = segt[r, k].tolist(), segr[r, k].tolist()
                seg = {"timestamp": (None if s != s else s, None if e != e else e), "ids": ids[b0:b1]}
                if pairs is not None:
                    seg["token_timestamps"] = [tuple(p) for p in pairs[r, b0:b1].tolist()]
                    if tokenizer is not None:
                        from .tokenizer import collate_words
                        seg["words"] = collate_words(tokenizer, seg["ids"], seg["token_timestamps"])
                segs.append(seg)
            out.append({"sequence": ids, "segments": segs})
    if return_chunks:
        for r in range(R):
            out[r]["chunks"] = []
        for k, (r, start, ln, esl, esr, _last) in enumerate(tab.tolist()):
            row = (start / SAMPLING_RATE, ln / SAMPLING_RATE, esl / SAMPLING_RATE, esr / SAMPLING_RATE, cids[k, :cn[k]].tolist())
            out[r]["chunks"].append(row + (ctimes[k, :cn[k]].tolist(),) if ctimes is not None else row)
    res = out[0] if single else out
    return (res, {"chunks": int(len(tab)), "passes": int(passes.value)}) if return_stats else res


# ---- decoding features the reference lacks, host-level over the same C-ABI -----------------------
HOP = 160  # samples per mel frame (WhisperFeatureExtractor hop_length)


def transcribe_long(model, audio: np.ndarray, prompt: Sequence[int] = PROMPT, eot: int = EOT, max_loop: int = MAX_LOOP,
                    suppress_tokens: Sequence[int] = (), begin_suppress_tokens: Sequence[int] = ()):
    """Long-form audio by consecutive 30 s windows (the reference handles one 30 s clip, main.mojo:22-27): the windows
    are independent utterances, so they go through the batch path `max_batch` at a time.  Returns (per-window id lists
    exactly as `transcribe` would give them, generated ids of all windows concatenated without prompt / eot)."""
    audio = np.asarray(audio, np.float32).ravel()
    win = model.config.n_frames * HOP  # 480 000 samples = 30 s for the released models
    n_win = max(1, -(-len(audio) // win))
    windows = [audio[i * win:(i + 1) * win] for i in range(n_win)]
    per_window: List[List[int]] = []
    for i in range(0, n_win, model.max_batch):
        group = windows[i:i + model.max_batch]
        mels = log_mel(model, group)
        per_window += model.transcribe_batch(mels, prompt=prompt, eot=eot, max_loop=max_loop,
                                             suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens)
    flat: List[int] = []
    for ids in per_window:
        gen = ids[len(prompt):]
        flat += gen[:-1] if gen and gen[-1] == eot else gen
    return per_window, flat


def detect_language(model, mel, sot: int = 50258, lang_first: int = 50259, lang_last: int = 50357):
    """Whisper's language identification: one decoder step on <|startoftranscript|> and a softmax restricted to the
    language ids (multilingual vocabulary: 50259..50357).  mel: [n_mels, 3000] or [B, n_mels, 3000].
    Returns (ids [B], probabilities [B, n_lang])."""
    from .whisper import KVCache
    m = np.asarray(mel, np.float32)
    batched = m.ndim == 3
    m = m if batched else m[None]
    B = m.shape[0]
    cache = KVCache(model, B)
    model.encoder.forward(m, cache)
    logits = model.decoder.forward(np.full((B, 1), sot, np.int32), None, cache, start_pos=0)
    lang = np.asarray(logits, np.float64).reshape(B, -1)[:, lang_first:lang_last + 1]
    p = np.exp(lang - lang.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    ids = lang_first + p.argmax(1)
    return (ids, p) if batched else (int(ids[0]), p[0])
