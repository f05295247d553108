"""Host-side mirror of /root/reference/whisper.mojo + layers.mojo's KVCache: same names, argument meaning and
error behaviour, every forward a call through the C-ABI (include/whisper_mi.h) into the HIP path.

    whisper = Whisper()                                  # whisper.mojo:175-178
    whisper.load(WeightLoader("whisper_tiny_weights.bin"))   # main.mojo:16-17
    tokens = whisper.transcribe(mel)                     # main.mojo:30, mel = [80, 3000] fp32

Extensions the reference lacks: a leading batch dimension (transcribe_batch), device-resident mels (torch CUDA
tensors), 16-bit operand / KV-cache dtypes, Whisper-base dims."""
from __future__ import annotations

import ctypes as C
import weakref
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from .config import (DT_F32, EOT, GELU_TANH, MAX_LOOP, POS_REF, PROMPT, WhisperConfig)
from .loader import WeightLoader


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _mel_arg(mel, cfg: WhisperConfig):
    """-> (pointer, on_device, B, keepalive).  Accepts numpy [B,n_mels,T] / [n_mels,T] or a torch CUDA tensor."""
    shape_tail = (cfg.n_mels, cfg.n_frames)
    if isinstance(mel, np.ndarray):
        a = np.ascontiguousarray(mel, np.float32)
        if a.ndim == 2:
            a = a[None]
        if a.shape[1:] != shape_tail:
            raise ValueError(f"mel must be [B, {cfg.n_mels}, {cfg.n_frames}], got {a.shape}")
        return a.ctypes.data_as(C.c_void_p), 0, a.shape[0], a
    import torch
    if not isinstance(mel, torch.Tensor):
        raise TypeError("mel must be a numpy array or a torch tensor")
    t = mel if mel.dim() == 3 else mel[None]
    if tuple(t.shape[1:]) != shape_tail:
        raise ValueError(f"mel must be [B, {cfg.n_mels}, {cfg.n_frames}], got {tuple(t.shape)}")
    if not t.is_cuda:
        return _mel_arg(t.numpy(), cfg)
    t = t.contiguous().float()
    torch.cuda.current_stream(t.device).synchronize()  # the library runs on its own HIP stream
    return C.c_void_p(t.data_ptr()), 1, t.shape[0], t


class KVCache:
    """layers.mojo:55-69 — KVCache(n_layers, d_model, max_len) for a batch of utterances; owns the device-side
    self/cross K/V arena (wm_state)."""

    def __init__(self, model: "Whisper", batch: int = 1):
        self.model = model
        self.batch = batch
        h = C.c_void_p()
        _lib.check(_lib.lib().wm_state_new(model._h, batch, C.byref(h)))
        self._h = h
        # the model owns the device arenas of its caches (wm_model_free frees them): remember WHICH loaded model this is, so
        # a cache that outlives a reload / close() neither frees nor uses memory that went away with the old model
        self._model_h = model._h.value
        model._caches.add(self)

    @property
    def current_len(self) -> int:
        """LayerCache.current_len (layers.mojo:18) — same for every layer."""
        return _lib.lib().wm_state_len(self._h)

    def reset(self):
        _lib.check(_lib.lib().wm_state_reset(self._h))

    def _invalidate(self):
        """Whisper.close() / load(): the library freed this cache's state together with its model."""
        self._h = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        mh = getattr(getattr(self, "model", None), "_h", None)
        if h and mh is not None and mh.value == getattr(self, "_model_h", None):
            _lib.lib().wm_state_free(h)


class WhisperEncoder:
    """whisper.mojo:34-99"""

    def __init__(self, model: "Whisper"):
        self._m = model

    def forward(self, mel, cache: Optional[KVCache] = None) -> np.ndarray:
        """whisper.mojo:71-99: mel [n_mels, 3000] -> [1500, d_model]  (or batched [B,...]).  When `cache` is given
        the encoder output also stays on the device inside it for WhisperDecoder.forward."""
        m = self._m
        ptr, on_dev, B, keep = _mel_arg(mel, m.config)
        cache = cache or KVCache(m, B)
        out = np.empty((B, m.config.n_audio_ctx, m.config.d_model), np.float32)
        _lib.check(_lib.lib().wm_encode(m._h, cache._h, ptr, on_dev, B, _fp(out)))
        single = (isinstance(mel, np.ndarray) and mel.ndim == 2) or (not isinstance(mel, np.ndarray) and mel.dim() == 2)
        return out[0] if single else out


class WhisperDecoder:
    """whisper.mojo:102-167"""

    def __init__(self, model: "Whisper"):
        self._m = model

    def forward(self, tokens, enc_out, cache: KVCache, use_cache: bool = True, start_pos=0) -> np.ndarray:
        """whisper.mojo:130-167.  tokens: List[int] (one utterance) or [B, q_len]; enc_out: the encoder output
        ([1500,d] / [B,1500,d]) — uploaded and projected to cross K/V on the cache's first use
        (layers.mojo:150-154) — or None when `cache` already holds one from WhisperEncoder.forward(mel, cache).
        Returns logits [vocab] / [B, vocab] for the last position."""
        if not use_cache:
            raise NotImplementedError("the decode path always runs KV-cached, as Whisper.transcribe does (whisper.mojo:195,212)")
        m = self._m
        t = np.asarray(tokens, np.int32)
        single = t.ndim == 1
        t = np.ascontiguousarray(t.reshape(1, -1) if single else t)
        B, q_len = t.shape
        if B != cache.batch:
            raise ValueError(f"cache was created for batch {cache.batch}, tokens have batch {B}")
        if enc_out is not None and cache.current_len == 0:
            e = np.ascontiguousarray(enc_out, np.float32).reshape(B, m.config.n_audio_ctx, m.config.d_model)
            _lib.check(_lib.lib().wm_state_set_encoder_output(m._h, cache._h, _fp(e), B))
        sp = np.ascontiguousarray(np.broadcast_to(np.asarray(start_pos, np.int32), (B,)))
        logits = np.empty((B, m.config.vocab_size), np.float32)
        _lib.check(_lib.lib().wm_decode_step(m._h, cache._h, _ip(t), q_len, _ip(sp), _fp(logits), None))
        return logits[0] if single else logits


class Whisper:
    """whisper.mojo:169-223"""

    def __init__(self, config: Optional[WhisperConfig] = None, compute_dtype: int = DT_F32, kv_dtype: Optional[int] = None,
                 gelu_mode: int = GELU_TANH, pos_mode: int = POS_REF, max_batch: int = 64, device: int = 0,
                 decoder_fp32: bool = False, coalesce: int = 0):
        self.config = config or WhisperConfig.tiny()
        self.compute_dtype = compute_dtype
        self.kv_dtype = compute_dtype if kv_dtype is None else kv_dtype
        self.gelu_mode = gelu_mode
        self.pos_mode = pos_mode
        self.max_batch = max_batch
        self.device = device
        self.decoder_fp32 = decoder_fp32  # compute_dtype narrows the encoder only; decoder weights / operands stay fp32
        self.coalesce = coalesce  # 2: consecutive transcribe_submit calls of equal batch size / options share one 2·B-row decode state
        self._h = None
        self._caches = weakref.WeakSet()  # live KVCaches of the loaded model
        self._n_align = 0  # alignment heads set on the loaded model (set_alignment_heads)
        self._sb_key = None  # the lists of the sequence-bias table set on the loaded model (_set_repeat); None = no table
        self._ct_key = None  # the phrases of the constraint table set on the loaded model, likewise
        self._nbest_pending = {}  # slot -> (arguments, mel keep-alive) of a submitted n-best score pass (score_candidates_submit / _wait)
        self._score_pending = {}  # slot -> (id table, lengths, mel keep-alive) of a submitted score pass (score_submit / score_wait)
        self._align_pending = {}  # slot -> (id table, lengths, context lengths, logprobs asked, keep-alives) of a submitted align pass
        self.encoder = WhisperEncoder(self)
        self.decoder = WhisperDecoder(self)

    def _cfg(self) -> _lib.WmConfig:
        return _lib.WmConfig(self.config.dims(), self.gelu_mode, self.compute_dtype, self.kv_dtype, self.max_batch,
                             int(self.decoder_fp32), int(self.coalesce))

    def load(self, loader: WeightLoader):
        """whisper.mojo:180-182.  Raises if the image size does not match the config."""
        self.close()
        h = C.c_void_p()
        cfg = self._cfg()
        w = loader.raw_data
        _lib.check(_lib.lib().wm_model_load_memory(_fp(w), w.size, C.byref(cfg), self.device, C.byref(h)))
        self._h = h
        self._n_align = 0
        self._sb_key = None  # a freshly loaded model has no sequence-bias table
        self._ct_key = None  # ... and no constraint table

    def load_file(self, path: str):
        self.close()
        h = C.c_void_p()
        cfg = self._cfg()
        _lib.check(_lib.lib().wm_model_load(path.encode(), C.byref(cfg), self.device, C.byref(h)))
        self._h = h
        self._n_align = 0
        self._sb_key = None  # a freshly loaded model has no sequence-bias table
        self._ct_key = None  # ... and no constraint table

    def close(self):
        h, self._h = self._h, None
        self._sb_key = self._ct_key = None
        if h:
            for c in list(self._caches):
                c._invalidate()
            self._caches.clear()
            self._pending = {}
            self._score_pending = {}
            self._nbest_pending = {}
            self._align_pending = {}
            _lib.lib().wm_model_free(h)  # also frees every state (KVCache arena, pipeline slot) created on it

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _opts(self, prompt, eot, max_loop, ignore_eot, suppress_tokens=(), begin_suppress_tokens=(), timestamps=None):
        """timestamps: None (the reference: raw argmax) or (timestamp_begin, no_timestamps_id, max_initial_timestamp_index | None)
        — HF's WhisperTimeStampLogitsProcessor inside the fused argmax."""
        p = np.asarray(prompt, np.int32)
        sup = np.asarray(list(suppress_tokens), np.int32)
        bsup = np.asarray(list(begin_suppress_tokens), np.int32)
        tb, no_ts, max_init = (0, -1, -1) if timestamps is None else (int(timestamps[0]), int(timestamps[1]),
                                                                      -1 if timestamps[2] is None else int(timestamps[2]))
        opts = _lib.WmDecodeOpts(_ip(p), len(p), eot, max_loop, self.pos_mode, int(ignore_eot),
                                 _ip(sup) if len(sup) else None, len(sup), _ip(bsup) if len(bsup) else None, len(bsup),
                                 tb, no_ts, max_init)
        return opts, (p, sup, bsup)

    def _set_repeat(self, rp, sb=None, top_k=0, ct=None):
        """wm_set_repeat_options with a call's (penalty, n), wm_set_sequence_bias with its lists (sb: _lib.seq_bias_args, None =
        off), wm_set_top_k with its k and wm_set_constraint with its phrases (ct: _lib.constraint_args, None = off): every greedy
        call sets them, so a call without the arguments runs with all of them off.  A table is rebuilt only when its lists differ
        from the last call's."""
        _lib.check(_lib.lib().wm_set_repeat_options(self._h, rp[0], rp[1]))
        _lib.check(_lib.lib().wm_set_top_k(self._h, top_k))
        key = None if sb is None else sb[0]
        if key != self._sb_key:
            ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
            a = [None, None, None, 0, None, None, 0] if sb is None else sb[1]
            q = lambda x, t: None if x is None else x.ctypes.data_as(t)
            _lib.check(_lib.lib().wm_set_sequence_bias(self._h, q(a[0], ip), q(a[1], ip), q(a[2], fp), a[3], q(a[4], ip), q(a[5], ip), a[6]))
            self._sb_key = key
        key = None if ct is None else ct[0]
        if key != self._ct_key:
            ip = C.POINTER(C.c_int32)
            if ct is None:
                _lib.check(_lib.lib().wm_set_constraint(self._h, None, None, 0, -1))
            else:
                ids, off, n, ff = ct[1]
                _lib.check(_lib.lib().wm_set_constraint(self._h, ids.ctypes.data_as(ip), off.ctypes.data_as(ip), n, ff))
            self._ct_key = key

    def _constraint_match(self, slot, B):
        """constraint_match of the constrained pass the slot collected last (wm_transcribe_constraint_match): int32 [B]"""
        out = np.zeros(B, np.int32)
        _lib.check(_lib.lib().wm_transcribe_constraint_match(self._h, slot, _ip(out), B))
        return out

    @staticmethod
    def _with_last(res, last):
        """a call's result with one more, last element"""
        return res + (last,) if isinstance(res, tuple) else (res, last)

    def set_alignment_heads(self, pairs: Sequence[Sequence[int]]):
        """(layer, head) pairs whose cross-attention aligns ids with audio (HF generation_config.alignment_heads, e.g.
        config.ALIGNMENT_HEADS_TINY); needed by return_token_timestamps.  An empty list switches the feature off."""
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        flat = np.asarray([int(v) for pr in pairs for v in pr], np.int32)
        if flat.size != 2 * len(pairs):
            raise ValueError("alignment heads are (layer, head) pairs")
        _lib.check(_lib.lib().wm_set_alignment_heads(self._h, _ip(flat) if flat.size else None, len(pairs)))
        self._n_align = len(pairs)

    @staticmethod
    def _frames_arg(n_frames, B):
        if n_frames is None:
            return None
        nf = np.ascontiguousarray(np.asarray(n_frames, np.int32).reshape(-1))
        if nf.size != B:
            raise ValueError(f"n_frames needs one entry per utterance ({B}), got {nf.size}")
        return nf

    @staticmethod
    def _prompt_rows(prompts, B):
        """per-utterance prompts -> ([B, Lmax] int32 table, [B] lengths)"""
        rows = [np.asarray(r, np.int32).reshape(-1) for r in prompts]
        if len(rows) != B:
            raise ValueError(f"prompts needs one id list per utterance ({B}), got {len(rows)}")
        lens = np.asarray([r.size for r in rows], np.int32)
        tab = np.zeros((B, max(1, int(lens.max()))), np.int32)
        for b, r in enumerate(rows):
            tab[b, :r.size] = r
        return tab, lens

    def _ns_args(self, no_speech_token, n_init, prompt, prompts, return_logprobs):
        """-> None or (token, n_init), checked on the host (ValueError) before anything else"""
        if no_speech_token is None:
            if n_init is not None:
                raise ValueError("n_init without no_speech_token")
            return None
        if not return_logprobs:
            raise ValueError("no_speech_token needs return_logprobs=True")
        lens = len(prompt) if prompts is None else [len(r) for r in prompts]
        return _lib.no_speech_args(no_speech_token, n_init, lens, self.config.vocab_size)

    def _lang_args(self, detect_language, n_init, prompt, prompts, return_token_timestamps, no_speech_token, return_logprobs):
        """-> (int32 language list, n_init), checked on the host (ValueError) before anything else"""
        if return_token_timestamps:
            raise ValueError("detect_language does not combine with return_token_timestamps")
        ids = _lib.lang_args(detect_language, self.config.vocab_size)
        if n_init is None:
            if prompts is not None:
                raise ValueError("n_init is required with per-row prompts (the number of initial ids, <|startoftranscript|> first)")
            n_init = len(prompt)
        n_init = int(n_init)
        shortest = len(prompt) if prompts is None else min(len(r) for r in prompts)
        if n_init < 2 or n_init > shortest:
            raise ValueError(f"n_init {n_init} outside [2, shortest prompt = {shortest}]")
        if no_speech_token is not None:
            if not return_logprobs:
                raise ValueError("no_speech_token needs return_logprobs=True")
            if int(no_speech_token) < 0 or int(no_speech_token) >= self.config.vocab_size:
                raise ValueError(f"no_speech_token {no_speech_token} is not a vocabulary id")
        return ids, n_init

    def detect_language(self, mel, lang_ids: Sequence[int], sot: int = PROMPT[0]):
        """openai-whisper's detect_language / HF WhisperGenerationMixin.detect_language: the encoder, one decoder pass
        over [sot] and the language kernel -> (ids [B] int32: per utterance the id of lang_ids with the largest logit, probs
        [B, n_lang] float32: the softmax over lang_ids, in list order).  lang_ids: 1..128 distinct vocabulary ids, any order
        (tokenizer.language_ids)."""
        ids = _lib.lang_args(lang_ids, self.config.vocab_size)
        if int(sot) < 0 or int(sot) >= self.config.vocab_size:
            raise ValueError(f"sot {sot} is not a vocabulary id")
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        out = np.zeros(B, np.int32)
        probs = np.zeros((B, ids.size), np.float32)
        _lib.check(_lib.lib().wm_detect_language(self._h, ptr, on_dev, B, int(sot), _ip(ids), ids.size, _ip(out), _fp(probs)))
        return out, probs

    def _lang_call(self, slot, ptr, on_dev, B, opts, p, prompts, max_loop, lang, return_logprobs, no_speech_token):
        """submit (slot is not None) or run a _lang pass; -> what transcribe_wait needs / the result"""
        ids, n_init = lang
        tab, lens = self._prompt_rows(prompts, B) if prompts is not None else (None, None)
        rows = (_ip(tab) if tab is not None else None, _ip(lens) if tab is not None else None, tab.shape[1] if tab is not None else 0)
        total = (tab.shape[1] if tab is not None else len(p)) + 1 + max_loop
        ns_tok = -1 if no_speech_token is None else int(no_speech_token)
        if slot is not None:
            _lib.check(_lib.lib().wm_transcribe_submit_lang(self._h, slot, ptr, on_dev, B, C.byref(opts), *rows, ns_tok, n_init, _ip(ids),
                                                            ids.size, int(return_logprobs)))
            return total, ("lang", ids.size, bool(return_logprobs), ns_tok >= 0)
        return self._lang_collect(None, B, total, ids.size, return_logprobs, ns_tok >= 0,
                                  lambda *a: _lib.lib().wm_transcribe_lang(self._h, ptr, on_dev, B, C.byref(opts), *rows, ns_tok, n_init,
                                                                           _ip(ids), ids.size, *a))

    def _lang_collect(self, slot, B, total, n_lang, lp, ns, call):
        toks, n = np.zeros((B, total), np.int32), np.zeros(B, np.int32)
        lps, avg, nsp = np.zeros((B, total), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        lang_out, lang_probs = np.zeros(B, np.int32), np.zeros((B, n_lang), np.float32)
        _lib.check(call(_ip(toks), _ip(n), _fp(lps) if lp else None, _fp(avg) if lp else None, _fp(nsp) if ns else None, _ip(lang_out),
                        _fp(lang_probs)))
        self.last_tokens, self.last_counts = toks, n
        out = [toks[b, :n[b]].tolist() for b in range(B)]
        lang = (lang_out, lang_probs)
        if not lp:
            return out, lang
        self.last_logprobs = lps
        return out, (self._split_times(lps, n, B), avg, nsp) if ns else (self._split_times(lps, n, B), avg), lang

    @staticmethod
    def _split_times(times, n, B):
        return [times[b, :n[b]].tolist() for b in range(B)]

    def _top_k(self, slot, k, plens):
        """wm_transcribe_top_k of the log-prob pass just collected on `slot` -> (top_ids, top_logprobs): per utterance an int32 /
        float32 array [generated ids, k], the row's prompt (plens[b] ids) cut off."""
        B, total = self.last_tokens.shape
        n = self.last_counts
        ids, lps = np.zeros((B, total, k), np.int32), np.zeros((B, total, k), np.float32)
        _lib.check(_lib.lib().wm_transcribe_top_k(self._h, slot, _ip(ids), _fp(lps)))
        return ([ids[b, plens[b]:max(n[b], plens[b])].copy() for b in range(B)],
                [lps[b, plens[b]:max(n[b], plens[b])].copy() for b in range(B)])

    @staticmethod
    def _plens(prompt, prompts, B):
        return [len(prompt)] * B if prompts is None else [len(r) for r in prompts]

    def transcribe_batch(self, mel, prompt: Sequence[int] = PROMPT, eot: int = EOT, max_loop: int = MAX_LOOP,
                         ignore_eot: bool = False, suppress_tokens: Sequence[int] = (),
                         begin_suppress_tokens: Sequence[int] = (), timestamps=None, return_token_timestamps: bool = False,
                         n_frames=None, prompts: Optional[Sequence[Sequence[int]]] = None, return_logprobs: bool = False,
                         no_speech_token: Optional[int] = None, n_init: Optional[int] = None,
                         detect_language: Optional[Sequence[int]] = None, repetition_penalty: Optional[float] = None,
                         no_repeat_ngram_size: Optional[int] = None, sequence_bias=None, bad_words_ids=None, top_k: Optional[int] = None,
                         constraint=None, free_from: Optional[int] = None):
        """Batched Whisper.transcribe: one List[int] per utterance = prompt + generated ids (+ eot when hit).
        constraint: a list of phrases, each a non-empty list of ids — every row's generated ids, without the free ids,
        are confined to one of the phrases followed by eot (HF generate's prefix_allowed_tokens_fn over a trie of the phrases).
        free_from: ids >= it (the timestamps) are always allowed and do not move a row through the trie; default the first timestamp
        id with timestamps=, else none.  At every step the ids outside the row's allowed set — the ids that continue a phrase from
        where the row stands, eot where a phrase ends, the free ids — are -inf, where bad_words_ids acts; log-probs and top-k see the
        allowed set only.  The result gets one more, last element constraint_match, int32 [B]: the index of the phrase the row stood
        on when it emitted eot, -1 if it ended otherwise.  At most 4096 phrases of 1..64 ids inside the vocabulary, below free_from
        and without eot, no duplicates, at most 65536 trie nodes; None = off, an empty list is a ValueError.  Not in the long-form and
        chunked calls.
        top_k (1..8, needs return_logprobs): the result gets one more, last element (top_ids, top_logprobs) — per
        utterance an int32 / float32 array [generated ids, k]: at every generated position the k candidates with the largest
        processed score (HF generate(output_scores=True), then log_softmax(scores).topk(k)), descending, equal scores lowest id
        first, over the set the log-probs normalise over.  Rank 0 is the emitted id with token_logprobs' value; a rank with no finite
        candidate left holds id -1 and -inf.  Not in the long-form and chunked calls.
        sequence_bias / bad_words_ids: HF generate's options of the same names, given as ids.  sequence_bias is a dict
        {(ids...): bias} or a list of [[ids...], bias]: a length-1 sequence always adds its bias to that id's logit; a longer one adds it
        to its last id when the row's history (its prompt, then what it generated) ends with the ids before it.  bad_words_ids is a
        list of id lists with bias -inf (an [eot] entry is dropped, as HF drops it).  Order: sequence_bias, repetition_penalty,
        no_repeat_ngram_size, bad_words_ids, then the suppress lists, the timestamp rules and the log-prob sums.  At most 1024
        sequences of 1..32 ids over both; a bias is finite or -inf; None / empty = off.  ValueError otherwise.
        repetition_penalty / no_repeat_ngram_size: HF generate's options of the same names, applied on the device at every
        step to each row's own history (its prompt, then what it generated), before the suppress lists, the timestamp rules and
        the log-prob sums: every id of the history has its logit multiplied (negative) or divided (else) by the penalty, once; every id
        that would complete an n-gram the history already holds is -inf.  None / 1.0 / 0 = off.  They combine with every other option
        here; no_speech_prob and detect_language read unprocessed logits, as in HF.  ValueError: penalty <= 0, n < 0, n > 64.
        detect_language: a list of language ids (tokenizer.language_ids) — HF generate's language=None: every utterance's
        language is detected on the device in the same pass and written over the second of its n_init initial ids (n_init: default
        the shared prompt's length, required with prompts=, >= 2); returns (ids, lang) or, with return_logprobs, (ids, (…the tuple
        below…), lang) with lang = (lang_ids [B], lang_probs [B, n_lang]).  Not with return_token_timestamps.
        return_logprobs: also return (token_logprobs, avg_logprob) as (ids, (token_logprobs, avg_logprob)): per utterance the
        log-probability of every id in the layout of its id list (0 at the prompt positions), HF's log_softmax of the processed
        scores at the chosen id, and avg_logprob [B] = their mean over the generated ids (openai-whisper's avg_logprob, HF's
        _retrieve_avg_logprobs).  Works with and without prompts=; not with return_token_timestamps.
        prompts: one decoder prompt per utterance, of any lengths (`prompt` is then ignored); every row decodes as if it were
        alone with its own prompt and comes back as its own prompt + generated ids.  Not with return_token_timestamps.
        return_token_timestamps: also return, per utterance, the time in seconds each id was spoken (HF generate's
        return_token_timestamps; needs set_alignment_heads) as (ids, times); n_frames: mel frames of real audio per utterance
        (HF's attention_mask.sum(-1)), None = the whole window.
        no_speech_token (needs return_logprobs): also openai-whisper's no_speech_prob [B], HF WhisperNoSpeechDetection — the
        probability of that id under the raw logits at each row's <|startoftranscript|> position, prompt length - n_init; the second
        element becomes (token_logprobs, avg_logprob, no_speech_prob).  n_init: the number of initial ids (<|startoftranscript|>
        first); defaults to the shared prompt's length, required with prompts=."""
        k = _lib.top_k_arg(top_k, return_logprobs)
        ct = _lib.constraint_args(constraint, free_from, self.config.vocab_size, eot, timestamps)
        res = self._transcribe_batch(mel, prompt, eot, max_loop, ignore_eot, suppress_tokens, begin_suppress_tokens, timestamps,
                                     return_token_timestamps, n_frames, prompts, return_logprobs, no_speech_token, n_init, detect_language,
                                     repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids, k, ct)
        # the alternatives rode the call's log-prob pass: its tables are fetched once the pass is collected
        if k:
            res = res + (self._top_k(0, k, self._plens(prompt, prompts, len(res[0]))),)
        if ct:  # the rows' matches, likewise
            res = self._with_last(res, self._constraint_match(0, len(res[0]) if isinstance(res, tuple) else len(res)))
        return res

    def _transcribe_batch(self, mel, prompt, eot, max_loop, ignore_eot, suppress_tokens, begin_suppress_tokens, timestamps,
                          return_token_timestamps, n_frames, prompts, return_logprobs, no_speech_token, n_init, detect_language,
                          repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids, k, ct=None):
        """transcribe_batch without the top-k tables and the constraint's matches; k: what wm_set_top_k gets for the pass (0 = off),
        ct: what wm_set_constraint gets (_lib.constraint_args, None = off)"""
        rp = _lib.repeat_args(repetition_penalty, no_repeat_ngram_size)
        sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, self.config.vocab_size)
        lang = None
        if detect_language is not None:
            lang = self._lang_args(detect_language, n_init, prompt, prompts, return_token_timestamps, no_speech_token, return_logprobs)
        ns = None if lang else self._ns_args(no_speech_token, n_init, prompt, prompts, return_logprobs)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        self._set_repeat(rp, sb, k, ct)
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        opts, keep2 = self._opts(prompt, eot, max_loop, ignore_eot, suppress_tokens, begin_suppress_tokens, timestamps)
        p = keep2[0]
        if lang:
            return self._lang_call(None, ptr, on_dev, B, opts, p, prompts, max_loop, lang, return_logprobs, no_speech_token)
        if return_logprobs:
            if return_token_timestamps:
                raise ValueError("return_logprobs does not combine with return_token_timestamps")
            tab, lens = self._prompt_rows(prompts, B) if prompts is not None else (None, None)
            total = (tab.shape[1] if tab is not None else len(p)) + 1 + max_loop
            toks = np.zeros((B, total), np.int32)
            n = np.zeros(B, np.int32)
            lps = np.zeros((B, total), np.float32)
            avg = np.zeros(B, np.float32)
            rows = (_ip(tab) if tab is not None else None, _ip(lens) if tab is not None else None, tab.shape[1] if tab is not None else 0)
            if ns is not None:
                nsp = np.zeros(B, np.float32)
                _lib.check(_lib.lib().wm_transcribe_lp_ns(self._h, ptr, on_dev, B, C.byref(opts), *rows, ns[0], ns[1], _ip(toks), _ip(n),
                                                          _fp(lps), _fp(avg), _fp(nsp)))
                self.last_tokens, self.last_counts, self.last_logprobs = toks, n, lps
                return [toks[b, :n[b]].tolist() for b in range(B)], (self._split_times(lps, n, B), avg, nsp)
            _lib.check(_lib.lib().wm_transcribe_lp(self._h, ptr, on_dev, B, C.byref(opts), *rows, _ip(toks), _ip(n), _fp(lps), _fp(avg)))
            self.last_tokens, self.last_counts, self.last_logprobs = toks, n, lps
            return [toks[b, :n[b]].tolist() for b in range(B)], (self._split_times(lps, n, B), avg)
        if prompts is not None:
            if return_token_timestamps:
                raise ValueError("per-utterance prompts do not combine with return_token_timestamps")
            tab, lens = self._prompt_rows(prompts, B)
            toks = np.zeros((B, tab.shape[1] + 1 + max_loop), np.int32)
            n = np.zeros(B, np.int32)
            _lib.check(_lib.lib().wm_transcribe_rows(self._h, ptr, on_dev, B, C.byref(opts), _ip(tab), _ip(lens), tab.shape[1],
                                                     _ip(toks), _ip(n)))
            self.last_tokens, self.last_counts = toks, n
            return [toks[b, :n[b]].tolist() for b in range(B)]
        total = len(p) + 1 + max_loop
        toks = np.zeros((B, total), np.int32)
        n = np.zeros(B, np.int32)
        if return_token_timestamps:
            nf = self._frames_arg(n_frames, B)
            times = np.zeros((B, total), np.float32)
            _lib.check(_lib.lib().wm_transcribe_tt(self._h, ptr, on_dev, B, C.byref(opts), _ip(nf) if nf is not None else None,
                                                   _ip(toks), _ip(n), _fp(times)))
        else:
            _lib.check(_lib.lib().wm_transcribe(self._h, ptr, on_dev, B, C.byref(opts), _ip(toks), _ip(n)))
        self.last_tokens, self.last_counts = toks, n
        ids = [toks[b, :n[b]].tolist() for b in range(B)]
        if return_token_timestamps:
            self._align_shape = getattr(self, "_align_shape", {})
            self._align_shape[0] = (B, max_loop, self._n_align)
            return ids, self._split_times(times, n, B)
        return ids

    def transcribe_long_form(self, features, n_frames=None, prompt: Sequence[int] = PROMPT, eot: int = EOT, max_loop: int = MAX_LOOP,
                             suppress_tokens: Sequence[int] = (), begin_suppress_tokens: Sequence[int] = (),
                             timestamps=(50364, 50363, 50), return_stats: bool = False, prompt_ids: Optional[Sequence[int]] = None,
                             condition_on_prev_tokens: bool = False, prompt_condition_type: str = "first-segment",
                             prev_sot_token: int = 50361, logprob_threshold: Optional[float] = None,
                             no_speech_threshold: Optional[float] = None, no_speech_token: Optional[int] = None,
                             detect_language: Optional[Sequence[int]] = None, return_token_timestamps: bool = False,
                             repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None,
                             sequence_bias=None, bad_words_ids=None, top_k: Optional[int] = None, constraint=None, free_from=None):
        """Sequential long-form transcription (HF generate's long-form path, greedy).
        constraint / free_from: refused here (ValueError) — the window scheduler does not carry transcribe_batch's phrase-list
        constraint yet.
        top_k: refused here (ValueError) — the top-k alternatives of transcribe_batch have no place in this result yet.
        sequence_bias / bad_words_ids: as transcribe_batch, matched against each window's own decoder ids.
        repetition_penalty / no_repeat_ngram_size: as transcribe_batch.  Every window's pass sees that window's decoder
        ids only — its prompt, a carried previous text included, then what it generates — as HF's per-window generate does.
        return_token_timestamps (HF generate's option on its long-form path; needs set_alignment_heads): every utterance
        also carries "token_times", a float64 array with the time in seconds of every id of "sequence", and every segment
        "token_timestamps", its slice of it.  Works with prompt_ids, condition_on_prev_tokens and detect_language; ValueError with
        logprob_threshold / no_speech_threshold.
        detect_language: a list of language ids (HF generate's language=None) — every recording's language is detected on
        its first window and replaces the second id of `prompt` for that recording; the call then also returns the detected ids
        [B] as its last element: (out, lang) or (out, stats, lang).
        logprob_threshold / no_speech_threshold (HF generate's options, temperature 0 only; no_speech_token: the <|nospeech|> id,
        HF's no_timestamps_token_id - 1): a window with avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold is
        skipped — no segments, no ids, seek advances by the window's frames.  With either threshold every segment carries its window's
        "avg_logprob" / "no_speech_prob", every utterance its window log "windows" (skipped windows included), the stats
        "skipped_windows".  logprob_threshold alone changes no ids.  ValueError: no_speech_threshold without logprob_threshold or token.
        condition_on_prev_tokens / prompt_ids / prompt_condition_type: HF generate's options of the same names — every window's
        decoder prompt carries the utterance's previous text (up to half the decoder context) and / or prompt_ids (as
        WhisperProcessor.get_prompt_ids returns them, leading <|startofprev|> = prev_sot_token included).
        features: [B, n_mels, T] log-mel of any length T (numpy, or a CUDA tensor on this model's device), or a list of
        [n_mels, T_b] arrays; n_frames: frames of real audio per utterance (HF's attention_mask.sum(-1)), None = T (or each
        array's length).  timestamps: (timestamp_begin, no_timestamps_id, max_initial_timestamp_index | None), required.
        Returns per utterance {"sequence": ids, "segments": [{"start", "end", "tokens"}]} — HF's return_segments output with
        the padding-free sequences row; return_stats also returns {"windows", "stalled"}."""
        if top_k is not None:
            raise ValueError("top_k is not available in long-form transcription (use transcribe_batch on 30 s windows)")
        if constraint is not None or free_from is not None:
            raise ValueError("constraint is not available in long-form transcription (use transcribe_batch on 30 s windows)")
        rp = _lib.repeat_args(repetition_penalty, no_repeat_ngram_size)
        sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, self.config.vocab_size)
        lo, _keep3 = _lib.long_opts(prompt_ids, condition_on_prev_tokens, prompt_condition_type, prev_sot_token, logprob_threshold,
                                    no_speech_threshold, no_speech_token)
        if no_speech_token is not None and int(no_speech_token) >= self.config.vocab_size:
            raise ValueError(f"no_speech_token {no_speech_token} is not a vocabulary id")
        quality = logprob_threshold is not None or no_speech_threshold is not None
        tt = _lib.long_tt_args(return_token_timestamps, logprob_threshold, no_speech_threshold)
        lang_list = None
        if detect_language is not None:
            lang_list = _lib.lang_args(detect_language, self.config.vocab_size)
            if len(prompt) < 2:
                raise ValueError("detect_language needs at least two initial ids (<|startoftranscript|> and the language slot)")
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        if timestamps is None:
            raise ValueError("long-form transcription needs the timestamp rules")
        n_mels = self.config.n_mels
        if isinstance(features, (list, tuple)):
            arrs = [np.asarray(f, np.float32) for f in features]
            for f in arrs:
                if f.ndim != 2 or f.shape[0] != n_mels:
                    raise ValueError(f"each feature array must be [{n_mels}, T_b], got {f.shape}")
            lens = [f.shape[1] for f in arrs]
            feats = np.zeros((len(arrs), n_mels, max([1] + lens)), np.float32)
            for b, f in enumerate(arrs):
                feats[b, :, :lens[b]] = f
            n_frames = lens if n_frames is None else n_frames
            features = feats
        if isinstance(features, np.ndarray):
            keep = np.ascontiguousarray(features, np.float32)
            if keep.ndim == 2:
                keep = keep[None]
            if keep.ndim != 3 or keep.shape[1] != n_mels or keep.shape[0] < 1 or keep.shape[2] < 1:
                raise ValueError(f"features must be [B, {n_mels}, T], got {features.shape}")
            ptr, on_dev = C.c_void_p(keep.ctypes.data), 0
        else:
            import torch
            if not isinstance(features, torch.Tensor):
                raise TypeError("features must be a numpy array, a list of [n_mels, T_b] arrays or a torch tensor")
            t = features if features.dim() == 3 else features[None]
            if t.dim() != 3 or t.shape[1] != n_mels or t.shape[0] < 1 or t.shape[2] < 1:
                raise ValueError(f"features must be [B, {n_mels}, T], got {tuple(features.shape)}")
            if not t.is_cuda:
                return self.transcribe_long_form(t.float().numpy(), n_frames, prompt, eot, max_loop, suppress_tokens,
                                                 begin_suppress_tokens, timestamps, return_stats, prompt_ids, condition_on_prev_tokens,
                                                 prompt_condition_type, prev_sot_token, logprob_threshold, no_speech_threshold, no_speech_token,
                                                 detect_language, return_token_timestamps, repetition_penalty, no_repeat_ngram_size,
                                                 sequence_bias, bad_words_ids)
            keep = t.contiguous().float()
            torch.cuda.current_stream(keep.device).synchronize()  # the library reads it on its own HIP stream
            ptr, on_dev = C.c_void_p(keep.data_ptr()), 1
        B, T = int(keep.shape[0]), int(keep.shape[2])
        nf = self._frames_arg(n_frames, B)
        opts, _keep2 = self._opts(prompt, eot, max_loop, False, suppress_tokens, begin_suppress_tokens, timestamps)
        self._set_repeat(rp, sb)
        h = C.c_void_p()
        if tt:  # one entry point with or without the language list
            lang = np.zeros(B, np.int32)
            _lib.check(_lib.lib().wm_transcribe_long_tt(self._h, ptr, on_dev, B, T, _ip(nf) if nf is not None else None, C.byref(opts),
                                                        C.byref(lo), _ip(lang_list) if lang_list is not None else None,
                                                        lang_list.size if lang_list is not None else 0, _ip(lang), 1, C.byref(h)))
            out, stats = _lib.long_result(h, B, False, True)
            res = (out, stats) if return_stats else (out,)
            res = res + (lang,) if lang_list is not None else res
            return res if len(res) > 1 else out
        if lang_list is not None:
            lang = np.zeros(B, np.int32)
            _lib.check(_lib.lib().wm_transcribe_long_lang(self._h, ptr, on_dev, B, T, _ip(nf) if nf is not None else None, C.byref(opts),
                                                          C.byref(lo), _ip(lang_list), lang_list.size, _ip(lang), C.byref(h)))
            out, stats = _lib.long_result(h, B, quality)
            return (out, stats, lang) if return_stats else (out, lang)
        _lib.check(_lib.lib().wm_transcribe_long_ex(self._h, ptr, on_dev, B, T, _ip(nf) if nf is not None else None, C.byref(opts),
                                                    C.byref(lo), C.byref(h)))
        out, stats = _lib.long_result(h, B, quality)
        return (out, stats) if return_stats else out

    def transcribe_chunked(self, pcm, chunk_length_s: float = 30.0, stride_length_s=None, return_chunks: bool = False, return_timestamps=False,
                           sampling_rate: int = 16000, **decode_options):
        """Chunked long-form transcription (HF's ASR pipeline with chunk_length_s / stride_length_s): pcm — one 1-D array
        of 16 kHz samples, a list of them, or a CUDA tensor [R, stride] with n_samples= — is cut into overlapping chunks, the chunks of all recordings fill passes of max_batch
        rows, and every recording's ids are stitched on the GPU.  decode_options: prompt, eot, max_loop, suppress_tokens,
        begin_suppress_tokens, timestamps, detect_language, repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids (as transcribe_batch, per
        chunk) and first_special.  -> per recording {"sequence": ids, "chunks": [(start_s, len_s, stride_l_s, stride_r_s, ids_k)]
        (with return_chunks)}; see frontend.transcribe_audio_chunked.  return_timestamps: False, True (HF's segments: "segments":
        [{"timestamp": (start, end | None), "ids"}]) or "word" (also "token_timestamps" per segment, "words" with tokenizer=;
        DESIGN §31).  sampling_rate / np.int16 host arrays: resampled to 16 kHz on the GPU, where the samples stay."""
        from . import frontend
        return frontend.transcribe_audio_chunked(self, pcm, chunk_length_s, stride_length_s, return_chunks, return_timestamps=return_timestamps,
                                                 sampling_rate=sampling_rate, **decode_options)

    def alignment_weights(self, slot: int = 0) -> np.ndarray:
        """The alignment heads' cross-attention probabilities of the slot's last timestamp pass (slot 0: transcribe_batch),
        [B, n_heads_selected, max_loop, n_audio_ctx] over all positions; rows past an utterance's last fed-back id are 0."""
        B, L, n_sel = self._align_shape[slot]
        out = np.zeros((B, n_sel, L, self.config.n_audio_ctx), np.float32)
        _lib.check(_lib.lib().wm_alignment_weights(self._h, slot, _fp(out)))
        return out

    def transcribe_submit(self, mel, slot: int = 0, prompt: Sequence[int] = PROMPT, eot: int = EOT, max_loop: int = MAX_LOOP,
                          ignore_eot: bool = False, suppress_tokens: Sequence[int] = (), begin_suppress_tokens: Sequence[int] = (),
                          timestamps=None, return_token_timestamps: bool = False, n_frames=None,
                          prompts: Optional[Sequence[Sequence[int]]] = None, return_logprobs: bool = False,
                          no_speech_token: Optional[int] = None, n_init: Optional[int] = None,
                          detect_language: Optional[Sequence[int]] = None, repetition_penalty: Optional[float] = None,
                          no_repeat_ngram_size: Optional[int] = None, sequence_bias=None, bad_words_ids=None, top_k: Optional[int] = None,
                          constraint=None, free_from: Optional[int] = None):
        """Pipelined form (wm_transcribe_submit): enqueue encoder + greedy loop for this batch on pipeline slot 0..7 and
        return at once; `transcribe_wait(slot)` collects the ids.  Submitting batch i+1 before waiting for batch i lets
        its encoder overlap batch i's decode.  return_token_timestamps / n_frames: as transcribe_batch; the matching
        transcribe_wait then returns (ids, times).  return_logprobs: as transcribe_batch; the matching transcribe_wait returns
        (ids, (token_logprobs, avg_logprob)).  no_speech_token / n_init: as transcribe_batch; the matching transcribe_wait returns
        (ids, (token_logprobs, avg_logprob, no_speech_prob)).  detect_language: as transcribe_batch; the matching transcribe_wait
        returns what transcribe_batch returns.  repetition_penalty / no_repeat_ngram_size: as transcribe_batch; the pass keeps the
        values it was submitted with, and under coalesce = 2 it pairs only with a submit that carries the same values.
        sequence_bias / bad_words_ids: as transcribe_batch, kept and paired likewise (the same lists as the previous call = the same table).
        top_k: as transcribe_batch, kept and paired likewise; the matching transcribe_wait returns the extra last element.
        constraint / free_from: as transcribe_batch, kept and paired like the sequence-bias table; the matching transcribe_wait
        returns constraint_match as its last element."""
        rp = _lib.repeat_args(repetition_penalty, no_repeat_ngram_size)
        sb = _lib.seq_bias_args(sequence_bias, bad_words_ids, self.config.vocab_size)
        k = _lib.top_k_arg(top_k, return_logprobs)
        ct = _lib.constraint_args(constraint, free_from, self.config.vocab_size, eot, timestamps)
        lang = None
        if detect_language is not None:
            lang = self._lang_args(detect_language, n_init, prompt, prompts, return_token_timestamps, no_speech_token, return_logprobs)
        ns = None if lang else self._ns_args(no_speech_token, n_init, prompt, prompts, return_logprobs)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        self._set_repeat(rp, sb, k, ct)
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        opts, keep2 = self._opts(prompt, eot, max_loop, ignore_eot, suppress_tokens, begin_suppress_tokens, timestamps)
        p = keep2[0]
        self._pending_top_k = getattr(self, "_pending_top_k", {})
        self._pending_top_k[slot] = (k, self._plens(prompt, prompts, B)) if k else None
        self._pending_ct = getattr(self, "_pending_ct", {})
        self._pending_ct[slot] = B if ct else None
        if lang:
            total, tag = self._lang_call(slot, ptr, on_dev, B, opts, p, prompts, max_loop, lang, return_logprobs, no_speech_token)
            self._pending = getattr(self, "_pending", {})
            self._pending[slot] = (B, total, keep, tag)
            return
        if return_logprobs:
            if return_token_timestamps:
                raise ValueError("return_logprobs does not combine with return_token_timestamps")
            tab, lens = self._prompt_rows(prompts, B) if prompts is not None else (None, None)
            rows = (_ip(tab) if tab is not None else None, _ip(lens) if tab is not None else None, tab.shape[1] if tab is not None else 0)
            if ns is not None:
                _lib.check(_lib.lib().wm_transcribe_submit_lp_ns(self._h, slot, ptr, on_dev, B, C.byref(opts), *rows, ns[0], ns[1]))
            else:
                _lib.check(_lib.lib().wm_transcribe_submit_lp(self._h, slot, ptr, on_dev, B, C.byref(opts), *rows))
            self._pending = getattr(self, "_pending", {})
            self._pending[slot] = (B, (tab.shape[1] if tab is not None else len(p)) + 1 + max_loop, keep, "lp_ns" if ns is not None else "lp")
            return
        if prompts is not None:  # per-utterance prompts, as transcribe_batch
            if return_token_timestamps:
                raise ValueError("per-utterance prompts do not combine with return_token_timestamps")
            tab, lens = self._prompt_rows(prompts, B)
            _lib.check(_lib.lib().wm_transcribe_submit_rows(self._h, slot, ptr, on_dev, B, C.byref(opts), _ip(tab), _ip(lens), tab.shape[1]))
            self._pending = getattr(self, "_pending", {})
            self._pending[slot] = (B, tab.shape[1] + 1 + max_loop, keep, None)
            return
        if return_token_timestamps:
            nf = self._frames_arg(n_frames, B)
            _lib.check(_lib.lib().wm_transcribe_submit_tt(self._h, slot, ptr, on_dev, B, C.byref(opts),
                                                          _ip(nf) if nf is not None else None))
        else:
            _lib.check(_lib.lib().wm_transcribe_submit(self._h, slot, ptr, on_dev, B, C.byref(opts)))
        self._pending = getattr(self, "_pending", {})
        self._pending[slot] = (B, len(p) + 1 + max_loop, keep, (max_loop, self._n_align) if return_token_timestamps else None)

    def transcribe_wait(self, slot: int = 0):
        top = getattr(self, "_pending_top_k", {}).pop(slot, None)
        ct = getattr(self, "_pending_ct", {}).pop(slot, None)
        res = self._transcribe_wait(slot)
        if top:
            res = res + (self._top_k(slot, *top),)
        return self._with_last(res, self._constraint_match(slot, ct)) if ct else res

    def _transcribe_wait(self, slot):
        B, total, _keep, tt = self._pending.pop(slot)
        if isinstance(tt, tuple) and tt and tt[0] == "lang":
            return self._lang_collect(slot, B, total, tt[1], tt[2], tt[3],
                                      lambda *a: _lib.lib().wm_transcribe_wait_lang(self._h, slot, *a))
        toks = np.zeros((B, total), np.int32)
        n = np.zeros(B, np.int32)
        if tt == "lp_ns":
            lps = np.zeros((B, total), np.float32)
            avg = np.zeros(B, np.float32)
            nsp = np.zeros(B, np.float32)
            _lib.check(_lib.lib().wm_transcribe_wait_lp_ns(self._h, slot, _ip(toks), _ip(n), _fp(lps), _fp(avg), _fp(nsp)))
            self.last_tokens, self.last_counts, self.last_logprobs = toks, n, lps
            return [toks[b, :n[b]].tolist() for b in range(B)], (self._split_times(lps, n, B), avg, nsp)
        if tt == "lp":
            lps = np.zeros((B, total), np.float32)
            avg = np.zeros(B, np.float32)
            _lib.check(_lib.lib().wm_transcribe_wait_lp(self._h, slot, _ip(toks), _ip(n), _fp(lps), _fp(avg)))
            self.last_tokens, self.last_counts, self.last_logprobs = toks, n, lps
            return [toks[b, :n[b]].tolist() for b in range(B)], (self._split_times(lps, n, B), avg)
        if tt is not None:
            times = np.zeros((B, total), np.float32)
            _lib.check(_lib.lib().wm_transcribe_wait_tt(self._h, slot, _ip(toks), _ip(n), _fp(times)))
        else:
            _lib.check(_lib.lib().wm_transcribe_wait(self._h, slot, _ip(toks), _ip(n)))
        self.last_tokens, self.last_counts = toks, n
        ids = [toks[b, :n[b]].tolist() for b in range(B)]
        if tt is not None:
            self._align_shape = getattr(self, "_align_shape", {})
            self._align_shape[slot] = (B, tt[0], tt[1])
            return ids, self._split_times(times, n, B)
        return ids

    # ---- transcript scoring -------------------------------------------------------------------------------------
    def _score_out(self, tab, lens, lps, top, sm, avg, return_top_ids):
        B = len(lens)
        out = ([lps[b, :lens[b]].tolist() for b in range(B)], (sm, avg))
        return out + ([top[b, :lens[b]].tolist() for b in range(B)],) if return_top_ids else out

    def score(self, mel, ids, context_len=None, return_top_ids: bool = False):
        """How likely is this transcript for this audio: teacher-forced log-probabilities of the given ids (wm_score).
        ids: one list per clip, the decoder prompt followed by the hypothesis (a trailing eot included if it is to be scored);
        context_len: how many leading ids are context — reported but not summed — None = 1, a number, or one per row.
        -> (token_logprobs, (sum_logprob [B], avg_logprob [B])) (+ top_ids when asked): token_logprobs[b][t] = log p(ids[b][t] |
        ids[b][:t], audio) over the raw logits (HF model(..., decoder_input_ids=ids[:, :-1]).logits.float().log_softmax(-1)), 0 at
        t = 0; top_ids[b][t] the arg-max id at that position (lowest id on ties, -1 at t = 0); avg_logprob = -HF loss of the row with
        labels = -100 on the context.  Positions follow self.pos_mode."""
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        tab, lens, ctx = _lib.score_args(ids, context_len, B, self.config.vocab_size, self.config.n_text_ctx, self.max_batch)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        lps, top = np.zeros(tab.shape, np.float32), np.full(tab.shape, -1, np.int32)
        sm, avg = np.zeros(B, np.float32), np.zeros(B, np.float32)
        _lib.check(_lib.lib().wm_score(self._h, ptr, on_dev, B, self.pos_mode, _ip(tab), _ip(lens), tab.shape[1], _ip(ctx), _fp(lps),
                                       _ip(top) if return_top_ids else None, _fp(sm), _fp(avg)))
        return self._score_out(tab, lens, lps, top, sm, avg, return_top_ids)

    def score_submit(self, mel, ids, slot: int = 0, context_len=None):
        """Pipelined Whisper.score on one of the eight slots; collect with score_wait.  Everything is validated before the call and
        the slot's record is written only once the library accepted the pass."""
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        tab, lens, ctx = _lib.score_args(ids, context_len, B, self.config.vocab_size, self.config.n_text_ctx, self.max_batch)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        if not 0 <= int(slot) < 8:
            raise ValueError("slot must be 0..7")
        _lib.check(_lib.lib().wm_score_submit(self._h, slot, ptr, on_dev, B, self.pos_mode, _ip(tab), _ip(lens), tab.shape[1], _ip(ctx)))
        self._score_pending[slot] = (tab, lens, keep)

    def score_wait(self, slot: int = 0, return_top_ids: bool = False):
        pend = self._score_pending
        if slot not in pend:
            raise _lib.WhisperMiError(f"no score pass was submitted on slot {slot}")
        tab, lens, _keep = pend[slot]
        B = len(lens)
        lps, top = np.zeros(tab.shape, np.float32), np.full(tab.shape, -1, np.int32)
        sm, avg = np.zeros(B, np.float32), np.zeros(B, np.float32)
        _lib.check(_lib.lib().wm_score_wait(self._h, slot, _fp(lps), _ip(top) if return_top_ids else None, _fp(sm), _fp(avg)))
        del pend[slot]  # only a collected pass leaves the table
        return self._score_out(tab, lens, lps, top, sm, avg, return_top_ids)

    # ---- n-best scoring -----------------------------------------------------------------------------------------
    def _nbest_args(self, mel, candidates, context_len):
        ptr, on_dev, U, keep = _mel_arg(mel, self.config)
        args = _lib.nbest_args(candidates, context_len, U, self.config.vocab_size, self.config.n_text_ctx, self.max_batch)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        return ptr, on_dev, U, keep, args

    @staticmethod
    def _nbest_bufs(tab, U):
        R = tab.shape[0]
        return (np.zeros(tab.shape, np.float32), np.full(tab.shape, -1, np.int32), np.zeros(R, np.float32), np.zeros(R, np.float32),
                np.full(R, -1, np.int32), np.full(U, -1, np.int32), np.zeros(R, np.float32))

    def _nbest_out(self, args, bufs, return_top_ids):
        tab, lens, _ctx, n_cand, _utt_of, row0 = args
        lps, top, sm, avg, order, best, post = bufs
        out = []
        for u, (r0, n) in enumerate(zip(row0.tolist(), n_cand.tolist())):
            d = dict(token_logprobs=[lps[r, :lens[r]].tolist() for r in range(r0, r0 + n)], sum_logprob=sm[r0:r0 + n].copy(),
                     avg_logprob=avg[r0:r0 + n].copy(), order=order[r0:r0 + n].tolist(), best=int(best[u]), posterior=post[r0:r0 + n].copy())
            if return_top_ids:
                d["top_ids"] = [top[r, :lens[r]].tolist() for r in range(r0, r0 + n)]
            out.append(d)
        return out

    def score_candidates(self, mel, candidates, context_len=None, normalize: bool = False, return_top_ids: bool = False):
        """Several candidate transcripts per clip on one encoder run (wm_score_nbest): mel [U, n_mels, frames]; candidates: per clip
        a list of id lists, each as a row of score(); context_len: None (= 1), a number, one per candidate row (flat, clip by clip) or
        per clip a list.  -> one dict per clip: token_logprobs / sum_logprob / avg_logprob (/ top_ids) per candidate — bit for bit what
        score() gives for the candidate with the clip's mel repeated — and, made on the device over key = sum_logprob (normalize:
        avg_logprob): order (candidate indices, key descending, equal keys lower index first), best = order[0], posterior (softmax
        of the keys over the clip's candidates).  At most max_batch candidates in all."""
        ptr, on_dev, U, keep, args = self._nbest_args(mel, candidates, context_len)
        tab, lens, ctx, n_cand = args[:4]
        bufs = self._nbest_bufs(tab, U)
        lps, top, sm, avg, order, best, post = bufs
        _lib.check(_lib.lib().wm_score_nbest(self._h, ptr, on_dev, U, _ip(n_cand), int(bool(normalize)), self.pos_mode, _ip(tab), _ip(lens),
                                             tab.shape[1], _ip(ctx), _fp(lps), _ip(top) if return_top_ids else None, _fp(sm), _fp(avg),
                                             _ip(order), _ip(best), _fp(post)))
        return self._nbest_out(args, bufs, return_top_ids)

    def score_candidates_submit(self, mel, candidates, slot: int = 0, context_len=None, normalize: bool = False):
        """Pipelined score_candidates on one of the eight slots; collect with score_candidates_wait.  Everything is validated before
        the call and the slot's record is written only once the library accepted the pass."""
        ptr, on_dev, U, keep, args = self._nbest_args(mel, candidates, context_len)
        if not 0 <= int(slot) < 8:
            raise ValueError("slot must be 0..7")
        tab, lens, ctx, n_cand = args[:4]
        _lib.check(_lib.lib().wm_score_nbest_submit(self._h, slot, ptr, on_dev, U, _ip(n_cand), int(bool(normalize)), self.pos_mode, _ip(tab),
                                                    _ip(lens), tab.shape[1], _ip(ctx)))
        self._nbest_pending[slot] = (args, U, keep)

    def score_candidates_wait(self, slot: int = 0, return_top_ids: bool = False):
        pend = self._nbest_pending
        if slot not in pend:
            raise _lib.WhisperMiError(f"no n-best score pass was submitted on slot {slot}")
        args, U, _keep = pend[slot]
        bufs = self._nbest_bufs(args[0], U)
        lps, top, sm, avg, order, best, post = bufs
        _lib.check(_lib.lib().wm_score_nbest_wait(self._h, slot, _fp(lps), _ip(top) if return_top_ids else None, _fp(sm), _fp(avg), _ip(order),
                                                  _ip(best), _fp(post)))
        del pend[slot]  # only a collected pass leaves the table
        return self._nbest_out(args, bufs, return_top_ids)

    # ---- forced alignment ---------------------------------------------------------------------------------------
    def _align_args(self, mel, ids, context_len, n_frames):
        ptr, on_dev, B, keep = _mel_arg(mel, self.config)
        tab, lens, ctx, nf = _lib.align_args(ids, context_len, n_frames, B, self.config.vocab_size, self.config.n_text_ctx, self.max_batch,
                                             self.config.n_audio_ctx)
        if self._h is None:
            raise _lib.WhisperMiError("model not loaded")
        return ptr, on_dev, B, keep, tab, lens, ctx, nf

    def _align_out(self, slot, tab, lens, ctx, times, lp):
        B = len(lens)
        self._align_shape = getattr(self, "_align_shape", {})
        self._align_shape[slot] = (B, int((lens - ctx - 1).max()), self._n_align)
        out = [times[b, :lens[b]].tolist() for b in range(B)]
        return (out, self._score_out(tab, lens, lp[0], None, lp[1], lp[2], False)) if lp is not None else out

    def align(self, mel, ids, context_len=None, n_frames=None, return_logprobs: bool = False):
        """When was each id of this transcript spoken (wm_align): token timestamps of GIVEN ids, HF's _extract_token_timestamps over
        the cross-attentions of the teacher-forced pass model(features, decoder_input_ids=ids[:, :-1]) with num_input_ids =
        context_len.  ids / context_len: as score() (context ids get time 0); n_frames: as transcribe_batch.  Needs
        set_alignment_heads.  -> times, one list per row with one time per id; return_logprobs: (times, what score() returns for the
        same inputs, computed by the same pass).  alignment_weights() then serves this pass: [B, heads, max_b R_b, n_audio_ctx] with
        R_b = len_b - context_len_b - 1."""
        ptr, on_dev, B, keep, tab, lens, ctx, nf = self._align_args(mel, ids, context_len, n_frames)
        times = np.zeros(tab.shape, np.float32)
        lp = (np.zeros(tab.shape, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)) if return_logprobs else None
        _lib.check(_lib.lib().wm_align(self._h, ptr, on_dev, B, self.pos_mode, _ip(tab), _ip(lens), tab.shape[1], _ip(ctx),
                                       _ip(nf) if nf is not None else None, _fp(times), *([_fp(a) for a in lp] if lp else [None] * 3)))
        return self._align_out(0, tab, lens, ctx, times, lp)

    def align_submit(self, mel, ids, slot: int = 0, context_len=None, n_frames=None, return_logprobs: bool = False):
        """Pipelined Whisper.align on one of the eight slots; collect with align_wait.  Everything is validated before the call and
        the slot's record is written only once the library accepted the pass."""
        ptr, on_dev, B, keep, tab, lens, ctx, nf = self._align_args(mel, ids, context_len, n_frames)
        if not 0 <= int(slot) < 8:
            raise ValueError("slot must be 0..7")
        _lib.check(_lib.lib().wm_align_submit(self._h, slot, ptr, on_dev, B, self.pos_mode, _ip(tab), _ip(lens), tab.shape[1], _ip(ctx),
                                              _ip(nf) if nf is not None else None, int(bool(return_logprobs))))
        self._align_pending[slot] = (tab, lens, ctx, bool(return_logprobs), keep)

    def align_wait(self, slot: int = 0):
        pend = self._align_pending
        if slot not in pend:
            raise _lib.WhisperMiError(f"no align pass was submitted on slot {slot}")
        tab, lens, ctx, want_lp, _keep = pend[slot]
        B = len(lens)
        times = np.zeros(tab.shape, np.float32)
        lp = (np.zeros(tab.shape, np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)) if want_lp else None
        _lib.check(_lib.lib().wm_align_wait(self._h, slot, _fp(times), *([_fp(a) for a in lp] if lp else [None] * 3)))
        del pend[slot]  # only a collected pass leaves the table
        return self._align_out(slot, tab, lens, ctx, times, lp)

    def align_phases(self, slot: int = 0) -> dict:
        """GPU milliseconds of the phases of the slot's last collected align pass (wm_align_phases)."""
        ms = np.zeros(6, np.float32)
        _lib.check(_lib.lib().wm_align_phases(self._h, slot, _fp(ms)))
        return dict(zip(("encoder", "prefill", "ln", "sweep", "merge", "align"), (float(v) for v in ms)))

    def score_phases(self, slot: int = 0) -> dict:
        """GPU milliseconds of the phases of the slot's last collected score pass (wm_score_phases; slot 0 also serves score)."""
        ms = np.zeros(5, np.float32)
        _lib.check(_lib.lib().wm_score_phases(self._h, slot, _fp(ms)))
        return dict(zip(("encoder", "prefill", "ln", "sweep", "merge"), (float(v) for v in ms)))

    def transcribe_wait_device(self, slot: int, packed) -> None:
        """transcribe_wait with the ids left on the GPU as the multi-GPU gather buffer: `packed` is a torch int32 CUDA tensor
        [rows, 1 + stride] on this model's device; row r becomes [length, ids zero-padded] (dist.gather_tokens_device)."""
        B, total, _keep, _tt = self._pending.pop(slot)
        rows, width = int(packed.shape[0]), int(packed.shape[1])
        if not packed.is_cuda or packed.dtype.itemsize != 4 or not packed.is_contiguous():
            raise ValueError("packed must be a contiguous int32 CUDA tensor")
        import torch
        # the library writes `packed` on its own HIP stream: whatever torch still has queued on the buffer (the fill that made it)
        # must have run, or it lands on top of the packed rows
        torch.cuda.current_stream(packed.device).synchronize()
        _lib.check(_lib.lib().wm_transcribe_wait_device(self._h, slot, C.c_void_p(packed.data_ptr()), rows, width - 1))
        self.last_tokens = self.last_counts = None

    def loop_steps(self, slot: int = 0) -> int:
        """Loop iterations (whisper.mojo:205) enqueued for the slot's most recent completed pass: max_loop unless the early exit
        (every utterance emitted eot, whisper.mojo:206-207) cut the loop.  Slot 0 also serves transcribe_batch."""
        return int(_lib.lib().wm_transcribe_steps(self._h, slot))

    def transcribe(self, mel) -> List[int]:
        """whisper.mojo:184-223: mel [80, 3000] -> token ids."""
        return self.transcribe_batch(mel)[0]
