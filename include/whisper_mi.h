/* whisper_mi.h — C-ABI of libwhispermi.so: the MI355X (gfx950) replacement for the hot path of
 * antonvice/whisper.Mojo.  Plain C, no torch / C++ types cross this boundary.
 *
 * The reference has no FFI of its own (it is one Mojo program); the surface below is what a Mojo
 * `sys.ffi.DLHandle` (or Python ctypes) binding of that program would bind, one entry per reference
 * function it replaces (file:line relative to the reference repo).  INTEGRATION.md shows the Mojo stub.
 *
 * Conventions: every function returns 0 on success or a negative WM_E_* code and never throws;
 * wm_last_error() gives the message (thread-local).  Opaque handles own all device memory; every host
 * buffer is caller-owned and caller-sized, except the result of long-form transcription (wm_long_result): its per-utterance
 * id lists and segment lists have lengths nobody knows before the run, so it is an opaque handle that the caller sizes its
 * buffers from (wm_long_result_sizes) and frees (wm_long_result_free).  One wm_model lives on one GPU; calls on one handle must be
 * serialised by the caller (the reference is single-caller too: whisper.mojo:184 takes self immutably and
 * builds its cache locally).  Different handles (other GPUs / processes) are independent.
 */
#ifndef WHISPER_MI_H
#define WHISPER_MI_H
#include <stddef.h>
#include <stdint.h>
#include "wm_synth.h" /* wm_dims */

#ifdef __cplusplus
extern "C" {
#endif

enum { WM_OK = 0, WM_E_ARG = -1, WM_E_SIZE = -2, WM_E_IO = -3, WM_E_HIP = -4, WM_E_STATE = -5 };
enum { WM_F32 = 0, WM_BF16 = 1, WM_F16 = 2 };
enum { WM_GELU_TANH = 0 /* whisper_tensor.mojo:288-308 */, WM_GELU_ERF = 1 /* HF */ };
enum { WM_POS_REF = 0 /* start_pos = current_len-1, whisper.mojo:217 */, WM_POS_HF = 1 /* = current_len */ };

/* Replaces WhisperConfig (whisper.mojo:15-31) + config.mojo:4-17.  dims.d_model / dims.n_heads must be 64
 * (layers.mojo:190-198 hard-codes a 64-wide head).  Shapes the kernels are instantiated for: d_model 128, 384 (tiny) or 512
 * (base) with ffn <= 2048 whose ffn/32 splits into <= 16 x <= 4, d_model 768 with 12 heads and ffn 3072 (small), and d_model 1024 with 16 heads and ffn 4096 (medium).  Anything else
 * is refused at load with WM_E_ARG and a message that names the field. */
typedef struct {
    wm_dims dims;
    int gelu_mode;     /* WM_GELU_* */
    int compute_dtype; /* WM_F32: exact fp32 MFMA everywhere.  WM_BF16 / WM_F16: GEMM operands (weights and
                          the activations fed to them) are 16-bit, accumulation / LayerNorm / softmax /
                          residual stream stay fp32 */
    int kv_dtype;      /* storage type of the self- and cross-attention K/V cache: WM_F32 or compute_dtype */
    int max_batch;     /* largest B any later call will pass (arena sizing) */
    int decoder_fp32;  /* != 0: compute_dtype applies to the ENCODER only (conv stem, encoder blocks, cross-K/V projection); the
                          decoder's weights and MFMA operands stay fp32 — BASELINE config 3 read literally ("bf16 encoder GEMMs").
                          0 (a zero-filled tail): one dtype for both, as before */
    int coalesce;      /* 2: two consecutive wm_transcribe_submit calls with the same batch size and options share ONE decode state of
                          2·B rows (the latency-bound launches of a decode step cost the same for 128 rows as for 64): the first call of
                          a pair is held until its partner arrives — or until it is waited for, then it runs alone — and every call
                          still gets exactly its own ids, bit-identical to an uncoalesced run (nothing in an utterance's arithmetic
                          depends on the batch it rides in).  A host-side mel buffer must then stay valid until the matching wait.
                          0 / 1: off */
} wm_config;

/* Replaces the literals in Whisper.transcribe (whisper.mojo:187-191 prompt, :206 eot, :205 loop bound). */
typedef struct {
    const int32_t* prompt;
    int n_prompt;
    int eot;
    int max_loop;   /* reference: 195 -> at most n_prompt + 1 + 195 ids per utterance */
    int pos_mode;   /* WM_POS_* */
    int ignore_eot; /* != 0: "fixed" mode — never stop early (bench) */
    /* SURVEY §8f rank 4 — logit masks the reference lacks (whisper.mojo:198,219 take the raw argmax), with the semantics
     * of HF generate's SuppressTokensLogitsProcessor / SuppressTokensAtBeginLogitsProcessor; applied inside the fused
     * argmax, never to the logits wm_decode_step returns.  NULL / 0 = none (the reference's behaviour). */
    const int32_t* suppress_tokens;       /* ids that can never be emitted */
    int n_suppress;
    const int32_t* begin_suppress_tokens; /* ids that cannot be the FIRST generated token */
    int n_begin_suppress;
    /* Timestamp rules, same row: the semantics of HF generate's WhisperTimeStampLogitsProcessor, applied after the two suppress
     * masks inside the fused argmax — timestamps come in pairs, never decrease, the first generated id is a timestamp no
     * later than timestamp_begin + max_initial_timestamp_index, <|notimestamps|> is never emitted, and whenever the
     * probability mass of all admissible timestamps exceeds the most likely text id the id is a timestamp.  `eot` doubles as
     * the processor's eos_token_id (ids below it are "normal text").  timestamp_begin <= 0 = off (the reference's behaviour;
     * a zero-filled struct tail keeps it off). */
    int timestamp_begin;             /* id of <|0.00|> (50364 for the multilingual vocabulary) */
    int no_timestamps_token;         /* id of <|notimestamps|> (50363), or < 0 */
    int max_initial_timestamp_index; /* HF generation config default 50 (= 1.00 s); < 0 = unlimited */
} wm_decode_opts;

typedef struct wm_model wm_model;
typedef struct wm_state wm_state;

const char* wm_last_error(void);

/* wm_config and wm_decode_opts have grown round by round (decoder_fp32, the timestamp fields) and carry no size field: a host
 * built against an older header would hand the library structs whose tail it never wrote.  WM_ABI_VERSION is bumped with every
 * such change; a host binding compares it with wm_abi_version() once after loading the library and refuses a mismatch (the
 * Python and C++ mirrors do). */
#define WM_ABI_VERSION 5
int wm_abi_version(void);

/* ---- WeightLoader(filename) + Whisper() + Whisper.load(loader)   loader.mojo:10-27, whisper.mojo:175-182 ----
 * path: the reference's headerless little-endian fp32 file (order of export_weights.py:19-90).  Unlike the
 * reference (loader.mojo:21-27 reads past the end silently) the byte size is validated: WM_E_SIZE. */
int wm_model_load(const char* path, const wm_config* cfg, int device, wm_model** out);
/* Same from a host image of n_floats fp32 values. */
int wm_model_load_memory(const float* weights, size_t n_floats, const wm_config* cfg, int device, wm_model** out);
void wm_model_free(wm_model* m);
size_t wm_weight_count(const wm_dims* dims);

/* ---- weight file format v2 ------------------------------------------------------------------------
 * v1 = the reference's headerless fp32 dump.  v2 = 64-byte header (magic "WMIWGT2", version, matrix dtype, dims, flags,
 * payload size) + the same tensors in the same order, conv / linear matrices in `dtype` (WM_F32 / WM_BF16 / WM_F16), all
 * vectors and positional tables in fp32; the token embedding stays fp32 when emb_f32 != 0 (then a v2 file in the model's
 * compute dtype loads to exactly the weights the v1 file gives).  wm_model_load accepts either format and validates
 * size / dims.  wm_weights_read expands either format to the fp32 image (wm_weight_count(dims) floats).  Host-only. */
int wm_weights_convert_v2(const char* v1_path, const char* v2_path, const wm_dims* dims, int dtype, int emb_f32);
int wm_weights_read(const char* path, const wm_dims* dims, float* out);

/* ---- KVCache(n_layers, d_model, 448)   layers.mojo:55-63 — one per batch of B utterances ------------------- */
int wm_state_new(wm_model* m, int batch, wm_state** out);
int wm_state_reset(wm_state* s); /* current_len = 0, has_cross = false */
void wm_state_free(wm_state* s);
int wm_state_len(const wm_state* s); /* LayerCache.current_len (layers.mojo:18) */

/* ---- WhisperEncoder.forward(mel) -> Tensor   whisper.mojo:71-99 ---------------------------------------------
 * mel: [B, n_mels, 2*n_audio_ctx] fp32 row-major (sample_input.bin layout, main.mojo:23-27); host pointer, or
 * a device pointer on the model's GPU when mel_on_device != 0.  Resets `s`, keeps the encoder output inside it
 * for the decoder, and (if enc_out != NULL) copies it to host as [B, n_audio_ctx, d_model] fp32. */
int wm_encode(wm_model* m, wm_state* s, const float* mel, int mel_on_device, int B, float* enc_out);
/* Stage-level tests: inject an encoder output [B, n_audio_ctx, d_model] (host) instead of running the encoder. */
int wm_state_set_encoder_output(wm_model* m, wm_state* s, const float* enc_out, int B);

/* ---- WhisperDecoder.forward(tokens, enc_out, cache, use_cache=True, start_pos) -> logits  whisper.mojo:130-167 --
 * tokens [B, q_len] (host), start_pos [B] (host; the reference passes one Int — per-utterance here; it stays a
 * CALLER argument so that the position quirk of whisper.mojo:217 lives in the host loop).  Appends q_len
 * positions to the cache (layers.mojo:140-143); computes the cross K/V on first use (layers.mojo:150-154).
 * logits: NULL or host [B, vocab] for the last position; next: NULL or host [B] = argmax (lowest index wins,
 * whisper_tensor.mojo:431-439). */
int wm_decode_step(wm_model* m, wm_state* s, const int32_t* tokens, int q_len, const int32_t* start_pos,
                   float* logits, int32_t* next);

/* ---- Whisper.transcribe(mel) -> List[Int]   whisper.mojo:184-223 ------------------------------------------
 * tokens_out: host [B, n_prompt + 1 + max_loop]; row b holds prompt + generated ids (incl. the trailing eot when
 * hit), exactly the reference's list; n_tokens[b] = its length.  The whole greedy loop runs on the GPU (token
 * feedback never visits the host); the host only reads a device-written "utterances finished" word between sub-chunks of 8 steps
 * and stops enqueueing once every utterance has emitted eot (see wm_transcribe_submit). */
int wm_transcribe(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                  int32_t* tokens_out, int32_t* n_tokens);

/* Pipelined form for back-to-back batches (serving / bench): wm_transcribe_submit enqueues the encoder, the prompt prefill and
 * the greedy loop on the slot's own HIP stream and returns immediately; wm_transcribe_wait blocks until that slot's ids are
 * ready and copies them out (same layout as wm_transcribe).  Eight slots (0..7): submitting batch i+1 before waiting for batch i
 * overlaps its MFMA-bound encoder with batch i's latency/HBM-bound decode; four passes in flight is the measured optimum (the chip
 * runs four hardware queues at a time, and ROCm must be allowed that many per-process queues: GPU_MAX_HW_QUEUES >= 8 in the
 * environment before HIP initialises — see INTEGRATION.md).
 * The loop stops like the reference's (whisper.mojo:206-207: break at eot — here: once EVERY utterance of the batch has emitted
 * eot): with ignore_eot == 0 it is enqueued in sub-chunks of 8 steps, two sub-chunks ahead of the GPU, by a host thread of the
 * library that reads a device-written "utterances finished" word between sub-chunks (no stream synchronisation); it therefore runs
 * at most 16 steps (+ the sub-chunk in progress) past the longest utterance, and the ids are identical to wm_transcribe's.  With
 * ignore_eot != 0 ("fixed" mode) all max_loop steps are enqueued at submit.  mel must stay valid until the matching wait when it
 * is a device pointer. */
int wm_transcribe_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts);
int wm_transcribe_wait(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens);
/* wm_transcribe_wait for the multi-GPU path: the slot's result stays ON THE DEVICE, packed as the gather buffer the one
 * collective of a batch moves — dev_packed [rows_cap, 1 + stride] int32 in the caller's DEVICE memory (e.g. a torch tensor handed to
 * RCCL's all-gather): row r = [n_tokens[r], ids zero-padded to stride]; rows past the batch are zero (ragged shards gather a fixed
 * row count per rank).  rows_cap >= B, stride >= n_prompt + 1 + max_loop.  Returns when the buffer is complete. */
int wm_transcribe_wait_device(wm_model* m, int slot, int32_t* dev_packed, int rows_cap, int stride);
/* Loop iterations that were enqueued for the slot's most recent completed pass (slot 0 also serves wm_transcribe): max_loop when
 * the pass ran to its bound, less when the early exit cut it.  -1: no pass yet / bad slot.  Diagnostics and tests. */
int wm_transcribe_steps(wm_model* m, int slot);

/* ---- per-row prompts -------------------------------------------------------------------------------------------
 * wm_transcribe / wm_transcribe_submit with a decoder prompt that differs from row to row, in content and in length: row b decodes
 * exactly as if it were decoded alone with its own prompt (HF generate's left-padded batch with decoder_attention_mask).
 * prompts: host [B][prompt_stride], row b holds prompt_len[b] ids; opts->prompt / n_prompt are ignored.  With Lmax the longest
 * prompt_len: tokens_out host [B][Lmax + 1 + max_loop], row b = its own prompt (unpadded) + generated ids; n_tokens[b] its length.
 * The timestamp rules and the suppress masks start at the first generated id as always.  The prefill runs in chunks of 16
 * positions.  WM_E_ARG, nothing launched: prompt_len[b] < 1 or > prompt_stride, an id outside the vocabulary,
 * Lmax + 1 + max_loop > n_text_ctx.  Not supported: per-row prompts with token timestamps (there is no _tt form), pairing under
 * coalesce = 2 (such a submit always runs alone), multi-lane decode states (WM_E_ARG, also up front).  Collected with wm_transcribe_wait (out
 * stride Lmax + 1 + max_loop). */
int wm_transcribe_rows(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts, const int32_t* prompts,
                       const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens);
int wm_transcribe_submit_rows(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                              const int32_t* prompts, const int32_t* prompt_len, int prompt_stride);

/* ---- log-probabilities -------------------------------------------------------------------------------------------
 * wm_transcribe / wm_transcribe_submit / wm_transcribe_rows with the log-probability of every generated id (the ids after the prompt,
 * a trailing eot included) and their mean per row: openai-whisper's avg_logprob, HF generate(output_scores=True) followed by
 * WhisperGenerationMixin._retrieve_avg_logprobs(scores, ids, 0.0).  logprob = s[id] - logsumexp_j s[j], s the logits row after the
 * processors this library applies: ids removed by suppress_tokens, by begin_suppress_tokens (first generated id only) or by the
 * timestamp rules are -inf; when the timestamp rule forces a timestamp every text id is -inf and the normaliser runs over the
 * admissible timestamps alone; with the rules off it runs over everything the mask leaves.  Computed by the fused argmax on the
 * captured-graph path (stage 1 adds one exp per logit, stage 2 one merge); a pass without _lp launches exactly what it did before.
 * prompts NULL: the shared prompt opts->prompt (prompt_len, prompt_stride ignored; the wm_transcribe_submit path, pairs under
 * coalesce = 2 only with other _lp submits of the same shape and options); non-NULL: per-row prompts as wm_transcribe_rows (runs alone).
 * token_logprobs: host fp32 in the layout of tokens_out; prompt positions and positions at and past n_tokens[b] are 0.
 * avg_logprob: host [B], sum of the row's generated log-probs / their count; 0 when nothing was generated.
 * A step whose candidates are all -inf (a mask over the whole vocabulary) emits id 0, as always; its log-prob is -inf, never NaN.
 * WM_E_ARG, nothing launched: multi-lane decode states.  Log-probs together with token timestamps are not supported (there is no
 * entry that asks for both).  wm_transcribe_wait_lp on a slot submitted without log-probs returns WM_E_STATE; wm_transcribe_wait on
 * an _lp slot returns the ids. */
int wm_transcribe_lp(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts, const int32_t* prompts,
                     const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs,
                     float* avg_logprob);
int wm_transcribe_submit_lp(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                            const int32_t* prompts, const int32_t* prompt_len, int prompt_stride);
int wm_transcribe_wait_lp(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob);

/* ---- no-speech probability ------------------------------------------------------------------------------------
 * The _lp trio plus openai-whisper's no_speech_prob, HF WhisperNoSpeechDetection: per row the softmax, in fp32 over the whole
 * vocabulary, of the RAW decoder logits (no suppress mask, no begin-suppress, no timestamp rules) at the position of
 * <|startoftranscript|> in the row's decoder input, read at no_speech_token (HF: no_timestamps_token_id - 1; here the caller names
 * it).  That position is prompt_len[b] - n_init (opts->n_prompt - n_init with the shared prompt), n_init the number of initial ids
 * (<|startoftranscript|> first); previous-text conditioning and prompt_ids come before them.  The prefill keeps the position's last
 * hidden row, one extra vocabulary sweep (the log-prob logits kernel, unmasked, into buffers of its own) and one small kernel run
 * between the prefill and the greedy loop; ids, token log-probs and avg_logprob are bit for bit those of the _lp call, and a pass
 * without _ns launches exactly what it did before.  no_speech_prob: host [B].
 * WM_E_ARG, nothing launched: what _lp refuses; no_speech_token outside [0, vocab); n_init < 1; n_init larger than a row's prompt.
 * Under coalesce = 2 such a submit pairs only with another of the same shape, options, token and n_init.  wm_transcribe_wait_lp_ns on
 * a slot submitted without the probe returns WM_E_STATE; the older waits on a probe slot return what they always return. */
int wm_transcribe_lp_ns(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts, const int32_t* prompts,
                        const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, int32_t* tokens_out, int32_t* n_tokens,
                        float* token_logprobs, float* avg_logprob, float* no_speech_prob);
int wm_transcribe_submit_lp_ns(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                               const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init);
int wm_transcribe_wait_lp_ns(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                             float* no_speech_prob);

/* ---- language detection ---------------------------------------------------------------------------------------
 * HF WhisperGenerationMixin.detect_language / openai-whisper detect_language: one decoder pass over [sot_token] alone at position 0,
 * the logits of the n_lang candidate ids only, their arg-max (ties: the smaller token id, as an arg-max over the vocabulary row with
 * the rest at -inf) and their softmax.  lang_ids: host [n_lang], 1 <= n_lang <= 128, any order, no duplicates.
 *
 * wm_detect_language: the encoder, the [sot] pass and the kernel.  lang_out: [B] token ids; probs_out: [B][n_lang] in list order, or
 * NULL.  Uses slot 0's state, like wm_transcribe: afterwards that state holds no usable encoder output or K/V (its cache slot 0 was
 * written by the [sot] pass), exactly as after wm_transcribe.  States of wm_state_new (wm_encode / wm_decode_step) are not touched.
 *
 * The _lang trio: the arguments of the _lp_ns trio plus the list, n_init (required, >= 2: the initial ids are the last n_init ids of
 * every row, the language is the second of them) and the outputs lang_out [B], lang_probs [B][n_lang] (or NULL).  The language is
 * detected on the device between the encoder and the prefill and written into each row's slot of the prompt table; nothing is read
 * back before the wait and the audio is encoded once.  The id given at the language slot is a placeholder.  prompts == NULL:
 * opts->prompt for every row.  token_logprobs == NULL and avg_logprob == NULL: a plain pass; no_speech_token < 0: no probe (then
 * no_speech_prob is not written; a probe needs the log-prob outputs).  Always a per-row-prompt pass on a single-lane state; under
 * coalesce = 2 it runs alone.  With everything on, ids, log-probs and no_speech_prob are those of _lp_ns called with the detected
 * prompts.  The returned ids carry the detected language.
 * WM_E_ARG, nothing launched: n_lang outside [1, 128]; an id outside the vocabulary or a duplicate; n_init < 2 or larger than a
 * row's prompt; sot_token outside the vocabulary; a multi-lane decode state; rows whose initial ids do not start with the same id
 * (one [sot] pass serves all rows); a probe without the log-prob outputs; what _rows / _lp / _lp_ns refuse.
 * wm_transcribe_wait_lang on a slot submitted without detection returns WM_E_STATE; the older waits on a _lang slot return what
 * they always return.  There is no token-timestamp form. */
int wm_detect_language(wm_model* m, const float* mel, int mel_on_device, int B, int sot_token, const int32_t* lang_ids, int n_lang,
                       int32_t* lang_out, float* probs_out);
int wm_transcribe_lang(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts, const int32_t* prompts,
                       const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
                       int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob,
                       int32_t* lang_out, float* lang_probs);
int wm_transcribe_submit_lang(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                              const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init,
                              const int32_t* lang_ids, int n_lang, int want_logprobs);
int wm_transcribe_wait_lang(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                            float* no_speech_prob, int32_t* lang_out, float* lang_probs);

/* ---- transcript scoring ---------------------------------------------------------------------------------------
 * How likely is THIS transcript for THIS audio: teacher-forced log-probabilities, HF
 * model(input_features, decoder_input_ids=y[:, :-1]).logits.float().log_softmax(-1) gathered at y[:, 1:].  Row b holds the ids
 * y[0 .. ids_len[b]) — the decoder prompt followed by the hypothesis, a trailing eot included if it is to be scored — at
 * ids[b * ids_stride]; context_len[b] in [1, ids_len[b] - 1] of them are context (NULL: 1 for every row).  For t in [1, ids_len[b]):
 *   token_logprobs[b][t] = z[t-1][y[t]] - logsumexp_j z[t-1][j]      top_ids[b][t] = argmax_j z[t-1][j]  (lowest id on ties)
 * z the RAW decoder logits after input t-1 (no suppress masks, no timestamp rules), fp32 normaliser over the whole vocabulary.
 * token_logprobs[b][0] = 0, top_ids[b][0] = -1; positions at and past ids_len[b] are 0 / -1.  sum_logprob[b] = the sum over
 * t >= context_len[b] (positions 1 .. context_len - 1 are reported, not summed); avg_logprob[b] = that sum / (ids_len[b] -
 * context_len[b]) = -HF loss of the row with labels = -100 on the context.  token_logprobs, top_ids (or NULL): host [B][ids_stride];
 * sum_logprob, avg_logprob: host [B].
 * pos_mode: WM_POS_HF — input t sits at position t; WM_POS_REF — position t for t < context_len[b] and t - 1 from there on (the
 * current_len - 1 of whisper.mojo:217), so that scoring the ids a WM_POS_REF transcription returned, with context_len = its prompt
 * length, reproduces that pass's own hidden rows.
 * One encoder run, the per-row prefill of wm_transcribe_rows over y[0 .. len - 1) (chunks of 16 positions, no logits launch), then one
 * LayerNorm launch, one vocabulary sweep for all sum(ids_len[b] - 1) rows and a merge: no loop, no captured graph, and no logits
 * matrix.  Rows are independent: a row scored in any batch gives the same bits.  Single-lane decode states only; under coalesce = 2 a
 * score submit always runs alone.  wm_score uses slot 0's state like wm_transcribe; afterwards the slot's state holds no usable pass.
 * WM_E_ARG, nothing launched: ids_len[b] < 2 or > min(ids_stride, n_text_ctx); context_len[b] outside [1, ids_len[b] - 1]; an id
 * outside the vocabulary; B over max_batch; a bad pos_mode; a multi-lane decode state.  wm_score_wait on a slot that holds a
 * transcribe pass returns WM_E_STATE, and so do the wm_transcribe_wait family on a score slot (the pass stays pending).
 * The id arrays are copied at submit; mel must stay valid until the matching wait when it is a device pointer. */
int wm_score(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride,
             const int32_t* context_len, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob);
int wm_score_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                    int ids_stride, const int32_t* context_len);
int wm_score_wait(wm_model* m, int slot, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob);
/* Diagnostics (tools/score_cost.py): GPU time of the phases of the slot's last collected score pass (slot 0 also serves wm_score), from
 * HIP events on the pass's stream, milliseconds: ms[0] encoder, [1] prefill chunks + row collection, [2] final LayerNorm, [3] vocabulary
 * sweep, [4] merge + sums.  WM_E_STATE: no completed score pass on the slot's state, or it has started another pass since. */
int wm_score_phases(wm_model* m, int slot, float* ms);
/* PCM in (the layout of wm_log_mel): front end + wm_score without the mel leaving the GPU */
int wm_score_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                 const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_logprobs, int32_t* top_ids, float* sum_logprob,
                 float* avg_logprob);

/* ---- n-best scoring ---------------------------------------------------------------------------------------------
 * Several candidate transcripts per clip on ONE encoder run: mel holds U clips (as wm_score takes it), clip u has n_cand[u] >= 1
 * candidates, and the R = sum n_cand[u] id rows — ids, ids_len, ids_stride, context_len exactly as wm_score takes and validates them —
 * are grouped by clip in the caller's order (clip 0's candidates first).  The encoder and the cross-K/V projection run over the U
 * clips, the decoder over the R rows; each row's cross-attention reads its clip's encoder output through a row map.
 * Per row: token_logprobs, top_ids (or NULL) [R][ids_stride], sum_logprob, avg_logprob [R] are what wm_score writes for the same rows
 * with each clip's mel repeated n_cand[u] times, bit for bit.
 * Per clip, computed on the device with key[c] = sum_logprob of the clip's candidate c (normalize != 0: avg_logprob) and row0[u] =
 * n_cand[0] + .. + n_cand[u - 1]:
 *   order [R]: entries [row0[u], row0[u] + n_cand[u]) hold the candidate indices 0 .. n_cand[u] - 1 sorted by key descending, equal
 *     keys lower index first;   best [U] = order[row0[u]];
 *   posterior [R]: exp(key_c - M_u) / sum_j exp(key_j - M_u) over the clip's candidates, M_u the clip's largest key, the sum in
 *     ascending candidate order (fp32, expf): with normalize = 0 the model's posterior over the candidate list.  A clip's results do
 *     not depend on the other clips of the call.
 * WM_E_ARG, nothing launched: everything wm_score refuses, per row; U < 1 or an n_cand[u] < 1; R over max_batch; a multi-lane decode
 * state.  State rules as wm_score: never coalesced, slot 0's state for the synchronous forms, no usable pass afterwards; the
 * wm_transcribe_wait, wm_score_wait, wm_align_wait and wm_score_nbest_wait families refuse each other's passes with WM_E_STATE (the
 * pass stays pending).  The next pass of any kind on the state clears the row map.  wm_score_phases serves the pass (its merge
 * phase includes the ranking launch). */
int wm_score_nbest(wm_model* m, const float* mel, int mel_on_device, int U, const int32_t* n_cand, int normalize, int pos_mode,
                   const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_logprobs,
                   int32_t* top_ids, float* sum_logprob, float* avg_logprob, int32_t* order, int32_t* best, float* posterior);
int wm_score_nbest_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int U, const int32_t* n_cand, int normalize, int pos_mode,
                          const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len);
int wm_score_nbest_wait(wm_model* m, int slot, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob, int32_t* order,
                        int32_t* best, float* posterior);
/* PCM in (the layout of wm_log_mel, U rows): front end + wm_score_nbest without the mel leaving the GPU */
int wm_score_nbest_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int U, int stride, const int32_t* n_cand, int normalize,
                       int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len,
                       float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob, int32_t* order, int32_t* best,
                       float* posterior);

/* ---- repetition processors -------------------------------------------------------------------------------------
 * HF generate's repetition_penalty (RepetitionPenaltyLogitsProcessor) and no_repeat_ngram_size (NoRepeatNGramLogitsProcessor) for
 * every greedy pass asked for from now on: wm_transcribe and its _submit / _rows / _lp / _lp_ns / _lang / _tt / _pcm forms and the
 * wm_transcribe_long family (a model-wide setting, like the alignment heads; a submit that is held for a coalesce = 2 partner keeps the
 * values in force when it was made, and pairs only with a submit made under the same values).  At every step, with hist the row's
 * decoder ids so far (its own prompt, then what it generated) and z its fp32 logits, in this order and before the suppress masks, the
 * timestamp rules, the arg-max and the log-prob sums:
 *   1. every id t in hist, once: z[t] = z[t] * penalty if z[t] < 0, else z[t] / penalty;
 *   2. with n = no_repeat_ngram_size >= 1 and len(hist) + 1 >= n: every id that follows an occurrence of hist's last n - 1 ids inside
 *      hist is -inf (n = 1: every id of hist).
 * Log-probs are those of the processed row: a banned id adds nothing to the normaliser, a penalised one exp of its penalised value.
 * The no-speech probe, language detection, wm_score and wm_align read unprocessed logits.  A long-form window's pass sees that
 * window's decoder ids only (a carried previous text included).  Both run on the device inside the captured step: two bit sets per
 * row, kept by the step's arg-max launch and read by the logits kernel; a pass with both off launches exactly what it did before.
 * penalty 1 and n 0 = off (the default).  WM_E_ARG: penalty <= 0 or not finite, n < 0 or n > 64.
 * The setting PERSISTS until the next wm_set_repeat_options on the model: a caller that wants one pass processed sets the values
 * before it and sets (1, 0) after it (the Python layer sets them on every greedy call).  It is read once, when a pass is asked
 * for; like every call on a wm_model it is not synchronised — threads that share a model serialise set + submit themselves. */
int wm_set_repeat_options(wm_model* m, float repetition_penalty, int no_repeat_ngram_size);

/* ---- top-k alternatives per generated id ---------------------------------------------------------------------------
 * HF generate(output_scores=True) followed by log_softmax(scores).topk(k) per step, for every log-prob pass asked for from now on
 * (wm_transcribe_lp / _lp_ns / _lang with log-probs, their submit forms and wm_transcribe_rows' log-prob kin), under the rules of
 * wm_set_repeat_options: model-wide, it persists until the next call, a submit held for a coalesce = 2 partner keeps the value in
 * force when it was made and pairs only with a submit made under the same value.  Passes without log-probs, wm_score, wm_align and
 * wm_detect_language ignore it; the long-form and chunked entries refuse to run while it is non-zero (WM_E_ARG).
 * At every generated position the candidates are what all processors leave for the row — the set the log-prob normalises over:
 * admissible text and admissible timestamps, the timestamps alone when the rule forces one, everything the masks leave with the
 * rules off; after sequence_bias, repetition_penalty, no_repeat_ngram_size, bad words, the suppress lists and the timestamp rules.
 * The k with the largest score come back in descending score, equal scores lowest id first (the arg-max's rule), each with
 * score - logsumexp over the same set.  Rank 0 is the id the pass emitted and its log-prob is bit for bit token_logprobs' value (a
 * step whose candidates are all -inf: id 0, -inf).  A rank with no finite candidate left holds id -1 and -inf, never NaN.
 * It runs on the device inside the captured step: the logits kernel also stores its processed rows, the step's arg-max launch
 * leaves each row's ranges and normaliser, and one selection launch behind it keeps the k best; a pass with top_k 0 launches
 * exactly what it did before.  0 = off (the default), 1..8; WM_E_ARG otherwise.
 *
 * wm_transcribe_top_k: the alternatives of the log-prob pass this slot collected last (slot 0: the synchronous entries), until the
 * slot's state runs another pass: top_ids, top_logprobs [B][n_prompt + 1 + max_loop][k] in the layout of tokens_out (for a
 * per-row-prompt pass: [B][prompt_stride + 1 + max_loop][k]), k the value the pass was asked for under.  Prompt positions and
 * positions past a row's n_tokens hold id -1 and log-prob 0.  WM_E_STATE: no such pass. */
int wm_set_top_k(wm_model* m, int top_k);
int wm_transcribe_top_k(wm_model* m, int slot, int32_t* top_ids, float* top_logprobs);

/* ---- phrase-list constraint ----------------------------------------------------------------------------------------
 * "The answer is one of these phrases": HF generate's prefix_allowed_tokens_fn (PrefixConstrainedLogitsProcessor) with the function
 * replaced by a trie of token ids, for every greedy pass asked for from now on — the passes wm_set_repeat_options names, with the
 * rules of wm_set_sequence_bias: model-wide, it persists until the next call, a held coalesce = 2 submit keeps its table and pairs
 * only with a submit made under the same one, and replacing the table changes no pass that was already asked for.
 * Phrase q is ids[offsets[q] .. offsets[q + 1]).  free_from: ids >= free_from (the timestamp ids, say) are always allowed and never
 * move a row through the trie; < 0 = none.  At every step, with gen the ids row b generated behind its own prompt:
 *   1. walk = gen without the ids >= free_from; node = where walk leads from the trie's root, or the dead node if it leaves the trie;
 *   2. allowed = the ids of the node's child edges, the pass's eot if a phrase ends at the node, and every id >= free_from (the dead
 *      node: the eot and the free ids) — never empty;
 *   3. every other id is -inf, where bad words act: behind sequence_bias, repetition_penalty and no_repeat_ngram_size, ahead of the
 *      suppress lists, the timestamp rules, the arg-max, the log-prob sums and the top-k selection.
 * The no-speech probe, language detection, wm_score and wm_align read unprocessed logits.  It runs on the device inside the captured
 * step: the step's arg-max launch moves the row's node and rewrites the row's ban set, which the logits kernel of the repetition
 * processors reads; a pass without a table launches exactly what it did before.  ids = NULL, n_phrases = 0 clears the table.
 * WM_E_ARG, with the setting unchanged: n_phrases = 0 with ids given, an empty phrase, an id outside the vocabulary or >= free_from,
 * a duplicate phrase, more than 4096 phrases, a phrase of more than 64 ids, more than 65536 trie nodes (root and dead node included),
 * offsets that do not start at 0.  A pass whose eot is an id of a phrase is refused with WM_E_ARG when it is asked for; the
 * long-form and chunked entries refuse to run while a table is set.
 *
 * wm_transcribe_constraint_match: for the B rows of the constrained pass this slot collected last (slot 0: the synchronous
 * entries), until the slot's state runs another pass: the index of the phrase that ended at the row's node when it emitted the eot
 * and stopped, -1 if it ended otherwise (the loop ran out, ignore_eot, the dead node, a node where no phrase ends).  WM_E_STATE: no
 * such pass. */
int wm_set_constraint(wm_model* m, const int32_t* ids, const int32_t* offsets, int n_phrases, int free_from);
int wm_transcribe_constraint_match(wm_model* m, int slot, int32_t* out, int B);

/* ---- sequence bias and bad words ---------------------------------------------------------------------------------
 * HF generate's sequence_bias (SequenceBiasLogitsProcessor) and bad_words_ids (NoBadWordsLogitsProcessor), given as ids, for every
 * greedy pass asked for from now on — the passes wm_set_repeat_options names, with the same rules: model-wide, it persists until the
 * next call, a submit held for a coalesce = 2 partner keeps the table in force when it was made and pairs only with a submit made
 * under the same table, and replacing the table changes no pass that was already asked for.
 * Sequence q of sequence_bias is ids[offsets[q] .. offsets[q + 1]) with bias[q]; bad word q is bad_ids[bad_offsets[q] ..
 * bad_offsets[q + 1]).  At every step, with hist the row's decoder ids so far and z its fp32 logits:
 *   1. a bias vector starts at 0; every length-1 sequence sets its id's entry; then, in the caller's order, every sequence s with
 *      2 <= len(s) <= len(hist) whose first len(s) - 1 ids are hist's last adds its bias to the entry of its last id (sequences that
 *      end in the same id are summed in that order, in fp32, as HF sums them); z += bias;
 *   2. repetition_penalty and no_repeat_ngram_size (wm_set_repeat_options) on the biased row;
 *   3. bad words: the same matching, -inf in place of the sum; a length-1 bad word equal to the pass's eot is dropped (HF's filter);
 *   4. the suppress masks, the timestamp rules, the arg-max and the log-prob sums see the processed row.
 * The no-speech probe, language detection, wm_score and wm_align read unprocessed logits; a long-form window's or a chunk's pass sees
 * that pass's decoder ids only.  It runs on the device inside the captured step: the step's arg-max launch matches every sequence
 * against the row's new history tail, the logits kernel reads the row's hits; a pass with both lists empty launches exactly what it
 * did before.  n_seq = n_bad = 0 switches it off (the default; the pointers may be NULL).
 * WM_E_ARG, with the setting unchanged: an id outside the vocabulary, a sequence of 0 or more than 32 ids, more than 1024 sequences
 * over the two lists, a duplicate sequence within a list, a bias that is NaN or +inf (-inf is allowed), offsets that do not start at 0. */
int wm_set_sequence_bias(wm_model* m, const int32_t* ids, const int32_t* offsets, const float* bias, int n_seq, const int32_t* bad_ids,
                         const int32_t* bad_offsets, int n_bad);

/* ---- token-level timestamps ---------------------------------------------------------------------------------
 * When each id was spoken, with the semantics of HF generate(..., return_token_timestamps=True)
 * (WhisperGenerationMixin._extract_token_timestamps, time_precision 0.02, median_filter_width 7, num_input_ids = n_prompt): the
 * cross-attention probabilities of a fixed set of alignment heads for the R = n_tokens[b] - n_prompt - 1 ids that were fed back,
 * cropped to the first n_frames[b] / 2 encoder positions (no renormalisation), z-scored over the rows (population std), median-filtered
 * (width 7, reflect) along the positions, averaged over the heads, then DTW against the positions.  token_times: host
 * [B, n_prompt + 1 + max_loop] fp32 in the layout of tokens_out: 0 for the prompt, the R jump times, the last id repeats the last one
 * (all 0 when R = 0).  Runs on the GPU after the greedy loop; a call without _tt enqueues exactly what it did before.
 *
 * wm_set_alignment_heads: (layer, head) pairs, HF generation_config.alignment_heads; at most 32, no duplicates; 0 pairs = off (the
 * default).  A _tt call on a model without alignment heads returns WM_E_STATE; n_frames[b] outside [2, 2·n_audio_ctx] WM_E_ARG.
 * n_frames NULL = the whole window.  The _tt submits pair under coalesce = 2 only with other _tt submits. */
int wm_set_alignment_heads(wm_model* m, const int32_t* layer_head_pairs, int n_pairs);
int wm_transcribe_tt(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts, const int32_t* n_frames,
                     int32_t* tokens_out, int32_t* n_tokens, float* token_times);
int wm_transcribe_submit_tt(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* opts,
                            const int32_t* n_frames);
/* WM_E_STATE when the slot's pass was submitted without timestamps */
int wm_transcribe_wait_tt(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_times);
/* n_frames[b] = min(2·n_audio_ctx, ceil(n_samples[b] / 160)): WhisperFeatureExtractor's attention mask */
int wm_transcribe_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                         int32_t* tokens_out, int32_t* n_tokens, float* token_times);
/* Diagnostics / tests: the alignment heads' probabilities of the slot's last completed _tt pass (slot 0 = wm_transcribe_tt),
 * out [B][n_sel][max_loop][n_audio_ctx] over ALL positions (before the crop); rows past R_b are 0.  WM_E_STATE once that pass's
 * state has run another pass. */
int wm_alignment_weights(wm_model* m, int slot, float* out);
/* Known-answer test of the normalisation + DTW stage: weights [n_sel][R][F] -> times [n_prompt + R + 1].  R <= 447. */
int wm_op_token_times(float* times, const float* weights, int n_sel, int R, int F, int n_prompt);

/* ---- forced alignment -----------------------------------------------------------------------------------------
 * When each id of a GIVEN transcript was spoken.  Rows, ids, context_len and pos_mode exactly as wm_score takes and validates them.
 * The decoder input of row b is y[0 .. len_b - 1); the cross-attention rows that count are the inputs t in [context_len[b], len_b - 1),
 * R_b = len_b - context_len[b] - 1 of them (0 is allowed); n_frames as the _tt calls (NULL = every column).  token_times: host
 * [B, ids_stride] fp32, what HF's _extract_token_timestamps gives for the cross-attentions of model(input_features,
 * decoder_input_ids = y[:, :-1]) with sequences = y and num_input_ids = context_len[b]: 0 for the context, the R_b jump times, the
 * last id repeats the last one, 0 past len_b.  Aligning the ids of a greedy _tt pass with context_len = its prompt length gives that
 * pass's own times.  token_logprobs / sum_logprob / avg_logprob: NULL as a group, or what wm_score writes for the same inputs, bit for
 * bit (the vocabulary side then runs as well).  State rules as wm_score: single-lane states, never coalesced, the slot's wait families
 * refuse each other's passes with WM_E_STATE (the pass stays pending).  WM_E_STATE without alignment heads; WM_E_ARG as wm_score and
 * as the _tt calls for n_frames; all before anything is launched.  wm_alignment_weights serves the slot's last align pass with
 * out [B][n_sel][L][n_audio_ctx], L = max_b R_b. */
int wm_align(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride,
             const int32_t* context_len, const int32_t* n_frames, float* token_times, float* token_logprobs, float* sum_logprob,
             float* avg_logprob);
int wm_align_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                    int ids_stride, const int32_t* context_len, const int32_t* n_frames, int want_logprobs);
/* token_logprobs non-NULL on a pass submitted with want_logprobs = 0: WM_E_STATE, the pass stays pending */
int wm_align_wait(wm_model* m, int slot, float* token_times, float* token_logprobs, float* sum_logprob, float* avg_logprob);
/* PCM in: front end + wm_align, n_frames[b] = min(2·n_audio_ctx, ceil(n_samples[b] / 160)) as wm_transcribe_pcm_tt */
int wm_align_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                 const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_times, float* token_logprobs,
                 float* sum_logprob, float* avg_logprob);
/* Diagnostics (tools/align_cost.py): ms[6] = wm_score_phases' five phases of the slot's last collected align pass (LayerNorm, sweep and
 * merge are 0 when it ran without log-probs) and [5] the align chain. */
int wm_align_phases(wm_model* m, int slot, float* ms);
/* Known-answer tests.  wm_op_dec_linear_capmap: LNx -> cross q with the capture by row map — B input rows, cap [cap_dst][cap_nsel][64]
 * in and out, cap_map [B] in [-1, cap_dst): row r's selected heads go to cap row cap_map[r], -1 stores nothing.
 * wm_op_token_times_rows: n_tab weight tables [n_tab][n_sel][L][T] (table b uses its R[b] x F[b] corner) through the normalisation and the
 * DTW in one launch each -> times [n_tab][out_stride], table b's times starting at id row0[b]. */
int wm_op_dec_linear_capmap(float* out, float* cap, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                            int B, int N, int K, int dtype, const int8_t* cap_sel, int cap_nsel, const int32_t* cap_map, int cap_dst);
int wm_op_token_times_rows(float* times, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F,
                           const int32_t* row0, int out_stride);
/* The align chain's first two stages alone.  wm_op_align_probs: the probabilities of n_sel (layer, head) pairs (layer_head_pairs
 * [n_sel][2]) over all T keys for the cross-q rows q [B][L][n_sel][64] (fp32, unscaled), utterance b's first rows[b] <= L rows.  Keys, one
 * of: kv, a host fp32 K/V cache [n_layers][2][B][T][d] (K halves read, V halves present as in the model) uploaded as kv_dtype (WM_F32 /
 * WM_BF16 / WM_F16), with X and Wk NULL; or the absorbed form, kv NULL, X [B][T][d] and Wk [n_layers][2][d][d] both uploaded as bf16,
 * K_h = X·Wk_hᵀ formed on the device.  probs [B][n_sel][L][T] in and out: rows >= rows[b] keep the caller's values.
 * wm_op_align_norm: wm_op_token_times_rows' tables through the normalisation only -> M [n_tab][L][T], in and out: cells outside table
 * b's R[b] x F[b] corner keep the caller's values.  Both refuse with WM_E_ARG before anything is launched. */
int wm_op_align_probs(float* probs, const float* q, const float* kv, int kv_dtype, const float* X, const float* Wk,
                      const int32_t* layer_head_pairs, int n_sel, const int32_t* rows, int B, int L, int T, int d, int n_layers);
int wm_op_align_norm(float* M, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F);

/* ---- log-mel front end --------------------------------------------------------------------------
 * Replaces the reference's call to HF WhisperProcessor (export_weights.py:100-116): 16 kHz mono PCM -> pad / trim to the
 * 30 s window -> 400-point Hann STFT (hop 160, reflect padding) -> 80 slaney mel bands -> log10 -> clamp to max-8 ->
 * (x+4)/4.  pcm: host [B, stride] fp32, n_samples[b] <= stride valid samples each.  mel_out: NULL or host
 * [B, n_mels, 2*n_audio_ctx] (the sample_input.bin layout the encoder takes). */
int wm_log_mel(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out);
/* PCM in, token ids out: front end + wm_transcribe without the mel ever leaving the GPU. */
int wm_transcribe_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                      int32_t* tokens_out, int32_t* n_tokens);

/* ---- sequential long-form transcription ------------------------------------------------------------------
 * Audio of any length, with the semantics of HF WhisperGenerationMixin.generate on its long-form path (greedy,
 * condition_on_prev_tokens, prompt_ids, logprob_threshold and no_speech_threshold through the _ex forms below, no temperature fallback,
 * no compression_ratio_threshold,
 * return_timestamps=True, return_segments=True): per utterance seek = 0; while seek < n_frames[b] the window
 * mel[:, seek : seek + min(n_frames[b] - seek, 2·n_audio_ctx)] zero-padded to 2·n_audio_ctx is decoded with opts (prompt as the
 * initial ids, timestamp rules from the first generated id), the trailing eot is dropped, the ids are split into segments at
 * timestamp pairs (HF _retrieve_segment, = wm_op_long_segments) and seek advances as HF's does.  The utterance's sequence is the
 * concatenation of its segments' ids.  One deliberate deviation: a window whose ids do not advance seek (e.g. <|0.00|><|0.00|>
 * and no later pair), on which HF and openai-whisper decode the same window forever, advances by its own length instead; its
 * segments are kept once and the window is counted (wm_long_result_stats).
 * Any B: utterances queue for rows of passes of R = min(max_batch, ceil(B / 2)) rows (spare rows repeat a real item), up to two
 * passes in flight on two internal decode states, never on the caller's slots 0..7.  An utterance is in at most one pass at a
 * time, so a single recording runs its windows one pass after another, and once one state runs out of ready utterances the
 * other's tail does too.  The two states (R rows each) stay allocated until the model is freed or B changes their size; the
 * long-form scratch that grows with the audio (PCM, long mel, windows) is released before each call returns.  WM_E_STATE while a coalesce = 2 submit is held.  WM_E_ARG: timestamp_begin <= 0,
 * ignore_eot != 0, n_frames[b] outside [0, T], n_prompt + 1 + max_loop > n_text_ctx.  An utterance of 0 frames has an empty
 * result.  The sequences assume eot is also generate's pad id. */
typedef struct wm_long_result wm_long_result;
typedef struct {
    int32_t first, count; /* the segment's ids are [first, first + count) of the utterance's sequence */
    double start, end;    /* seconds, float64 as HF computes them */
} wm_segment;
/* Log-mel of long audio, HF WhisperFeatureExtractor(truncation=False, padding="longest", return_attention_mask=True) with the
 * recordings zero-padded to `stride` samples (stride = the longest n_samples is HF's "longest"): F = stride / 160 frames, one
 * clamp max per utterance over its whole spectrogram.  pcm: host [B][stride]; n_samples[b] <= stride; stride > 200.  mel_out:
 * NULL or host [B][n_mels][F]; n_frames_out: NULL or [B], min(ceil(n_samples[b] / 160), F) (the ones of HF's attention mask).
 * The device copies of the PCM and the mel are released before the call returns. */
int wm_log_mel_long(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out, int32_t* n_frames_out);
/* mel: [B][n_mels][T] fp32, host or (mel_on_device) device; n_frames[b] frames of real audio in row b (NULL = T).
 * Word-level times on top of the segments: wm_transcribe_long_tt below. */
int wm_transcribe_long(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* opts,
                       wm_long_result** out);
/* wm_log_mel_long + wm_transcribe_long without the mel leaving the GPU */
int wm_transcribe_long_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                           wm_long_result** out);
/* Long-form with HF's condition_on_prev_tokens / prompt_ids / prompt_condition_type.  Every window's decoder prompt is
 * what HF's _prepare_decoder_input_ids builds for that utterance alone (= wm_op_long_prompt): with conditioning, <|startofprev|> (or,
 * all-segments, the whole prompt_ids) + the last n_text_ctx / 2 - 1 ids of the utterance's segments so far (a segment of more than
 * two ids that ends in a timestamp pair loses its last id) + opts->prompt; first-segment: prompt_ids without its leading
 * <|startofprev|> counts as a segment before the first window and never appears in the result; prompt_ids without conditioning:
 * prompt_ids + opts->prompt for every window.  Passes whose rows all carry opts->prompt run as wm_transcribe_long's do, the others as
 * per-row passes.  NULL / zero wm_long_opts = wm_transcribe_long.  Checked before the first window (WM_E_ARG): the longest possible
 * prompt + 1 + max_loop <= n_text_ctx, n_prompt_ids <= n_text_ctx / 2, ids in range, all-segments without conditioning. */
typedef struct {
    int condition_on_prev_tokens;   /* 0 / 1 */
    int prev_sot_token;             /* <|startofprev|> (50361); required when conditioning or prompt_ids are used */
    const int32_t* prompt_ids;      /* NULL / 0 = none; as WhisperProcessor.get_prompt_ids returns them */
    int n_prompt_ids;
    int prompt_condition_type;      /* 0 first-segment, 1 all-segments (needs condition_on_prev_tokens) */
    /* Thresholds (a zero tail keeps everything off).  When either use_* flag is set every pass of the run is a log-prob
     * pass (wm_transcribe_lp) and, unless no_speech_token is -1, carries the no-speech probe at the first of opts->prompt's
     * ids.  HF _need_fallback at the single temperature 0: a window is skipped iff avg_logprob < logprob_threshold and
     * no_speech_prob > no_speech_threshold; it then contributes no segments and no ids, seek advances by the window's own frame
     * count, and a conditioned prompt is built from the segments without it.  logprob_threshold alone changes no ids and only makes
     * the quality values available; with it alone no_speech_token may be -1 (no probe: no_speech_prob is reported as NaN).  WM_E_ARG
     * before anything is launched: use_no_speech_threshold without use_logprob_threshold (HF dereferences it) or without a vocabulary
     * id; with either flag, a no_speech_token that is neither -1 nor a vocabulary id. */
    int use_logprob_threshold;
    float logprob_threshold;
    int use_no_speech_threshold;
    float no_speech_threshold;
    int no_speech_token;
} wm_long_opts;
int wm_transcribe_long_ex(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* opts,
                          const wm_long_opts* lopts, wm_long_result** out);
int wm_transcribe_long_pcm_ex(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                              const wm_long_opts* lopts, wm_long_result** out);
/* Long-form with language detection: the arguments of the _ex pair plus the language list and lang_out [B].  HF detects
 * once per recording, on its first window: before the scheduler loop every recording's window at seek 0 is gathered, in groups of at
 * most the pass's rows, and run through wm_detect_language's device path (one extra encoder run over the first windows, as in HF);
 * the ids are read back once per group.  From then on recording b's initial ids are opts->prompt with the second id replaced by
 * lang_out[b], and every pass is a per-row-prompt pass.  Thresholds, prompt_ids and condition_on_prev_tokens work unchanged on top.
 * WM_E_ARG, nothing launched: what the _ex pair and wm_detect_language refuse; opts->n_prompt < 2; multi-lane decode states. */
int wm_transcribe_long_lang(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* opts,
                            const wm_long_opts* lopts, const int32_t* lang_ids, int n_lang, int32_t* lang_out, wm_long_result** out);
int wm_transcribe_long_pcm_lang(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                                const wm_long_opts* lopts, const int32_t* lang_ids, int n_lang, int32_t* lang_out, wm_long_result** out);
/* Long-form with token timestamps: the arguments of the _lang pair plus a flag; lang_ids NULL = no language detection
 * (lang_out is then not written).  token_timestamps != 0: every window pass also carries the alignment-head capture and the chain of
 * wm_transcribe_tt, with num_input_ids = the row's own decoder prompt length (previous text and prompt_ids included) and num_frames =
 * the window's real frames; an id's time is its window-relative fp32 time plus the window's time_offset, summed in float64.
 * wm_long_result_token_times then serves one time per id of the utterance's sequence.  One encoder run per window; no align pass.
 * WM_E_STATE: no alignment heads set.  WM_E_ARG: thresholds set in wm_long_opts together with the flag (log-probabilities and token
 * timestamps do not share a pass, as in wm_transcribe_lp; out of scope here).  token_timestamps = 0: exactly the _lang / _ex pair. */
int wm_transcribe_long_tt(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* opts,
                          const wm_long_opts* lopts, const int32_t* lang_ids, int n_lang, int32_t* lang_out, int token_timestamps,
                          wm_long_result** out);
int wm_transcribe_long_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* opts,
                              const wm_long_opts* lopts, const int32_t* lang_ids, int n_lang, int32_t* lang_out, int token_timestamps,
                              wm_long_result** out);
/* times: [n_tokens] seconds, parallel to wm_long_result_get's tokens (may be NULL when 0).  WM_E_STATE for a run without the flag. */
int wm_long_result_token_times(const wm_long_result* r, int b, double* times);
/* Host-only: one window's share of that array.  rel: the window-relative fp32 times of its n generated ids (eot already dropped),
 * segs: wm_op_long_segments' segments of those ids; times: room for n entries, one per id a segment keeps. */
int wm_op_long_token_times(const float* rel, int n, int64_t seek, const wm_segment* segs, int n_segs, double* times, int32_t* n_times);
/* Host-only, the counterpart of wm_op_long_segments: the decoder prompt of ONE utterance's next window.  seq / segs: the utterance's
 * segments so far (first, count into seq; n_segs may be 0); init: opts->prompt.  out: room for n_text_ctx ids. */
int wm_op_long_prompt(const int32_t* seq, const wm_segment* segs, int n_segs, const int32_t* init, int n_init, const wm_long_opts* lopts,
                      int timestamp_begin, int n_text_ctx, int32_t* out, int32_t* n_out);
int wm_long_result_sizes(const wm_long_result* r, int b, int32_t* n_tokens, int32_t* n_segments);
/* tokens: [n_tokens] (may be NULL when 0), segs: [n_segments] */
int wm_long_result_get(const wm_long_result* r, int b, int32_t* tokens, wm_segment* segs);
/* windows decoded in all, how many of them did not advance seek (the deviation above), passes run, and rows those passes decoded
 * (passes · R: rows - windows were spare rows) */
int wm_long_result_stats(const wm_long_result* r, int32_t* windows, int32_t* stalled, int32_t* passes, int32_t* rows);
/* the longest decoder prompt (ids) any pass of the run carried, and how many of its passes went out as per-row passes */
int wm_long_result_prompt_stats(const wm_long_result* r, int32_t* longest_prompt, int32_t* row_passes);
/* Thresholds only (WM_E_STATE for a run without): each segment's window values, openai-whisper's segment fields; [n_segments] */
int wm_long_result_quality(const wm_long_result* r, int b, float* seg_avg_logprob, float* seg_no_speech_prob);
/* Thresholds only: utterance b's window log in decode order, skipped windows included.  Call with NULL arrays for the count. */
int wm_long_result_windows(const wm_long_result* r, int b, int32_t* n_windows, int64_t* seek, float* avg_logprob, float* no_speech_prob,
                           int32_t* skipped);
/* windows the skip rule dropped (they are counted in wm_long_result_stats' windows) */
int wm_long_result_skip_stats(const wm_long_result* r, int32_t* skipped_windows);
void wm_long_result_free(wm_long_result* r);
/* Host-only: HF _retrieve_segment on one window's generated ids (eot already dropped).  segs: room for max(1, n) entries;
 * advance: the seek advance in frames exactly as HF computes it (0 in the zero-advance case). */
int wm_op_long_segments(const int32_t* ids, int n, int timestamp_begin, int64_t seek, int seek_num_frames, wm_segment* segs,
                        int32_t* n_segs, int32_t* advance);

/* ---- chunked long-form transcription ------------------------------------------------------------------------
 * HF's ASR pipeline with chunk_length_s / stride_length_s / batch_size: every recording is cut into overlapping chunks
 * (pipelines/automatic_speech_recognition.py::chunk_iter), every chunk is decoded on its own — its own 30 s log-mel with its own clamp
 * max, the decode options applying per chunk — in passes of up to max_batch rows that mix the chunks of all recordings, and each
 * recording's id lists are stitched on the device as tokenization_whisper._find_longest_common_sequence(sequences) stitches them
 * after _decode_asr's strip: every id >= first_special (50257 for the multilingual vocabulary: eot, language, task, timestamp ids) is
 * dropped, a chunk that keeps no id is no operand.  Unlike wm_transcribe_long, a single recording fills whole batches.
 *
 * wm_chunk_table (host only): HF's list of chunks for R recordings of n_samples[r] samples, one row of six ints per chunk in
 * recording order: (recording, start, len, stride_left_eff, stride_right_eff, is_last).  Step chunk_len - stride_left - stride_right;
 * the first chunk of a recording has left stride 0 and the last right stride 0; a chunk is kept only if len > stride_left_eff; the walk
 * ends at the first chunk with start + chunk_len >= n_samples[r].  table NULL (cap 0): only n_chunks is written.  WM_E_ARG: chunk_len
 * <= stride_left + stride_right (HF raises for <, and for = in range()), chunk_len > window when window > 0 (the model's window in
 * samples, 160 · 2 · n_audio_ctx); WM_E_SIZE: cap rows do not hold the table.
 *
 * wm_transcribe_chunked: pcm [R][stride] fp32 at 16 kHz, host or (pcm_on_device) device; n_samples[r] <= stride.  opts: as
 * wm_transcribe, applied to every chunk; lang_ids non-NULL: every pass is a wm_transcribe_submit_lang pass (n_init = opts->n_prompt,
 * the detected id sits in each chunk's ids); wm_set_repeat_options applies as always.  merged [R][cap], merged_len [R]: the stitched
 * ids; cap >= (most chunks of one recording) · (n_prompt + 1 + max_loop), else WM_E_SIZE.  chunk_ids [n_chunks][n_prompt + 1 +
 * max_loop] with chunk_n [n_chunks] (both or neither): every chunk's own ids, in table order, exactly what wm_transcribe_pcm of that
 * chunk's samples returns.  n_passes (or NULL): passes submitted.  Between the upload of the PCM and the download of the merged ids
 * only the chunk table and its recording offsets cross the bus: chunk_gather_kernel cuts the chunks on the device, each pass's ids go from its decode state
 * into one packed device table (wm_transcribe_wait_device's rows), chunk_merge_kernel reads that table.  Uses the caller's slots 0..1
 * (0..3 with coalesce = 2): WM_E_STATE while one of them holds a pass; a held coalesce submit is flushed first.  The scratch is
 * released before the call returns.  Timestamps in chunked mode: wm_transcribe_chunked_ts below.  Not here: HF's split at a language change. */
int wm_chunk_table(const int32_t* n_samples, int R, int chunk_len, int stride_left, int stride_right, int window, int32_t* table, int cap,
                   int32_t* n_chunks);
int wm_transcribe_chunked(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                          int stride_left, int stride_right, const wm_decode_opts* opts, const int32_t* lang_ids, int n_lang, int first_special,
                          int32_t* merged, int32_t* merged_len, int cap, int32_t* chunk_ids, int32_t* chunk_n, int32_t* n_passes);
/* Known-answer tests.  wm_op_chunk_gather: chunk_gather_kernel alone — out [n][N] (in and out: a cell the kernel does not store keeps
 * the caller's value) = pcm [R][T_max] cut at items [n][3] = (recording, start, len), zero-padded past len.  WM_E_ARG: an item that
 * leaves its recording or the row.
 * wm_op_chunk_merge: chunk_merge_kernel alone — ids [n_rows][stride] with lens [n_rows]; recording r owns rows [rec_off[r],
 * rec_off[r + 1]) (rec_off [n_rec + 1]); merged [n_rec][cap] (in and out), merged_len [n_rec].  stride <= 2048; cap must hold every
 * recording's ids.  One launch for all recordings. */
int wm_op_chunk_gather(float* out, const float* pcm, int R, int64_t T_max, const int32_t* items, int n, int N);
int wm_op_chunk_merge(int32_t* merged, int32_t* merged_len, const int32_t* ids, const int32_t* lens, const int32_t* rec_off, int n_rows,
                      int n_rec, int stride, int cap, int first_special);

/* ---- chunked long-form transcription with timestamps ----------------------------------------------------------
 * HF's ASR pipeline with chunk_length_s and return_timestamps = True (mode 1, segments) or "word" (mode 2): wm_transcribe_chunked's
 * arguments and passes, stitched by tokenization_whisper._decode_asr's state machine instead of the plain merge — each chunk's ids are
 * walked, timestamp ids inside a stride are skipped, a segment closes at an end timestamp, and the id lists a segment gathered over
 * several chunks are merged by _find_longest_common_sequence (mode 2: a position counts only when the ids are equal and the left
 * (start, end) pair <= the right pair).  Ids >= opts->timestamp_begin are timestamps, ids in [first_special, timestamp_begin) are
 * ignored, every other id is text.  time_precision: seconds per timestamp id, 0 = the model's (window seconds / n_audio_ctx);
 * segment_size is n_audio_ctx.  All times are float64, formed with Python's operations in Python's order and rounded as Python's
 * round(x, 2), on the device.
 * merged [R][cap], merged_len [R]: the segments' ids concatenated (cap as wm_transcribe_chunked).  n_seg [R]; seg_times [R][seg_cap][2]:
 * start and end in seconds, NaN for HF's None; seg_range [R][seg_cap][2]: [begin, end) in merged.  WM_E_SIZE when a recording has
 * more than seg_cap segments (n_seg holds the count; cap + 1 always suffices).  Mode 2: pairs [R][cap][2], the (start, end) of every
 * merged id; every pass carries the alignment-head capture with n_frames = chunk samples / 160 (the ragged form of
 * wm_transcribe_submit_tt) and its times are packed into one device table next to its ids, so nothing new crosses the bus between the
 * PCM upload and the results; chunk_times [n_chunks][n_prompt + 1 + max_loop] (or NULL; with chunk_ids): every chunk's token times
 * as wm_transcribe_wait_tt returns them.  WM_E_ARG: opts without the timestamp rule (timestamp_begin <= 0), mode 2 without alignment
 * heads, with lang_ids or with a chunk shorter than 320 samples, mode outside {1, 2}.  Not here: the language fields and HF's split at
 * a language change, _strip_prompt of a <|startofprev|> prompt, word grouping (host side: Tokenizer / tokenizer.collate_words).
 * wm_op_chunk_segments: chunk_segments_kernel alone (a known-answer test) — ids [n_rows][stride] with lens [n_rows], strides
 * [n_rows][3] = (len, stride_left, stride_right) in samples, times [n_rows][stride] aligned with the ids (mode 2) or NULL (mode 1);
 * the outputs as above, all in and out: a cell the kernel does not store keeps the caller's value.  WM_E_SIZE: cap below a recording's
 * ids (nothing is launched) or more segments than seg_cap (nothing is stored beyond it). */
int wm_transcribe_chunked_ts(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                             int stride_left, int stride_right, const wm_decode_opts* opts, const int32_t* lang_ids, int n_lang,
                             int first_special, int mode, double time_precision, int32_t* merged, int32_t* merged_len, int cap,
                             int32_t* n_seg, double* seg_times, int32_t* seg_range, int seg_cap, double* pairs, int32_t* chunk_ids,
                             int32_t* chunk_n, float* chunk_times, int32_t* n_passes);
int wm_op_chunk_segments(const int32_t* ids, const int32_t* lens, const int32_t* strides, const float* times, const int32_t* rec_off,
                         int n_rows, int n_rec, int stride, int first_special, int timestamp_begin, double time_precision, int segment_size,
                         int32_t* merged, int32_t* merged_len, int cap, int32_t* n_seg, double* seg_times, int32_t* seg_range, int seg_cap,
                         double* pairs);

/* ---- PCM at any sample rate and as int16: resampling to 16 kHz on the device -----------------------------------
 * Every audio entry above takes fp32 PCM at 16 kHz.  These turn rows of fp32 (WM_F32) or int16 (WM_I16, converted as x / 32768 in the
 * same kernel) PCM at sr_in into that, by band-limited sinc interpolation exactly as torchaudio.functional.resample(x, sr_in, 16000)
 * defines it with its defaults (lowpass_filter_width 6, rolloff 0.99, sinc_interp_hann).  With g = gcd(sr_in, 16000), orig = sr_in /
 * g, nw = 16000 / g, base = min(orig, nw) · 0.99, width = ceil(6 · orig / base):
 *   h[p][k] = sinc(t) · cos(pi t / 12)^2 · base / orig,  t = clamp((-p / nw + (k - width) / orig) · base, -6, 6),  0 <= p < nw,
 *   0 <= k < 2 · width + orig, computed in float64 and rounded once to fp32;  y[j] = sum_k h[j % nw][k] · x[(j / nw) · orig - width + k]
 *   with x zero outside the row, accumulated in fp32 in ascending k;  a row of n samples gives ceil(nw · n / orig).
 * sr_in = 16000 is the identity (orig = nw = 1, width = 0, one tap of 1).  A row's values depend on that row's samples alone.
 * WM_E_ARG, nothing launched: sr_in <= 0; orig or nw above 1024 (every common rate from 8 kHz to 192 kHz passes); in_dtype outside
 * {WM_F32, WM_I16}; n_in[b] outside [0, stride_in]; B above 65535.  WM_E_SIZE, nothing launched: stride_out below the longest row's output,
 * a row that resamples to 2^31 samples or more.
 *
 * wm_resample_len (host only): the output length of a row of n_in samples.
 * wm_resample_pcm: in [B][stride_in] on the host or (in_on_device) the model's device -> out [B][stride_out] fp32 on the host or
 * (out_on_device) the device, zero at and beyond n_out[b]; n_in and n_out [B] are host arrays.  Runs on the model's stream and returns
 * when the result is there.  The table of a rate is built on first use and kept in the model.  stride_out <= 2^31 - 1.
 * wm_op_resample (known-answer tests): resample_kernel alone on host rows; out is in and out — a cell at or beyond n_out[b] keeps the
 * caller's value; n_out is what the kernel wrote.
 * wm_op_resample_taps (host only): the table h [nw][2 · width + orig] into taps (cap floats; NULL with cap 0: only the three sizes);
 * WM_E_SIZE when cap does not hold it. */
enum { WM_I16 = 3 }; /* an input dtype of the resampling entries alone */
int wm_resample_len(int64_t n_in, int sr_in, int64_t* n_out);
int wm_resample_pcm(wm_model* m, const void* in, int in_dtype, int in_on_device, const int32_t* n_in, int B, int64_t stride_in, int sr_in,
                    float* out, int out_on_device, int64_t stride_out, int32_t* n_out);
int wm_op_resample(float* out, const void* in, int in_dtype, const int32_t* n_in, int B, int64_t stride_in, int sr_in, int64_t stride_out,
                   int32_t* n_out);
int wm_op_resample_taps(int sr_in, float* taps, int64_t cap, int* orig, int* nw, int* width);

/* ---- the log-mel front end one stage at a time (known-answer tests) ----------------------------------------------
 * Each hook launches its kernel through the launcher wm_log_mel / wm_log_mel_long use, on host arrays.  The DFT stage between frames
 * and mel_log is wm_op_matmul_nt(M, 512, 416, WM_F32) with the basis below as B: the same launcher and kernel.  WM_E_ARG, nothing
 * launched: a null pointer, a size outside the ranges given, an offset or an item that leaves its array.
 * wm_op_fe_tables (host only, no HIP call): the tables of a model with n_mels filters (1..128), computed in float64 and rounded once —
 *   window [400] the periodic Hann window; dft [512][416] the real-DFT basis, row k = cos(2 pi k n / 400), row 256 + k = -sin(...),
 *   k < 201, n < 400, every other entry 0; fb [201][n_mels] the slaney mel filters; band [n_mels][2] = [lo, hi), the bins outside which
 *   filter m is 0.
 * wm_op_fe_frames: frames_kernel — out [B][n][416] = the reflect-padded, windowed frames t0 .. t0 + n of pcm [B][N], columns 400..415
 *   zero.  N > 200, t0 + n <= N / 160.  n_samples [B] or NULL: given, zero_tails_kernel first zeroes pcm[b][n_samples[b]..N) as the
 *   runtime does after its upload.  out holds B * n + 1 rows and is in and out: the guard row keeps the caller's values.
 * wm_op_fe_mel_log: mel_log_kernel — spec [B][n][512] (re at k, im at 256 + k) -> logmel[b][m][t_out + t] = log10(max(sum_k fb[k][m]
 *   (re^2 + im^2), 1e-10)); logmel [B][n_mels][out_frames] is in and out, t_out + n <= out_frames: columns outside [t_out, t_out + n)
 *   keep the caller's values.
 * wm_op_fe_mel_norm: per row of n values y = (max(x, max(x) - 8) + 4) / 4.  long_mode 0: mel_norm_kernel; 1: the two-stage
 *   mel_max_partial_kernel + mel_norm_long_kernel of long audio.  logmel, out [B][n].
 * wm_op_window_gather: window_gather_kernel — out[r][m][t] = mel[b][m][seek + t] for t < len, 0 for len <= t < W, for items [rows][3]
 *   = (b, seek, len), len <= W, seek + len <= F.  mel [B][n_mels][F]; out [rows][n_mels][W], in and out. */
int wm_op_fe_tables(int n_mels, float* window, float* dft, float* fb, int32_t* band);
int wm_op_fe_frames(float* out, const float* pcm, const int32_t* n_samples, int B, int N, int n, int t0);
int wm_op_fe_mel_log(float* logmel, const float* spec, int B, int n, int n_mels, int out_frames, int t_out);
int wm_op_fe_mel_norm(float* out, const float* logmel, int B, int64_t n, int long_mode);
int wm_op_window_gather(float* out, const float* mel, const int32_t* items, int rows, int B, int n_mels, int F, int W);

/* ---- op-level entry points (host pointers; known-answer tests only) ------------------------------------------
 * Same argument meaning as the reference ops: out-param first, caller-allocated. */
/* matmul(C, A, B, bias)  whisper_tensor.mojo:151-246 : C[M,N] = A[M,K]·B[N,K]ᵀ (+bias[N], may be NULL).
 * dtype selects the operand rounding (WM_F32 exact).  Requires K % 32 == 0. */
int wm_op_matmul_nt(float* C, const float* A, const float* B, const float* bias, int M, int N, int K, int dtype);
/* C = layer_norm(A, ln_g, ln_b, 1e-5) · Bᵀ (+ bias): the LayerNorm -> projection pair of ResidualAttentionBlock.forward
 * (layers.mojo:449-455, 489-497) on the encoder's kernels.  require_fused != 0 demands the one-kernel form (the LayerNorm applied while
 * the GEMM loads its fp32 A rows; 16-bit dtypes, K = 384, N % 128 == 0, N <= 3072): any other shape is REFUSED by the kernel launcher —
 * WM_E_ARG, wm_last_error says why, nothing is launched and C is untouched.  require_fused == 0: fused where possible, else a
 * LayerNorm launch + a plain GEMM.  N % 128 == 0, K % 128 == 0, K <= 1024.  Known-answer and negative tests. */
int wm_op_ln_matmul_nt(float* C, const float* A, const float* ln_g, const float* ln_b, const float* B, const float* bias, int M, int N,
                       int K, int dtype, int require_fused);
/* layer_norm(out, inp, gamma, beta, eps)  whisper_tensor.mojo:249-285 (one-pass variance). cols % 128 == 0, <= 1024 */
int wm_op_layer_norm(float* out, const float* inp, const float* gamma, const float* beta, int rows, int cols,
                     float eps);
/* The LayerNorm launch of the base / small encoder as it is made before a projection: launch_layernorm_rows<dtype> storing the
 * operand-dtype rows (out_t, returned widened to fp32), the fp32 rows (out_f), or both from one launch.  Either of out_t / out_f may be
 * NULL, not both.  Both hold rows + 1 rows, in and out: the device buffers start from the caller's values (out_t's rounded to dtype),
 * so the guard row after the last comes back as it went in unless the kernel wrote it.  cols as wm_op_layer_norm.  Known-answer tests. */
int wm_op_layer_norm_t(float* out_t, float* out_f, const float* inp, const float* gamma, const float* beta, int rows, int cols,
                       float eps, int dtype);
/* One launch of the encoder's tiled GEMM kernels (gemm_nt_kernel, gemm_nt_lds_kernel) with every field of their shared epilogue:
 *   C[b][m][n] = act(Σ_k A[b·strideA + m·lda + k]·W[n][k] + bias[n]) + pos[m][n] + residual[b·strideR + m·ldr + n]
 * A: flat, a_len >= (batch-1)·strideA + (M-1)·lda + K elements (lda < K: overlapping rows, the implicit-GEMM conv form); W [N][K];
 * bias [N], pos [M][N], residual (r_len elements) may each be NULL.  residual_in_place != 0: the residual is C itself (fp32 output
 * only; residual must be NULL, ldr / strideR are taken from ldc / strideC).  act 0 / 1 (GELU, gelu_mode 0 tanh form, 1 erf).
 * group_n > 0: column n goes to C + (n / group_n)·group_stride + m·ldc + n % group_n (the cross-K/V scatter), group_n % 64 == 0.
 * dtype: operand rounding of A and W on upload; out_dtype: WM_F32 or dtype, 16-bit results are returned widened.
 * C (c_len elements, flat) is in and out: the device buffer starts from the caller's values rounded to out_dtype, so whatever the
 * kernel did not write (guard rows, gaps between batches or groups) comes back as it went in.
 * kernel_ran receives the WM_GEMM_NT_* answer of the launcher's own dispatch query.  WM_E_ARG with nothing launched and C untouched:
 * null / non-positive arguments, bad dtype / out_dtype, N % 128 or K % 32, lda / strideA not multiples of 8, ldc / strideC / ldr /
 * strideR / group_stride not multiples of 4, a bad group_n, residual_in_place without fp32 output, a size that overflows a_len /
 * c_len / r_len, or a shape that dispatches to the row-panel or full-row kernel.  Known-answer tests. */
enum { WM_GEMM_NT_REFUSED = -1, WM_GEMM_NT_DIRECT = 0, WM_GEMM_NT_LDS = 1, WM_GEMM_NT_ROWPANEL = 2, WM_GEMM_NT_FULLROW = 3 };
int wm_op_gemm_nt_epi(float* C, size_t c_len, const float* A, size_t a_len, const float* W, const float* bias, const float* pos,
                      const float* residual, size_t r_len, int M, int N, int K, int batch, long long lda, long long strideA,
                      long long ldc, long long strideC, long long ldr, long long strideR, int residual_in_place, int act, int gelu_mode,
                      int group_n, long long group_stride, int dtype, int out_dtype, int* kernel_ran);
/* wm_op_gemm_nt_epi for the shapes the launcher gives to the two ring kernels — gemm_nt_rowpanel_kernel (16-bit operands, K = 384,
 * N <= 3072, batch 1, no pos / residual) and gemm_nt_fullrow_kernel (16-bit operands, N = 384, K % 128 == 0, fp32 output) — with the
 * LayerNorms they carry.  Every argument of wm_op_gemm_nt_epi means the same here, and:
 *   ln_g, ln_b [K], both or neither: A holds the fp32 residual rows (not rounded to dtype) and the row-panel kernel multiplies
 *     round_dtype(LayerNorm(A row)·ln_g + ln_b).  Handed to the launcher as asked: a shape that cannot fuse is refused.
 *   lno_g, lno_b [N], lno_out (lno_len elements), all or none: the full-row kernel also writes round_dtype(LayerNorm(C row)·lno_g +
 *     lno_b) to lno_out, laid out like C (ldc, strideC).  lno_out is in and out like C: uploaded rounded to dtype, returned widened.
 * WM_E_ARG with nothing launched and C / lno_out untouched: whatever wm_op_gemm_nt_epi refuses (but the ring shapes), a shape that
 * dispatches to a tiled kernel, a LayerNorm the launcher refuses for the shape, ldc / strideC / group_stride not multiples of 8 where
 * 16-bit rows are written (16-bit output, lno_out), lno_len below the extent of C, (M-1)·lda + K >= 2^31.  Known-answer tests. */
int wm_op_gemm_nt_ring(float* C, size_t c_len, const float* A, size_t a_len, const float* W, const float* bias, const float* pos,
                       const float* residual, size_t r_len, int M, int N, int K, int batch, long long lda, long long strideA,
                       long long ldc, long long strideC, long long ldr, long long strideR, int residual_in_place, int act, int gelu_mode,
                       int group_n, long long group_stride, int dtype, int out_dtype, const float* ln_g, const float* ln_b,
                       const float* lno_g, const float* lno_b, float* lno_out, size_t lno_len, int* kernel_ran);
/* The q_len == 1 path of MultiHeadAttention.forward over cached keys / values (layers.mojo:186-272): per utterance and head
 * s_j = (q·K_j)·0.125 (scale AFTER the dot product), running max from -1e10, p = exp(s - max), o = Σ p_j V_j / Σ p_j.
 * q, out [B, 64·n_heads] fp32; k, v [B, t, 64·n_heads] fp32 host rows, rounded to kv_dtype as the cache holds them.
 * n_chunks > 1: the keys of an utterance are swept by n_chunks workgroups and merged (the cross-attention form; needs
 * t/512 <= n_chunks <= t/32 rounded up);  n_chunks == 1: one workgroup per utterance, the key count read from the decode
 * control block (the self-attention form).  out_dtype: element type of the kernels' output (the single-workgroup form's direct
 * store, the merge's store), returned widened to fp32.  len >= 0 (single-workgroup form): the control block's length — a row sweeps
 * len + 1 of the t cache rows (len < 0: t - 1, all of them).  q_B > 0: prefill rows, position-major (B = P·q_B; k, v hold q_B
 * utterances): row p·q_B + b attends over utterance b — len + 1 + p keys in the single-workgroup (causal) form, needs len + P <= t.
 * nq = 4 (chunked form, B = 4·q_B): one K/V sweep per (utterance, chunk) serves the four positions; else 0.  1 <= n_heads <= 16,
 * n_chunks <= 64.  Known-answer tests. */
int wm_op_attention_cached(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                           int n_chunks, int out_dtype, int q_B, int len, int nq);
/* wm_op_attention_cached's single-workgroup forms (n_chunks = 1, nq = 0) with a key window: utterance u sweeps the cache rows
 * [key_lo[u], len + 1 (+ p)) — key_lo [n_utt], 0 <= key_lo[u] <= t.  An empty window gives zeros.  key_lo = 0 is wm_op_attention_cached
 * bit for bit. */
int wm_op_attention_cached_lo(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                              int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* key_lo);
/* wm_op_attention_cached's chunked forms (n_chunks >= 2; nq = 0 or 4) with K/V by row map: k, v hold n_utt clips of t
 * rows, and the query row in batch slot b — of q_B slots, or of B when q_B == 0 — attends over clip utt_of[b] (0 <= utt_of[b] < n_utt,
 * else WM_E_ARG).  Equal bit for bit to wm_op_attention_cached on k[utt_of], v[utt_of]. */
int wm_op_attention_cached_map(float* out, const float* q, const float* k, const float* v, int B, int t, int n_heads, int kv_dtype,
                               int n_chunks, int out_dtype, int q_B, int len, int nq, const int32_t* utt_of, int n_utt);
/* One launch of the decode step's skinny linear, out[B, N] = epi(pro(x)[B, K]·W[N, K]ᵀ + bias), wired as a decode step wires its six
 * per-layer launches.  W is rounded to dtype on upload.  pro: ln_g / ln_b [K] non-NULL: LayerNorm (eps 1e-5) of the fp32 rows x;
 * x_is_t != 0 (no LayerNorm): x is uploaded in dtype, as the producer kernel leaves it.  epi: + bias [N] (or NULL); act != 0: GELU
 * (gelu_mode); + residual [B, N] (or NULL; residual == out: in place, out holds the residual on entry); out_is_t != 0 (no residual,
 * no cache): the kernel stores dtype, returned widened.
 * QKV mode (kcache, vcache non-NULL; N = 3·d): out is [B, d] (q); columns [d, 2d) / [2d, 3d) are appended to kcache / vcache
 * [n_utt][cap_rows][d] — uploaded in kv_dtype from the caller's values, returned after the launch — at row len of utterance r
 * (kv_B == 0, B <= n_utt), or, kv_B > 0 (prefill, B = P·kv_B position-major rows, len + P <= cap_rows), row len + r / kv_B of
 * utterance r % kv_B.
 * Capture (cap non-NULL, no cache; N = 64·heads): cap [B][cap_steps][cap_nsel][64], caller-initialised and returned; the 64 output
 * columns of every head h with cap_sel[h] >= 0 (cap_sel [32], values < cap_nsel) also go to cap[r][len - cap_step0][cap_sel[h]] when
 * 0 <= len - cap_step0 < cap_steps.
 * K must split over the kernel's waves (a multiple of 32, K/32 = waves·steps with waves <= 16, steps <= 4).  Known-answer tests. */
int wm_op_dec_linear(float* out, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                     const float* residual, int B, int N, int K, int dtype, int x_is_t, int out_is_t, int act, int gelu_mode,
                     float* kcache, float* vcache, int n_utt, int cap_rows, int kv_dtype, int kv_B, int len, float* cap,
                     const int8_t* cap_sel, int cap_step0, int cap_steps, int cap_nsel);
/* wm_op_dec_linear on the K-long form of the kernel, the one fc2 of d_model 768 / 1024 runs: 16 waves walking groups of k-steps into
 * the same accumulators.  Same arguments and results; K must be 3072 or 4096 and ln_g / ln_b NULL (the form has no LayerNorm
 * prologue).  K = 3072 gives wm_op_dec_linear's bits; K = 4096 is refused by wm_op_dec_linear and taken here.  Known-answer tests. */
int wm_op_dec_linear_long(float* out, const float* x, const float* W, const float* bias, const float* ln_g, const float* ln_b,
                          const float* residual, int B, int N, int K, int dtype, int x_is_t, int out_is_t, int act, int gelu_mode,
                          float* kcache, float* vcache, int n_utt, int cap_rows, int kv_dtype, int kv_B, int len, float* cap,
                          const int8_t* cap_sel, int cap_step0, int cap_steps, int cap_nsel);
/* The decode step's final LayerNorm + tied-embedding logits and fused argmax (whisper.mojo:156-166, whisper_tensor.mojo:431-439):
 * logits[B, N] = layer_norm(x, ln_g, ln_b, 1e-5)·emb[N, K]ᵀ on the decode step's logits kernel, emb rounded to dtype on upload (the
 * kernel variant follows from dtype, K and B as in a decode step), and ids[B] = the fused argmax of those logits (stage 1 in the
 * logits kernel, stage 2 the step's argmax) with the lowest-index rule; an all -inf candidate set gives id 0.  mask [N]: additive
 * 0 / -inf applied to the argmax candidates only, or NULL.  ranges [B][4] = (text_lo, text_hi, ts_lo, ts_hi), or NULL: with
 * 0 < timestamp_begin < N the timestamp decision is on — the best admissible text id in [text_lo, text_hi) unless
 * logsumexp of the admissible timestamps in [ts_lo, ts_hi) exceeds its logit, then the best admissible timestamp.
 * x [B, K] fp32, K in {128, 384, 512, 768, 1024}.  Known-answer tests. */
int wm_op_logits(float* logits, int32_t* ids, const float* x, const float* ln_g, const float* ln_b, const float* emb, const float* mask,
                 const int32_t* ranges, int timestamp_begin, int B, int N, int K, int dtype);
/* wm_op_logits on the log-prob instantiation of the same kernel variant, plus logprob[B] = logits[id] - logsumexp over the candidates
 * the processors leave (the rule of wm_transcribe_lp; all candidates -inf: id 0, logprob -inf).  logits and ids equal wm_op_logits's
 * bit for bit. */
int wm_op_logits_lp(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                    const float* mask, const int32_t* ranges, int timestamp_begin, int B, int N, int K, int dtype);
/* wm_op_logits / wm_op_logits_lp (logprob NULL / non-NULL) on the repetition-processor instantiation of the same kernel variant
 * (DESIGN §29), with given sets: seen, ban [B][ceil(N / 32)], id t = bit (t & 31) of word t >> 5.  Row b's logits at the ids of seen[b]
 * are multiplied (negative) or divided (else) by penalty, then those of ban[b] are -inf — before everything the mask, the ranges
 * and the log-prob sums do.  `logits` are the processed values. */
int wm_op_logits_processed(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                           const float* mask, const int32_t* ranges, int timestamp_begin, const uint32_t* seen, const uint32_t* ban,
                           float penalty, int B, int N, int K, int dtype);
/* wm_op_logits_lp with the top-k alternatives: the top-k instantiation of the arg-max launch and the selection launch
 * behind it, as a decode step runs them.  top_ids, top_lp [B][top_k], 1 <= top_k <= 8: the rule of wm_set_top_k on the row's
 * candidates (mask, ranges); rank 0 equals (ids, logprob).  seen / ban (both or NULL, with penalty): as wm_op_logits_processed. */
int wm_op_logits_topk(float* logits, int32_t* ids, float* logprob, int32_t* top_ids, float* top_lp, int top_k, const float* x,
                      const float* ln_g, const float* ln_b, const float* emb, const float* mask, const int32_t* ranges, int timestamp_begin,
                      const uint32_t* seen, const uint32_t* ban, float penalty, int B, int N, int K, int dtype);
/* The sets' bookkeeping alone: the init kernel on each row's prompt tokens[b][0 .. prompt_len[b]), then `steps` argmax launches, step
 * s appending tokens[b][prompt_len[b] + s - 1] (a row past n_ids[b] has ended and does nothing).  seen, ban: host
 * [steps + 1][B][ceil(vocab / 32)] — entry 0 after the init, entry s after step s.  1 <= prompt_len[b] <= n_ids[b] <= stride. */
int wm_op_repeat_sets(uint32_t* seen, uint32_t* ban, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B, int stride,
                      int vocab, int ngram, int steps);
/* wm_op_logits_processed on the sequence-bias instantiation of the same kernel variant, with given hit state: hit
 * [B][ceil(N / 32)] (id t = bit (t & 31) of word t >> 5), the slots' ids slot_id [n_slots] (ascending, 1 <= n_slots <= 1024) and per
 * row and slot the summed bias slot_bias [B][n_slots] and slot_flags [B][n_slots] (bit 0: on, bit 1: a ban).  Where row b's bit of id t
 * is set, t's slot adds its bias before the penalty, or makes the value -inf when it carries a ban. */
int wm_op_logits_seq_bias(float* logits, int32_t* ids, float* logprob, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                          const float* mask, const int32_t* ranges, int timestamp_begin, const uint32_t* seen, const uint32_t* ban, float penalty,
                          const uint32_t* hit, const int32_t* slot_id, int n_slots, const float* slot_bias, const int32_t* slot_flags, int B,
                          int N, int K, int dtype);
/* The hit state's bookkeeping alone, as wm_op_repeat_sets runs the sets': the table is built from the two lists as
 * wm_set_sequence_bias builds it (same refusals), the init kernel runs on each row's prompt, then `steps` argmax launches append the
 * rows' ids.  Out: slot_id [n_seq + n_bad] and *n_slots (one slot per distinct last id, ascending); hit [steps + 1][B][ceil(vocab /
 * 32)]; slot_bias, slot_flags [steps + 1][B][n_seq + n_bad], the first *n_slots of each row written — entry 0 after the init, entry s
 * after step s.  eot: the id whose length-1 bad word is dropped, -1 = none. */
int wm_op_seq_bias_hits(uint32_t* hit, float* slot_bias, int32_t* slot_flags, int32_t* slot_id, int32_t* n_slots, const int32_t* tokens,
                        const int32_t* prompt_len, const int32_t* n_ids, int B, int stride, int vocab, int eot, const int32_t* seq_ids,
                        const int32_t* seq_off, const float* seq_bias, int n_seq, const int32_t* bad_ids, const int32_t* bad_off, int n_bad,
                        int steps);
/* The phrase-list constraint's bookkeeping alone, replayed likewise: the table is built from the phrases as
 * wm_set_constraint builds it (same refusals; eot: allowed where a phrase ends, refused inside a phrase), the init kernels run on each
 * row's prompt with no_repeat_ngram_size = ngram, then `steps` argmax launches append the rows' ids.  Out: node [steps + 1][B], the
 * rows' trie nodes (the root is 0, nodes are numbered as the phrases first reach them, the dead node is the last), and mask
 * [steps + 1][B][ceil(vocab / 32)], the rows' ban words: the complement of the node's allowed set with the n-gram bans on top, bits
 * past the vocabulary clear — entry 0 after the init, entry s after step s. */
int wm_op_constraint_states(int32_t* node, uint32_t* mask, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B,
                            int stride, int vocab, int eot, int ngram, const int32_t* ids, const int32_t* offsets, int n_phrases, int free_from,
                            int steps);
/* The timestamp rules' state machine alone, replayed likewise.  Launches: the pass's real init (row_prompts == 0:
 * launch_init_tokens on the prompt tokens[0][0 .. prompt_len[0]) that every row must share, at most 16 ids; else
 * launch_init_tokens_rows on the ragged rows with Lmax = max prompt_len), launch_set_step / launch_set_rows_step (cache length Lmax,
 * row positions), then `steps` launch_argmax_step with the rules on and `advance` set, step s handed tokens[b][prompt_len[b] + s - 1]
 * as its only candidate (a text id as the text partial, a timestamp id as the timestamp partial), so the kernel's own decision picks
 * it.  Out: states [steps + 1][B][8], each a TsState (n_gen, last_ts, pen_ts, t_last, text_lo, text_hi, ts_lo, ts_hi) — entry 0 after
 * the init, entry s after step s; a row's entries count up to its own end n_ids[b] only (behind it the kernel moves the state of the
 * finished row on as for id 0).  picks [steps][B]: the launches' `next`.  out_tokens [B][stride], n_tokens [B], pos [B], ctl [4]
 * (len, n_finished, 2 pad words): the final values.  key_lo [B], tok_rows, pos_rows [Lmax][B]: with row_prompts, else NULL.
 * WM_E_ARG, nothing launched: timestamp_begin <= 0 or >= vocab, eos outside [0, timestamp_begin], a bad row table (the rule of
 * wm_op_repeat_sets), rows of a shared prompt that differ.  max_initial < 0: none. */
int wm_op_ts_states(int32_t* states, int32_t* picks, int32_t* out_tokens, int32_t* n_tokens, int32_t* pos, int32_t* ctl, int32_t* key_lo,
                    int32_t* tok_rows, int32_t* pos_rows, const int32_t* tokens, const int32_t* prompt_len, const int32_t* n_ids, int B, int stride,
                    int vocab, int timestamp_begin, int eos, int max_initial, int steps, int row_prompts);
/* The pass-control and data-movement kernels, one launch each, exactly the runtime's.  Every output array is in and out:
 * it goes to the device with the caller's values and comes back whole, so a sentinel shows what the kernel left alone.  Arrays with
 * B_held (rows_held) rows hold that many rows while the launch covers B (rows_cap): the rest is the guard.
 *
 * wm_op_init_tokens: launch_init_tokens (len NULL: prompt [n_prompt], 1 .. 16 ids) or launch_init_tokens_rows (prompt [B][row_stride],
 * len [B] in [1, Lmax]).  out_tokens [B_held][out_stride], n_tokens, finished [B_held], ctl [4]; optional (NULL = the kernel gets a
 * null pointer): tok_rows + pos_rows [rows_held][B] (required with len), ts_state [B_held][8] (with vocab, timestamp_begin, eos,
 * max_initial as wm_op_ts_states), logprobs [B_held][out_stride] + lp_sum [B_held], key_lo [B_held] (with len only). */
int wm_op_init_tokens(int32_t* out_tokens, int32_t* n_tokens, int32_t* finished, int32_t* ctl, int32_t* tok_rows, int32_t* pos_rows,
                      int32_t* ts_state, float* logprobs, float* lp_sum, int32_t* key_lo, const int32_t* prompt, int n_prompt, const int32_t* len,
                      int row_stride, int Lmax, int rows_held, int B, int B_held, int out_stride, int vocab, int timestamp_begin, int eos,
                      int max_initial);
/* launch_set_rows_step: ctl->len = Lmax, pos[b] = len[b] + pos_delta.  ctl [4], pos [B_held], len [B]. */
int wm_op_set_rows_step(int32_t* ctl, int32_t* pos, const int32_t* len, int Lmax, int pos_delta, int B, int B_held);
/* launch_set_step: pos[b] = pos_value and tok[b] = tok_value where the array is given, ctl->len = len when set_len != 0. */
int wm_op_set_step(int32_t* ctl, int32_t* pos, int32_t* tok, int len, int set_len, int pos_value, int tok_value, int B, int B_held);
/* launch_pack_tokens over rows_cap rows: dst[r] = [n, ids zero-padded to stride] with n = min(n_tokens[r], stride) for r < rows, zeros
 * for rows <= r < rows_cap.  dst [rows_held][1 + stride], out_tokens [rows][out_stride], n_tokens [rows]. */
int wm_op_pack_tokens(int32_t* dst, const int32_t* out_tokens, const int32_t* n_tokens, int out_stride, int rows, int rows_cap, int rows_held,
                      int stride);
/* launch_dec_embed: x[b] = tok_emb[tok[b]] + pos_emb[pos[b]] in fp32.  x [B_held][d], tok_emb [vocab][d], pos_emb [n_pos][d]; an id or
 * a position outside its table is WM_E_ARG. */
int wm_op_dec_embed(float* x, const float* tok_emb, const float* pos_emb, const int32_t* tok, const int32_t* pos, int B, int B_held, int d,
                    int vocab, int n_pos);
/* The two row copies.  dst NULL: launch_no_speech_capture, out[r] = rows[r] for r < n_rows; else launch_score_collect, out[dst[r]] =
 * rows[r] where dst[r] >= 0 (dst [n_rows] in [-1, out_rows), else WM_E_ARG).  out [out_rows][d], rows [n_rows][d], d % 4 == 0. */
int wm_op_rows_copy(float* out, const float* rows, const int32_t* dst, int n_rows, int out_rows, int d);
/* launch_mel_transpose_pad on B clips: mel [B][C][L] fp32 -> image [B_held][L + 2][Cp] in dtype (Cp = C rounded up to 32), rounded to
 * dtype on upload and widened on return: row t + 1 = frame t, rows 0 and L + 1 and channels >= C zero, clips behind B untouched. */
int wm_op_mel_transpose_pad(float* image, const float* mel, int B, int B_held, int C, int L, int dtype);
/* The no-speech probe's launches on the kernel variant wm_op_logits_lp picks for (dtype, K, B): prob[b] = softmax(LN(x[b])·embᵀ)[token]
 * over all N columns, lse[b] the row's logsumexp.  prob, lse: [B]. */
int wm_op_no_speech(float* prob, float* lse, const float* x, const float* ln_g, const float* ln_b, const float* emb, int B, int N, int K,
                    int dtype, int token);
/* lang_detect_kernel alone: lang_out[b] = the id among lang_ids with the largest LN(x[b])·emb[id] (ties: the smaller id),
 * probs[b][i] = the softmax over the n_lang candidates at list position i.  emb [N][K] is rounded to dtype on upload.
 * 1 <= n_lang <= 128, ids distinct and inside [0, N), K 128, 384 or 512.  probs may be NULL. */
int wm_op_lang_detect(int32_t* lang_out, float* probs, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                      const int32_t* lang_ids, int n_lang, int B, int N, int K, int dtype);
/* The score pass's vocabulary side alone: the final LayerNorm once per row into the sweep's operand form, the MFMA-tiled
 * sweep with the fused log-sum-exp / target gather / arg-max, and the merge.  With z = layer_norm(x, ln_g, ln_b, 1e-5)·emb[N, K]ᵀ (emb
 * rounded to dtype on upload; the arithmetic class per dtype and K is wm_op_logits's): logprob[r] = z[r][target[r]] - logsumexp_j z[r][j]
 * and top_id[r] = argmax_j z[r][j], lowest id on ties.  target[r] < 0: the row is not scored — logprob[r] = 0, top_id[r] is still
 * written; target[r] >= N: WM_E_ARG.  x [M, K] fp32, K in {128, 384, 512, 768, 1024}; logprob, top_id, target: [M].  Known-answer tests. */
int wm_op_score_logits(float* logprob, int32_t* top_id, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                       const int32_t* target, int M, int N, int K, int dtype);
/* The absorbed cross-attention of bf16-encoder / fp32-K/V models: per row r and head h, with X = x[utt(r)] and
 * utt(r) = r % q_B when q_B > 0 (prefill rows, position-major; rows = P·q_B) else r,
 *   out[r, h] = Σ_j softmax_j(0.125·q_h[r]·(Wk_h X_j)) (Wv_h X_j) + bv_h,
 * computed as the decode step does: q' = 0.125·q_h·Wk_h once per row, the X sweep in nsplit key chunks, merge + Wv apply.
 * q [rows, 64·n_heads] and bv [64·n_heads] fp32; Wk, Wv [64·n_heads, 64·n_heads] and x [n_utt, n_keys, 64·n_heads] rounded to bf16
 * on upload.  out [rows, 64·n_heads] in out_dtype WM_F32 or WM_BF16, returned widened to fp32.  1 <= n_heads <= 8,
 * 1 <= nsplit <= 64 (chunks of ceil(n_keys / nsplit) keys; trailing chunks may be empty).  Known-answer tests. */
int wm_op_xattn(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* x, int rows, int q_B,
                int n_utt, int n_keys, int n_heads, int nsplit, int out_dtype);
/* wm_op_xattn with X by row map: utt(r) = utt_of[r % q_B] when q_B > 0 else utt_of[r]; utt_of holds q_B (or rows) entries
 * of [0, n_utt), else WM_E_ARG; any number of rows may share a clip.  Equal bit for bit to wm_op_xattn on x[utt_of]. */
int wm_op_xattn_map(float* out, const float* q, const float* Wk, const float* Wv, const float* bv, const float* x, int rows, int q_B,
                    int n_utt, int n_keys, int n_heads, int nsplit, int out_dtype, const int32_t* utt_of);
/* The n-best ranking launch alone: key [R = sum n_cand] fp32 grouped by clip, n_cand [U] >= 1; order, posterior [R] and
 * best [U] as wm_score_nbest defines them.  A non-finite key is refused with WM_E_ARG (NaN keys have no rank).  Known-answer tests. */
int wm_op_score_rank(int32_t* order, int32_t* best, float* posterior, const float* key, const int32_t* n_cand, int U);
/* The first launch of wm_op_xattn alone: q'[r, h] = (0.125·q_h[r])·Wk_h as the X sweep reads it, three bf16 images whose sum is the
 * fp32 product (x = hi + mid + lo by truncation).  images [rows, 3, n_heads, 64·n_heads], widened to fp32; q [rows, 64·n_heads] fp32;
 * Wk [64·n_heads, 64·n_heads] rounded to bf16 on upload.  late_loads != 0: the loop that requests its Wk rows after q is staged
 * (the default requests all of them first); the images are equal bit for bit.  1 <= n_heads <= 8.  Known-answer tests. */
int wm_op_xattn_absorb(float* images, const float* q, const float* Wk, int rows, int n_heads, int late_loads);
/* The MLP half of ResidualAttentionBlock.forward  layers.mojo:489-517 :  x += fc2(gelu(fc1(layer_norm(x, ln_g, ln_b)))),
 * x [M, d] in place; fc1_w [ffn, d], fc2_w [d, ffn] (HF [out, in]).  With next_g / next_b / xn_out non-NULL also returns
 * layer_norm(x_new, next_g, next_b) rounded to the operand dtype (what the next projection is fed) in xn_out [M, d].
 * Runs on the encoder's own kernels: for 16-bit dtypes with d = 384 the LayerNorm rides the fc1 GEMM's A load, and the residual
 * add and the next LayerNorm ride fc2's epilogue.  d % 128 == 0, ffn % 128 == 0. */
int wm_op_mlp_block(float* x, const float* ln_g, const float* ln_b, const float* fc1_w, const float* fc1_b, const float* fc2_w,
                    const float* fc2_b, const float* next_g, const float* next_b, float* xn_out, int M, int d, int ffn, int dtype,
                    int gelu_mode);
/* The block attention path of MultiHeadAttention.forward without cache and without mask (the encoder's: layers.mojo:273-342:
 * per head gather, S = q_h·k_hᵀ, scale 1/8 after the product, row softmax, O = S·v_h, scatter).  q, k, v, out [n_ctx, 64·n_heads]
 * fp32 host rows; dtype = operand rounding of q, k, v and of the probabilities (WM_F32: exact).  Runs the encoder's fused
 * attention kernel (never materialises S).  Known-answer tests. */
int wm_op_attention(float* out, const float* q, const float* k, const float* v, int n_ctx, int n_heads, int dtype);
/* wm_op_attention over B utterances in ONE launch, as an encoder pass makes it: q, k, v, out [B, n_ctx, 64·n_heads].  B = 1 is
 * wm_op_attention.  B <= 0, n_heads outside 1..64 or a bad dtype: WM_E_ARG, nothing launched, out untouched. */
int wm_op_attention_batch(float* out, const float* q, const float* k, const float* v, int B, int n_ctx, int n_heads, int dtype);
/* gelu(t) in place  whisper_tensor.mojo:288-308 (mode WM_GELU_TANH) */
int wm_op_gelu(float* t, size_t n, int mode);
/* softmax(t) rows in place  whisper_tensor.mojo:311-355 */
int wm_op_softmax_rows(float* t, int rows, int cols);
/* conv1d(out, inp, weight, bias, stride, padding, out_T)  whisper_tensor.mojo:367-428; K=3, padding=1.
 * inp [C_in, L_in]; weight in the ORIGINAL [C_out, C_in, 3] file layout (the transpose of
 * whisper_tensor.mojo:358-364 is internal); out [C_out, L_out] or [L_out, C_out] when out_T. */
int wm_op_conv1d_k3(float* out, const float* inp, const float* weight, const float* bias, int C_in, int L_in,
                    int C_out, int stride, int out_T, int dtype);
/* argmax(t)  whisper_tensor.mojo:431-439 */
int wm_op_argmax(const float* t, int n, int32_t* idx);

/* ---- measurement helpers (bench.py) ----------------------------------------------------------------------------- */
enum { WM_KERNEL_CROSS_ATTN = 0, WM_KERNEL_DECODE_STEP = 1, WM_KERNEL_ENCODER = 2,
       WM_KERNEL_DECODE_STEP_SHARED = 3 /* the step as wm_transcribe_submit's passes run it: K/V stream at two workgroups per CU */ };
/* Launches `reps` instances of the named kernel / stage on the library's stream between two HIP events and
 * returns the average duration in microseconds.  State must have been encoded (cross K/V present). */
int wm_bench_kernel(wm_model* m, wm_state* s, int which, int reps, float* avg_us);
/* Algorithmic HBM bytes one launch of `which` moves for state `s` (SURVEY §8d formulas). */
int wm_bench_bytes(wm_model* m, wm_state* s, int which, double* bytes);

/* Synthetic weights / mels (include/wm_synth.h) exported for hosts that cannot include the header. */
size_t wm_synth_weights(const wm_dims* dims, uint64_t seed, float* out);
void wm_synth_mel_host(uint64_t seed, int n_mels, int n_frames, float* out);

#ifdef __cplusplus
}
#endif
#endif
