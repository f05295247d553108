// wm_kernels.h — launcher declarations shared by the kernel translation units and the C-ABI host code.
#pragma once
#include "wm_device.h"

#include <atomic>
#include <cstdlib>

// Developer switches (A/B knobs, timelines, debug chains) exist only in the -DWM_DEV build (libwhispermi_dev.so, built by
// `python whisper.mojo_amd/build.py --dev`).  In the product library wm_env() is a constant nullptr, so every switch folds
// to its measured-best default at compile time and no launch path reads the environment.
#ifdef WM_DEV
static inline const char* wm_env(const char* name) { return std::getenv(name); }
#else
static constexpr const char* wm_env(const char*) { return nullptr; }
#endif

namespace wm {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property of ONE kernel: the record is keyed on the kernel itself
// (a non-type template parameter — keyed on the function TYPE, every instantiation of a kernel template with the same signature
// shared one flag) and holds, per device, the largest byte count set so far.  Returns the HIP status.
template <auto Kernel> static inline hipError_t ensure_dyn_lds(int bytes) {
    static std::atomic<int> set_bytes[64];  // zero-initialised; index = device
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::atomic<int>& have = set_bytes[dev & 63];
    if (have.load(std::memory_order_acquire) >= bytes) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess) {
        int cur = have.load(std::memory_order_relaxed);
        while (cur < bytes && !have.compare_exchange_weak(cur, bytes, std::memory_order_release)) {
        }
    }
    return e;
}

// Launcher status: a launcher that cannot serve a shape REFUSES it (nothing is launched) and says so; the C-ABI entry above turns
// that into WM_E_ARG with wm_last_error set.  0 = launched.
enum { WM_LAUNCH_OK = 0, WM_LAUNCH_BAD_SHAPE = 1, WM_LAUNCH_HIP = 2 };
// message of the last refusal on this thread (static text)
const char* launch_last_refusal();
int launch_refuse(const char* why);  // records `why`, returns WM_LAUNCH_BAD_SHAPE
int launch_hip_failed(const char* what, hipError_t e);

// Per-state decode control block, resident in HBM so that a captured decode step can be replayed unchanged.
struct StepCtl {
    int len;         // LayerCache.current_len BEFORE this step (= cache row the new K/V is written to)
    int n_finished;  // utterances that have emitted eot
    int pad0, pad1;
};

// ---- encoder ------------------------------------------------------------------------------------------------
struct GemmParams {
    const void* A;
    const void* W;
    void* C;
    int M, N, K;  // per batch
    long lda, ldw, ldc;
    long strideA, strideC;  // per-batch element strides (grid.z)
    const float* bias;      // [N] or null
    const float* residual;  // fp32, indexed [m*ldr + n] (+ z*strideR), or null
    long ldr, strideR;
    const float* pos;  // fp32 [M][N] added after the activation (conv2 + pos_emb, whisper.mojo:83-89), or null
    int act;           // 0 none, 1 gelu
    int gelu_mode;
    int group_n;  // >0: column n goes to C + (n/group_n)*group_stride + m*ldc + n%group_n  (cross-K/V scatter)
    long group_stride;
    int xcd_remap;  // set by the launcher (LDS-staged kernel only)
    // LayerNorm fused into the A load (row-panel kernel only — ask gemm_nt_fuses_layernorm first): A is then the fp32 residual
    // stream [M][lda] and the operand is LN(A) * ln_g + ln_b rounded to T, exactly what layernorm_rows + a plain GEMM compute
    const float* ln_g;
    const float* ln_b;
    // LayerNorm of the OUTPUT rows fused into the epilogue (full-row kernel only — ask gemm_nt_fuses_layernorm_out first): besides
    // C the kernel writes LN(C) * lno_g + lno_b as 16-bit operands to lno_out, laid out like C (ldc, strideC): the next GEMM's A
    const float* lno_g;
    const float* lno_b;
    void* lno_out;
    long long* dbg;  // developer build: phase stamps of the row-panel kernel (wm_bench_kernel id 43), else null
};
bool gemm_nt_fuses_layernorm_out(int operand_bytes, const GemmParams& p);
// true when launch_gemm_nt<T, *> takes the A-stationary row-panel kernel for these parameters (the only one that can fuse a LayerNorm)
bool gemm_nt_fuses_layernorm(int operand_bytes, const GemmParams& p, int batch);
// the kernel launch_gemm_nt<T, TO> runs for (sizeof T, sizeof TO, p, batch): the launcher dispatches on this very function.  why (may be
// null) receives the refusal text.  The values are include/whisper_mi.h's WM_GEMM_NT_*.
enum { GEMM_NT_REFUSED = -1, GEMM_NT_DIRECT = 0, GEMM_NT_LDS = 1, GEMM_NT_ROWPANEL = 2, GEMM_NT_FULLROW = 3 };
int gemm_nt_kernel_for(int operand_bytes, int out_bytes, const GemmParams& p, int batch, const char** why);
template <typename T> void launch_mel_transpose_pad(const float* mel, void* out, int B, int C, int L, int Cp, hipStream_t st);
template <typename T, typename TO> int launch_gemm_nt(const GemmParams& p, int batch, hipStream_t st);  // WM_LAUNCH_*
template <typename T>
void launch_layernorm_rows(const float* x, const float* gamma, const float* beta, void* out_t, float* out_f, int rows,
                           int cols, float eps, hipStream_t st);
template <typename T> void launch_flash_attn_enc(const void* qkv, void* out, int B, int H, int n_ctx, float scale, hipStream_t st);

// ---- decoder ------------------------------------------------------------------------------------------------
// Timestamp rules of the fused argmax (semantics of HF's WhisperTimeStampLogitsProcessor, absent from the
// reference).  Per utterance: what the rules need of the history, and the id ranges the NEXT argmax may choose from — written
// by stage 2 of one step (argmax_step), read by stage 1 of the next (dec_logits).
struct TsState {
    int n_gen;    // ids generated so far (after the prompt)
    int last_ts;  // the last one was a timestamp
    int pen_ts;   // the one before was a timestamp (or there is none)
    int t_last;   // the latest timestamp id emitted, -1 = none
    int text_lo, text_hi;  // admissible "text" ids (everything below timestamp_begin): [text_lo, text_hi)
    int ts_lo, ts_hi;      // admissible timestamp ids: [ts_lo, ts_hi)
};
struct TsRules {
    int tb;        // timestamp_begin: first timestamp id (<|0.00|>); <= 0 = rules off
    int eos;       // ids below it are "normal text" (masked after the first timestamp of a pair)
    int max_init;  // max_initial_timestamp_index, < 0 = none
    int vocab;
};
__host__ __device__ inline void ts_next_ranges(TsState& st, const TsRules& r) {  // ranges for the next argmax from the history
    st.text_lo = 0;
    st.text_hi = r.tb;
    st.ts_lo = r.tb;
    st.ts_hi = r.vocab;
    if (st.n_gen == 0) {  // the first id is a timestamp, at most <|max_init * 0.02|>
        st.text_hi = 0;
        if (r.max_init >= 0 && r.tb + r.max_init + 1 < st.ts_hi) st.ts_hi = r.tb + r.max_init + 1;
        return;
    }
    if (st.last_ts) {
        if (st.pen_ts)
            st.ts_hi = st.ts_lo;  // two in a row: the next one is not a timestamp
        else
            st.text_lo = r.eos;  // first of a pair: no normal text
    }
    if (st.t_last >= 0) {  // never decrease; do not re-emit a closed pair's value
        const int ts_end = (st.last_ts && !st.pen_ts) ? st.t_last : st.t_last + 1;
        if (ts_end > st.ts_lo) st.ts_lo = ts_end;
    }
}

// Repetition processors of the greedy loop (HF RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor).  Per
// utterance two bit sets over the vocabulary, `words` 32-bit words each: `seen` = the ids of its decoder history (prompt + generated),
// `ban` = the ids that would complete an n-gram the history already holds.  Set from the prompt by repeat_init, kept current by the
// step's argmax launch, read by the logits epilogue.  The values live in device memory: one captured step serves any (penalty, ngram).
struct RepeatCtl {
    float penalty;  // 1 = off
    int ngram;      // 0 = off
};
static const int REPEAT_NGRAM_MAX = 64;
inline int repeat_words(int vocab) { return (vocab + 31) / 32; }

// Sequence bias and bad words of the greedy loop (HF SequenceBiasLogitsProcessor, NoBadWordsLogitsProcessor).  The model's
// table: the sequences of both lists, grouped by their LAST id into `slots` (ascending id; inside a slot the length-1 bias entry first,
// then the bias sequences in the caller's order, then the bans), so one thread sums a slot's biases in HF's order.  Per utterance, for
// the NEXT step: one SeqSlot per slot — the summed bias of the sequences whose prefix ends its history, whether one of them is a ban —
// and a bit set over the vocabulary, `words` 32-bit words, with the bit of every slot that is on.  Built from the prompt by
// seq_bias_init, kept current by the step's argmax launch (a bit is touched only where a slot goes on or off), read by the logits
// epilogue.  The kernels reach the table through the state's control block, so one captured step serves any table.
static const int SEQ_BIAS_MAX = 1024;     // sequences over the two lists together (so at most as many slots)
static const int SEQ_BIAS_LEN_MAX = 32;   // ids per sequence
struct SeqSlot {
    float bias;  // sum over the slot's matching bias sequences, in table order
    int flags;   // bit 0: on (a sequence of the slot matches: the id's bit is set); bit 1: a ban matches
};
struct SeqBiasCtl {
    int n_seq, n_slots;
    int eot;              // a length-1 ban of this id is dropped (HF's filter); -1 = none
    const int* ids;       // flattened sequences, table order
    const int* off;       // [n_seq + 1]
    const float* bias;    // [n_seq] (a ban's is not read)
    const int* ban;       // [n_seq] != 0: a bad word
    const int* slot_id;   // [n_slots] ascending
    const int* slot_off;  // [n_slots + 1] into the sequences
    const int* slot_of;   // [vocab] id -> slot, -1 = none (the epilogue's lookup at a set bit)
};

// Phrase-list constraint of the greedy loop (HF PrefixConstrainedLogitsProcessor over a trie of token ids).  The model's
// table: the trie of the phrases flattened to CSR — node v's child edges are edge_id / edge_next [edge_off[v] .. edge_off[v + 1]), ids
// ascending; terminal[v] is the index of the phrase that ends at v or -1.  Node 0 is the root; node `dead` has no edges and no phrase:
// where a walk leaves the trie it stays.  Per utterance: the node its generated ids have reached (ids >= free_from do not move it).
// The allowed set of a node — its edges' ids, eot where a phrase ends, every id >= free_from — is written, complemented, over the
// row's whole `ban` set of the repetition processors, the n-gram bans OR-ed on top: the logits epilogue reads nothing new.  Built by
// constraint_init, kept current by the step's argmax launch, reached through the state's control block like the sequence-bias table.
static const int CONSTRAINT_PHRASES_MAX = 4096;  // phrases of a table
static const int CONSTRAINT_LEN_MAX = 64;        // ids per phrase
static const int CONSTRAINT_NODES_MAX = 65536;   // trie nodes, the root and the dead node included
struct ConstraintCtl {
    int n_nodes, dead;
    int eot;        // allowed where a phrase ends; the pass's
    int free_from;  // ids >= this are always allowed and never move the node; the vocabulary size = none
    const int* edge_off;   // [n_nodes + 1]
    const int* edge_id;    // [edges] ascending inside a node
    const int* edge_next;  // [edges]
    const int* terminal;   // [n_nodes] phrase index or -1
};

struct DecLinearParams {
    const float* x;  // [B][ldx] fp32 activations
    int ldx;
    int x_is_t;    // != 0 (no LayerNorm prologue): x holds operand-dtype elements (TW) written by the producer kernel — exactly the
                   // values the MFMA fragment conversion would produce, so results are unchanged; half the bytes, no conversion
    int out_is_t;  // != 0 (plain output, no residual / cache append): out is stored as TW for such a consumer
    const float* ln_g;  // LayerNorm prologue (null = none)
    const float* ln_b;
    const void* W;  // [N][K], operand dtype
    int N, K, B;
    const float* bias;  // [N] or null
    int act, gelu_mode;
    const float* residual;  // [B][ldr] fp32 or null (may alias out)
    int ldr;
    float* out;  // [B][ldo] fp32
    int ldo;
    // QKV mode (kcache != null): columns [0,d) -> out (q), [d,2d) -> kcache, [2d,3d) -> vcache at row ctl->len
    void* kcache;
    void* vcache;
    long kv_batch_stride;  // elements between utterances in the cache
    int d_model;
    int kv_dtype;  // WM_F32 / WM_BF16 / WM_F16
    int kv_B;      // > 0: prompt prefill, rows are position-major (row = t * kv_B + b): row's K/V go to utterance b, cache row len + t
    const StepCtl* ctl;
    // dec_logits only: fused argmax stage 1 — per-utterance best (value, column) of each 128-column workgroup
    float* amax_val;  // [B][amax_stride] or null
    int* amax_idx;
    int amax_stride;
    const float* amax_mask;  // [N] additive mask (0 / -inf) applied to the argmax candidates only, or null
    // timestamp rules (null = off): candidates are split into text ids and timestamp ids by the utterance's TsState ranges; the
    // workgroups that cover ids >= ts_begin also emit the best admissible timestamp and (max, sum exp) of the admissible ones
    const TsState* ts_state;  // [B]
    int ts_begin;
    float* ts_val;  // [B][amax_stride] like amax_val; written for parts >= ts_begin / (ids per part) only
    int* ts_idx;
    float* ts_m;
    float* ts_s;
    // log-probabilities (null = off, needs amax_val): per part the sum of exp(v - amax_val) over the admissible text candidates —
    // with amax_val their (max, sum exp) pair, the text side of the softmax normaliser; the timestamp side is (ts_m, ts_s).  Non-null
    // selects the LP instantiation of the same kernel variant; null launches exactly the kernel, grid and LDS without it.
    float* lp_s;  // [B][amax_stride]
    long long* ts;  // developer timeline (dec_logits only)
    int ts_id;
    long long* dbg;  // developer build: per-(workgroup, wave) phase stamps of dec_logits (100 MHz clock), null = off
    // alignment-head capture (token timestamps; cap null = off): the output columns of every head h with cap_sel[h] >= 0 are also
    // stored, fp32, to cap[row * cap_row_stride + (step * cap_nsel + cap_sel[h]) * 64 + (column % 64)], step = ctl->len - cap_step0;
    // steps outside [0, cap_steps) are not stored
    float* cap;
    long cap_row_stride;
    int cap_step0, cap_steps, cap_nsel;
    signed char cap_sel[32];
    // capture by row map (forced alignment; null = the addressing above): [B] destination row of each input row, -1 = none.
    // Row r stores to cap[(cap_map[r] * cap_nsel + cap_sel[h]) * 64 + (column % 64)]; ctl->len, cap_row_stride, cap_step0 and
    // cap_steps are not read
    const int* cap_map;
    // dec_logits only — repetition processors (rp_seen null = off, needs rp_ban and rp_ctl): row b's logits at the ids of
    // rp_seen[b] are multiplied (negative) or divided (else) by rp_ctl->penalty, then those of rp_ban[b] are -inf — before the logits
    // store, the mask, the ranges and the log-prob sums.  Non-null selects the RP instantiation of the same kernel variant; null
    // launches exactly the kernel, grid and LDS without it.
    const unsigned* rp_seen;  // [B][rp_words]
    const unsigned* rp_ban;
    const RepeatCtl* rp_ctl;
    int rp_words;
    // dec_logits only — sequence bias / bad words (sb_hit null = off, needs the rp_* fields: penalty 1 and n-gram 0 are
    // exact no-ops): where row b's bit in sb_hit[b] is set, the slot of that id adds its bias BEFORE the penalty and, with a ban,
    // sets -inf AFTER the n-gram ban.  Non-null selects the SB instantiation of the same kernel variant.
    const unsigned* sb_hit;  // [B][rp_words]
    const SeqSlot* sb_val;   // [B][SEQ_BIAS_MAX]
    const SeqBiasCtl* sb_ctl;
};
template <typename TW> int launch_dec_linear(const DecLinearParams& p, hipStream_t st);  // WM_LAUNCH_*
bool dec_linear_supports_k(int K);  // K/32 k-steps must split into NW <= 16 waves x KPW <= 4 steps, or K = 3072 (the op hooks' answer)
bool dec_linear_long_supports_k(int K);   // K = 3072 or 4096: the K-long form (wm_op_dec_linear_long)
bool dec_linear_model_supports_k(int K);  // either of the two (checked at model load)
template <typename TW> int launch_dec_logits(const DecLinearParams& p, hipStream_t st);  // WM_LAUNCH_*
int dec_logits_parts(int N);  // fused-argmax partials per utterance that launch_dec_logits writes (amax_stride must cover them)
int dec_logits_ids_per_part(int N);  // vocabulary ids one part covers

struct AttnDecParams {
    const float* q;  // [B][d] fp32
    const void* K;   // [B][rows][d] cache of this layer
    const void* V;
    long batch_stride;
    int n_keys;  // >= 0: fixed key count (cross);  < 0: ctl->len + 1 (self, includes the row just written)
    int q_B;     // > 0: prompt prefill, query rows are position-major (row = t * q_B + b): K/V of utterance b, self length + t
    int nq;      // 4 (cross-attention, with q_B): one workgroup per (utterance, chunk) serves the 4 positions; else 0/1
    const StepCtl* ctl;
    int nsplit;
    float scale;
    float* part_o;      // [B][nsplit][d]
    float* part_ml;     // [B][nsplit][H][2]
    float* direct_out;  // non-null (nsplit must be 1): write the normalised output [B][d] here, skip the partials
    int out_dtype;      // element type of direct_out: WM_F32 / WM_BF16 / WM_F16 (the operand dtype of the projection that reads it)
    int H, d, B;
    int rps;  // filled by the launcher
    // cross-attention only: bytes of UNUSED dynamic LDS per workgroup.  34 KB (+ 20 KB static) admits two workgroups per CU
    // instead of four and leaves 52 KB of LDS and half the register file free: when several passes share the chip
    // (wm_transcribe_submit), the other passes' latency-bound launches then start beside this K/V stream instead of queueing
    // behind it — measured four passes in flight, tiny B = 64: 19.6 -> 19.1 ms per pass, although the kernel alone is
    // 1 us slower (26.3 vs 25.3 us).  0 for a pass that has the chip to itself.
    int lds_pad;
    long long* ts;  // developer timeline (null = off): see ts_put in kernels_decoder.hip
    int ts_id;
};
// key_lo non-null (per-row prompts; single-workgroup self-attention forms only): [utterances], utterance u sweeps the keys
// [key_lo[u], len + 1 (+ t)) — a separate kernel; with key_lo null exactly the launch it always was
// utt_of non-null (n-best scoring; chunked cross-attention forms only): [q_B, or B when q_B == 0] device ints, the row in
// batch slot b reads the K/V of utterance utt_of[b] — separate kernels likewise
template <typename TKV> int launch_attn_decode(const AttnDecParams& p, hipStream_t st, const int* key_lo = nullptr, const int* utt_of = nullptr);  // WM_LAUNCH_*
void launch_attn_combine(const float* part_o, const float* part_ml, void* out, int out_dtype, int B, int nsplit, int H, int d,
                         hipStream_t st, long long* ts = nullptr, int ts_id = 0);

// Cross-attention over the bf16 encoder output X with the K/V projections absorbed (bf16 encoder operands, fp32 K/V models):
//   s_hj = (scale·q_h·Wk_h)·X_j      o_h = ((Σ_j p_hj X_j) / l_h)·Wv_hᵀ + bv_h
// three launches: absorb (q' once per row, split into three bf16 images), the X sweep (un-normalised partials per key chunk),
// merge + V-apply (writes the attention output in out_dtype).  d = 64·H, H <= 8.
struct XAttnParams {
    const float* q;      // [rows][d] cross-Q output (fp32, unscaled)
    const void* Wk;      // [d][d] bf16, this layer's K projection (row = output feature h*64+e)
    const void* Wv;      // [d][d] bf16
    const float* bv;     // [d]
    const void* X;       // [utterances][n_keys][d] bf16 encoder output (ln_post)
    long x_stride;       // elements per utterance
    int n_keys, nsplit, H, d, rows;
    int q_B;             // > 0: prompt prefill, row r reads utterance r % q_B (position-major rows); else row = utterance
    float scale;
    void* qs;            // [rows][3][H][d] bf16: q' = hi + mid + lo
    float* part_y;       // [rows][nsplit][H][d]
    float* part_ml;      // [rows][nsplit][H][2]
    void* out;           // [rows][d] in out_dtype
    int out_dtype;
};
// late_loads: the absorb loop that requests its Wk rows after the q staging, as it was; same images bit for bit (op tests, A/B)
int launch_xattn_absorb(const XAttnParams& p, hipStream_t st, bool late_loads = false);  // WM_LAUNCH_*
int launch_xattn(const XAttnParams& p, hipStream_t st, const int* utt_of = nullptr);  // utt_of: as launch_attn_decode's, X of utt_of[slot]
int launch_xattn_merge(const XAttnParams& p, hipStream_t st);

void launch_dec_embed(const float* tok_emb, const float* pos_emb, const int* tok, const int* pos, float* x, int B, int d,
                      hipStream_t st);
// Top-k alternatives: what argmax_step leaves per row for the selection launch behind it — where the row's entries go,
// the id it emitted with its log-prob, the candidate ranges the step's processors left (read BEFORE the timestamp history moves on; a
// forced timestamp leaves no text range) and the normaliser as the pair the log-prob was formed from: lp = (value - ref) - logz.
static const int TOPK_MAX = 8;
struct TopkRow {
    int slot;  // entry of the [..][k] tables, -1: the row stores nothing (finished)
    int id0;
    float lp0;
    int lo0, hi0, lo1, hi1;  // candidates: ids of [lo0, hi0) ∪ [lo1, hi1)
    float ref, logz;
};
// argmax over logits rows (lowest index wins) + greedy-loop bookkeeping
struct ArgmaxParams {
    const float* logits;
    int ldl, V, B;
    const float* pval;  // non-null: reduce the fused-argmax partials [B][npart] instead of scanning the logits
    const int* pidx;
    int npart;
    int* next;        // [B] next token (also the next step's input)
    int* out_tokens;  // [B][out_stride] or null
    int out_stride;
    int* n_tokens;  // [B]
    int* finished;  // [B]
    StepCtl* ctl;
    int eot, ignore_eot;
    int advance;  // != 0: also do the end-of-step bookkeeping (len += 1, pos[b] += 1)
    int* pos;
    // non-null: a host-visible (pinned, device-mapped) pair the launch updates for the host's early-exit check, no stream
    // synchronisation needed: [0] = utterances finished BEFORE this step (never more than the truth), [1] = loop steps completed
    int* host_progress;
    long long* ts;  // developer timeline (null = off)
    int ts_id;
    // non-null: also write the NEXT step's input row x[b] = tok_emb[chosen id] + pos_emb[pos[b] (+1 when advancing)] — the
    // embedding launch of the following step folded into this one
    const float* emb_tok;
    const float* emb_pos;
    float* emb_out;
    int d, max_pos;
    // timestamp rules (ts_state null = off): pval / pidx then hold the best admissible TEXT id of each part, ts_* the timestamp side
    TsState* ts_state;
    TsRules rules;
    const float* ts_val;
    const int* ts_idx;
    const float* ts_m;
    const float* ts_s;
    int ts_part0;  // first part that covers timestamp ids
    // log-probabilities (lp_s null = off; needs pval): lp = s[id] - logsumexp(s) over the candidates the processors leave — admissible
    // text ∪ admissible timestamps, the timestamps alone when the rule forces one, everything the mask leaves with the rules off.  A step
    // whose candidates are all -inf emits id 0 with lp = -inf (never NaN).
    const float* lp_s;  // [B][npart] stage 1's text-side sums (DecLinearParams.lp_s)
    float* logprobs;    // [B][out_stride] or null: lp goes where the id goes in out_tokens (same guard: a finished row does not store)
    float* lp_sum;      // [B], with logprobs: running sum of the row's stored values
    float* lp_next;     // [B] or null: lp of next[b], stored unconditionally (op-level entry)
    // repetition processors (rp_seen null = off, needs out_tokens): a row that stores its id also sets the id's bit in
    // rp_seen[b], clears the bits rp_ban[b] held for this step and sets those of the next one from its history out_tokens[b]
    unsigned* rp_seen;  // [B][rp_words]
    unsigned* rp_ban;
    const RepeatCtl* rp_ctl;
    int rp_words;
    // sequence bias / bad words (sb_hit null = off, needs the rp_* fields): a row that stores its id also matches every
    // sequence's prefix against its new history tail and rewrites its slots and the bits of the slots that went on or off
    unsigned* sb_hit;  // [B][rp_words]
    SeqSlot* sb_val;   // [B][SEQ_BIAS_MAX]
    const SeqBiasCtl* sb_ctl;
    // top-k alternatives (tk_rows null = off, needs lp_s): the row's TopkRow for the selection launch behind this one
    TopkRow* tk_rows;  // [B]
};
int launch_argmax_step(const ArgmaxParams& p, hipStream_t st);  // WM_LAUNCH_*: refuses sets without the partials form or the id table
// The same launch under a phrase-list constraint (needs the rp_* fields): a row that stores its id moves its trie node
// along that id (ids >= free_from stay put, an id without an edge goes to the dead node) and rewrites rp_ban[b] as the complement of
// the new node's allowed set with the n-gram bans on top; a row that stores the eot and ends leaves its node's phrase in ct_match.
// A struct of its own, so the kernels of launch_argmax_step keep the argument block they always had.
struct ArgmaxCtParams : ArgmaxParams {
    int* ct_node;   // [B]
    int* ct_match;  // [B]
    const ConstraintCtl* ct_ctl;
};
int launch_argmax_step_ct(const ArgmaxCtParams& p, hipStream_t st);  // WM_LAUNCH_*
// Top-k alternatives, the selection launch: one workgroup per row sweeps the step's stored, processed logits row under
// the mask and the ranges of rows[b], keeps the k best (value descending, lowest id first among equals) and stores ids and
// log-probs (value - ref) - logz at table entry rows[b].slot (none when it is negative).  Rank 0 is rows[b]'s own (id0, lp0); a rank
// without a finite candidate holds (-1, -inf).
struct TopkSelectParams {
    const float* logits;  // [B][ldl]: what the logits kernel stored (behind the repetition processors and the sequence bias)
    int ldl, V, B;
    const float* mask;    // [V] additive (0 / -inf) or null: the mask the step's argmax ran under
    const TopkRow* rows;  // [B]
    int k;                // 1..TOPK_MAX
    int* ids;             // [entries][k]
    float* lps;           // [entries][k]
};
int launch_topk_select(const TopkSelectParams& p, hipStream_t st);  // WM_LAUNCH_*
// Start of a pass with the repetition processors, behind the init-tokens launch: writes ctl, clears both sets of the B rows, sets
// `seen` from each row's prompt out_tokens[b][0 .. n_tokens[b]) and `ban` for the first generated id.
struct RepeatInitParams {
    unsigned* seen;  // [B][words]
    unsigned* ban;
    int words, B;
    RepeatCtl* ctl;
    float penalty;
    int ngram;
    const int* out_tokens;  // [B][out_stride]
    int out_stride;
    const int* n_tokens;  // [B]
};
void launch_repeat_init(const RepeatInitParams& p, hipStream_t st);
// Start of a pass with sequence bias / bad words, behind the init-tokens launch: writes ctl, clears the B rows' bits and builds their
// slots and bits for the first generated id from each row's prompt out_tokens[b][0 .. n_tokens[b]).
struct SeqBiasInitParams {
    unsigned* hit;  // [B][words]
    SeqSlot* val;   // [B][SEQ_BIAS_MAX]
    int words, B;
    SeqBiasCtl* ctl;
    SeqBiasCtl table;       // what ctl becomes
    const int* out_tokens;  // [B][out_stride]
    int out_stride;
    const int* n_tokens;  // [B]
};
int launch_seq_bias_init(const SeqBiasInitParams& p, hipStream_t st);  // WM_LAUNCH_*
// Start of a pass with a phrase-list constraint, behind the repeat-init launch (and the sequence-bias one): writes ctl, puts every row
// on the root with no match, and rewrites the row's `ban` as the complement of the root's allowed set with the n-gram bans of its
// prompt out_tokens[b][0 .. n_tokens[b]) on top (ngram = 1: the ids of `seen`).
struct ConstraintInitParams {
    unsigned* ban;         // [B][words]
    const unsigned* seen;  // [B][words]
    int words, B, vocab;
    int* node;   // [B]
    int* match;  // [B]
    ConstraintCtl* ctl;
    ConstraintCtl table;  // what ctl becomes
    int ngram;
    const int* out_tokens;  // [B][out_stride]
    int out_stride;
    const int* n_tokens;  // [B]
};
int launch_constraint_init(const ConstraintInitParams& p, hipStream_t st);  // WM_LAUNCH_*
struct InitTokensParams {
    int* out_tokens;
    int out_stride;
    int* n_tokens;
    int* finished;
    StepCtl* ctl;
    int B, n_prompt;
    int prompt[16];
    int* tok_rows;  // non-null: also fill the prefill's position-major token / position rows [n_prompt][B]
    int* pos_rows;
    TsState* ts_state;  // non-null: start state of the timestamp rules
    TsRules rules;
    float* logprobs;  // non-null: zero the utterance's row of the log-prob table [B][out_stride] and its sum lp_sum[b]
    float* lp_sum;
};
void launch_init_tokens(const InitTokensParams& p, hipStream_t st);
// Per-row prompts: the prompt of row b is table[b * stride .. + len[b]); the rows end together at position Lmax.
struct RowPromptParams {
    const int* table;  // [B][stride]
    const int* len;    // [B], 1 <= len[b] <= Lmax; the dead slots in front of a shorter prompt embed its first id (never attended to)
    int stride, Lmax;
    int* key_lo;       // [B] out: Lmax - len[b], first cache row of the utterance's own keys
};
// as launch_init_tokens, tok_rows / pos_rows [Lmax][B] required; also writes key_lo
void launch_init_tokens_rows(const InitTokensParams& p, const RowPromptParams& r, hipStream_t st);
void launch_set_rows_step(StepCtl* ctl, int Lmax, int* pos, const int* len, int pos_delta, int B, hipStream_t st);
// No-speech probe.  capture: copies B rows of d floats (the residual rows of one prefill position, contiguous in the
// position-major activations) into the probe's [B][d] buffer.  finish: per row, the probability of `token` under the softmax whose
// per-part (max, Σ exp(v − max)) pairs the LP logits kernel left in pmax / psum (its amax_val / lp_s outputs, launched without mask
// and ranges on the captured rows), merged in ascending part order; the token's logit is recomputed from the row.
struct NoSpeechParams {
    const float* x;  // [B][ldx] captured residual rows (before the final LayerNorm)
    int ldx;
    const float* ln_g;
    const float* ln_b;
    const void* emb;  // [N][K] token embedding in the logits kernel's operand dtype
    int K, token, B;
    const float* pmax;  // [B][stride]
    const float* psum;
    int npart, stride;
    float* prob;  // [B] out: exp(logit − lse)
    float* lse;   // [B] out: log Σ exp over the whole vocabulary
};
void launch_no_speech_capture(const float* rows, float* out, int B, int d, hipStream_t st);
template <typename TW> void launch_no_speech_finish(const NoSpeechParams& p, hipStream_t st);
// Language detection: per row, the logits of the n_lang candidate ids only (LayerNorm of the captured [SOT]-pass row as
// the no-speech finish forms it, rounded to TW, times each candidate's embedding row, fp32 sums), their arg-max (ties: the smaller
// token id) and their softmax in list order.  The callers check 1 <= n_lang <= LANG_DETECT_MAX, 1 <= K <= LANG_DETECT_MAX_K and
// that every id is a vocabulary id.
static const int LANG_DETECT_MAX = 128;
static const int LANG_DETECT_MAX_K = 1280;
struct LangDetectParams {
    const float* x;  // [B][ldx] residual rows of the [SOT] pass (before the final LayerNorm)
    int ldx;
    const float* ln_g;
    const float* ln_b;
    const void* emb;      // [N][K] token embedding in the decoder's operand dtype
    const int* lang_ids;  // [n_lang] device list, any order
    int n_lang, K, B;
    int* lang_out;  // [B] out: the winning token id
    float* probs;   // [B][n_lang] out, list order; or null
    int* patch;     // non-null: the id is also written to patch[b * patch_stride + patch_col[b]] (the row's prompt-table slot)
    int patch_stride;
    const int* patch_col;  // [B]
};
template <typename TW> void launch_lang_detect(const LangDetectParams& p, hipStream_t st);
// ---- transcript scoring (kernels_score.hip) ------------------------------------------------------------------
// The vocabulary side of a teacher-forced pass over M hidden rows: final LayerNorm once per row into the sweep's operand form (a),
// the sweep (per (row, part): max, Σ exp(v − max), arg-max; the target's logit), the merge.  logprob[slot[r]] =
// logit[r][target[r]] − logsumexp(logit[r]) (0 when target[r] < 0), top_id[slot[r]] = the row's arg-max, lowest id on ties.
struct ScoreParams {
    const float* x;  // [M][K] residual rows (before the final LayerNorm)
    const float* ln_g;
    const float* ln_b;
    const void* emb;    // [N][K] token embedding in the decoder's operand dtype
    void* a;            // score_operand_bytes(M, K, dtype) of scratch
    const int* target;  // [M]
    const int* slot;    // [M] or null (= the row index)
    int M, N, K;
    float* pmax;  // [M][score_parts(N, dtype)] each
    float* psum;
    int* pidx;
    float* ztgt;  // [M]
    float* logprob;
    int* top_id;  // or null
};
int score_parts(int N, int dtype, int* stages_per_part = nullptr);  // dtype: WM_F32 = 0 / 16-bit; never a function of M
size_t score_operand_bytes(int M, int K, int dtype);
// WM_LAUNCH_*: LayerNorm, sweep, merge.  ev non-null: ev[0] is recorded behind the LayerNorm, ev[1] behind the sweep (phase timing)
template <typename TW> int launch_score(const ScoreParams& p, hipStream_t st, hipEvent_t* ev = nullptr);
// rows[r] -> out[dst[r]] for the n_rows rows of a prefill chunk whose dst[r] >= 0 (d floats each)
void launch_score_collect(const float* rows, float* out, const int* dst, int n_rows, int d, hipStream_t st);
void launch_score_sums(const float* logprob, int stride, const int* len, const int* ctx, float* sum, float* avg, int B, hipStream_t st);
// n-best scoring: per clip u the candidates row0[u] .. row0[u] + n_cand[u] of key [R] are ranked (descending, equal keys
// lower index first) and turned into a posterior, one workgroup per clip.  order / posterior [R], best [U].
struct ScoreRankParams {
    const float* key;  // [R]
    const int* row0;   // [U]
    const int* n_cand;  // [U]
    int* order;
    int* best;
    float* posterior;
};
void launch_score_rank(const ScoreRankParams& p, int U, hipStream_t st);
// rows of the gather buffer of SURVEY §8e: dst[r] = [n_tokens[r], ids of row r zero-padded to `stride`] for r < rows; rows in
// [rows, rows_cap) are zeroed (ragged shards gather a fixed row count per rank)
void launch_pack_tokens(const int* out_tokens, const int* n_tokens, int out_stride, int rows, int rows_cap, int stride, int* dst, hipStream_t st);
void launch_set_step(StepCtl* ctl, int len, int set_len, int* pos, int pos_value, int* tok, int tok_value, int B,
                     hipStream_t st);

// ---- token-level timestamps (kernels_align.hip) ------------------------------------------------------------------------
// After a greedy loop that captured the cross-attention queries of the alignment heads (DecLinearParams.cap), per utterance b with
// R_b = n_tokens[b] - n_prompt - 1 fed-back rows and F_b kept columns: probabilities of every head over all keys (align_probs), their
// z-score over rows, width-7 median over columns and mean over heads (align_norm), DTW over the negated matrix and the token times
// (align_dtw) — HF WhisperGenerationMixin._extract_token_timestamps.
static const int ALIGN_MAX_HEADS = 32;
static const int ALIGN_MAX_ROWS = 447;  // max_loop bound (n_text_ctx - 1)
struct AlignParams {
    const float* cap;     // [B][L][n_sel][64] captured cross-q rows (unscaled)
    int B, L, n_sel, n_prompt, T, d;  // utterances, rows per utterance (max_loop), heads, prompt length, n_audio_ctx, d_model
    const int* n_tokens;  // [B] ids per utterance
    const int* n_frames;  // [B] columns kept (F_b <= T), or null = T
    // keys of selected head k, K/V path (X null): kv_dtype rows kv + layer_k*kv_layer_stride + b*T*d + head_k*64, stride d
    const void* kv;
    int kv_dtype;
    long kv_layer_stride;
    // xattn path: K_h = X·Wk_hᵀ from the bf16 encoder rows X [B][T][d] and the bf16 K projection Wk (cross_kv_w, [n_layers][2][d][d]) into kh
    const void* X;
    const void* Wk;
    float* kh;            // [B][n_sel][T][64]
    int layer[ALIGN_MAX_HEADS], head[ALIGN_MAX_HEADS];
    float* probs;         // [B][n_sel][L][T]
    float* mean;          // [B][n_sel][T]
    float* stdv;          // [B][n_sel][T]
    float* M;             // [B][L][T] normalised, filtered, head-averaged matrix
    unsigned* trace;      // [B][L][ceil(T/16)] 2-bit DTW trace in global memory, or null: in LDS (the launcher decides)
    float* times;         // [B][out_stride]
    int out_stride;
    // ragged rows (forced alignment; both null = the n_tokens / n_prompt form above, both set = n_tokens is not read):
    // rows[b] = R_b rows of utterance b (clamped to [0, L]), row0[b] = the first id that has a row (times[b][0 .. row0[b]) = 0, the
    // id row0[b] + R_b repeats the last time, everything behind it is 0).  out_need: the host's max_b(row0[b] + rows[b] + 1)
    const int* rows;
    const int* row0;
    int out_need;
};
int launch_align_probs(const AlignParams& p, hipStream_t st);  // WM_LAUNCH_*
int launch_align_norm(const AlignParams& p, hipStream_t st);
int launch_align_dtw(const AlignParams& p, hipStream_t st);
size_t align_dtw_lds_bytes(int L, int T);  // dynamic LDS of align_dtw with the trace in LDS (0: does not fit, trace goes to global)
// A long-form window pass with token timestamps: one kernel, launched on both sides of the chain.  Row r of the pass holds
// window items[r] = (utterance, seek, frames) with n_tokens[r] ids, prompt_len[r] of them prompt (null: n_prompt for every row).
//   mode 0, before the chain: rows[r] = n_tokens[r] - prompt_len[r] - 1 clamped to [0, L] (0 for the spare rows r >= n_real) and
//           row0[r] = prompt_len[r]: the ragged tables the chain reads (AlignParams::rows / row0).
//   mode 1, behind it: out[r][i], i in [0, L], = double(times[r][prompt_len[r] + i]) + double(seek_r) · 0.02 / 2 for the row's
//           n_tokens[r] - prompt_len[r] generated ids, 0 past them and in the spare rows (L = 0 is allowed: no chain ran, times is 0).
struct AlignWindowParams {
    int mode, B, n_real, L, n_prompt, out_stride;  // rows of the pass, real ones, max_loop, longest prompt, columns of `times`
    const int* n_tokens;    // [B]
    const int* prompt_len;  // [B] or null
    const int* items;       // [B][3]
    int *rows, *row0;       // [B]
    const float* times;     // [B][out_stride], the chain's output
    double* out;            // [B][L + 1]
};
int launch_align_window(const AlignWindowParams& p, hipStream_t st);  // WM_LAUNCH_*

// ---- log-mel front end (kernels_frontend.hip) ------------------------------------------------------------------------
void launch_zero_tails(float* pcm, const int* len, int B, int N, hipStream_t st);
void launch_frames(const float* pcm, float* F, const float* window, int B, int N, int n_frames, int hop, hipStream_t st, int t0 = 0);
void launch_mel_log(const float* spec, const float* fb, const int* band, float* logmel, int B, int n_frames, int n_mels, hipStream_t st,
                    int out_frames = 0, int t_out = 0);
// long-audio front end and window gather (kernels_frontend.hip); part: >= 256·B floats of scratch
void launch_mel_norm_long(float* logmel, float* part, int B, size_t n, hipStream_t st);
void launch_window_gather(const float* mel, const int* items, float* out, int rows, int n_mels, int F, int W, hipStream_t st);
void launch_mel_norm(const float* logmel, float* out, int B, int n, hipStream_t st);
// chunked long-form: rows [row0, row0 + rows) of the item table (item_stride ints each: recording, start, len, ...) cut
// out of pcm [R][T_max] into out [rows][N], zero-padded past len
void launch_chunk_gather(const float* pcm, const int* items, int item_stride, int row0, float* out, int rows, size_t T_max, int N, hipStream_t st);
// any sample rate / int16 -> fp32 16 kHz: resample_kernel.  x [B][stride_in] float or int16 with n_in[b] samples ->
// y [B][stride_out] and n_out[b] = ceil(nw * n_in[b] / orig); cells of y at or beyond n_out[b] are not stored.  taps: compact and
// phase-minor, taps[q * nw + p] = h[p][lo[p] + q]; span [nw][2] = (lo, cnt), each phase's non-zero taps.  frames = resample_frames().
struct ResampleParams {
    const void* x;
    float* y;
    const int* n_in;
    int* n_out;
    size_t stride_in, stride_out;
    const float* taps;
    const int* span;
    int orig, nw, width, frames;
};
int resample_frames(int orig, int nw, int width);  // input frames per workgroup
int launch_resample(const ResampleParams& p, bool in_i16, int B, int64_t max_n_out, hipStream_t st);  // WM_LAUNCH_*
// the stitch (kernels_chunked.hip): packed rows [n][1 + stride] = (count, ids), recording r owning rows [rec_off[r], rec_off[r + 1]) ->
// merged [n_rec][cap], merged_len [n_rec].  One workgroup per recording; LDS 2 · stride ints + 3 KB.  WM_LAUNCH_*
static const int CHUNK_MERGE_MAX_IDS = 2048;
int launch_chunk_merge(const int* rows, const int* rec_off, int n_rec, int stride, int first_special, int* merged, int* merged_len, int cap,
                       hipStream_t st);
// the stitch with timestamps: chunk_segments_kernel, one workgroup per recording; LDS 4 · stride ints + 3 KB.  WM_LAUNCH_*
struct ChunkSegArgs {
    const int* rows;      // [n_chunks][1 + stride]: (count, ids), the decoder prompt included
    const int* rec_off;   // [n_rec + 1]
    const int* tab;       // chunk k: tab[k * tab_cols + tab_c0 + 0 .. 2] = (len, stride_left, stride_right) in samples
    const float* times;   // word mode: [n_chunks][stride] token times aligned with the ids; else null
    int tab_cols, tab_c0, stride, first_special, timestamp_begin, segment_size;
    double time_precision;
    int* merged;          // [n_rec][cap]
    int* merged_len;      // [n_rec]
    int* n_seg;           // [n_rec]: the segments found, also when more than seg_cap
    double* seg_times;    // [n_rec][seg_cap][2]: start, end (NaN = None)
    int* seg_range;       // [n_rec][seg_cap][2]: [begin, end) in merged
    double* pairs;        // word mode: [n_rec][cap][2]
    int cap, seg_cap;
};
int launch_chunk_segments(const ChunkSegArgs& a, int n_rec, hipStream_t st);

// ---- small ops for the op-level C-ABI ----------------------------------------------------------------------------
void launch_gelu(float* t, size_t n, int mode, hipStream_t st);
void launch_softmax_rows(float* t, int rows, int cols, hipStream_t st);
void launch_argmax_plain(const float* t, int n, int* idx, hipStream_t st);
template <typename T> void launch_convert(const float* in, void* out, size_t n, hipStream_t st);
void launch_transpose_f32(const float* in, float* out, int rows, int cols, hipStream_t st);

}  // namespace wm
