// wm_runtime.h — what the runtime's host sources share: the model and state types, a pass's request structs, and the core functions of
// whisper_mi.cpp (and the few of one subsystem that another calls) that every later subsystem builds on.  The file map is in DESIGN §38.
// Internal to the library like wm_host.h, which it includes: the types keep default visibility, every function declared here is hidden.
#pragma once
#include "wm_host.h"

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>

using namespace wm;

#pragma GCC visibility push(default)  // as in wm_host.h: the types keep the visibility they always had

// the front end's framing (wm_frontend.cpp); the hop also turns samples into frames in the chunked, score and long-form entries
static const int FE_NFFT = 400, FE_HOP = 160, FE_NFREQ = 201;
static int dec_dtype(const wm_config& c) { return c.decoder_fp32 ? WM_F32 : c.compute_dtype; }  // operand dtype of the decoder
static int grow(DevBuf& b, size_t bytes) { return b.p && b.bytes >= bytes ? 0 : b.alloc(bytes); }

struct EncLayer {
    DevBuf qkv_w, qkv_b, o_w, o_b, ln1_g, ln1_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_g, ln2_b;
};
struct DecLayer {
    DevBuf sqkv_w, sqkv_b, so_w, so_b, ln1_g, ln1_b, cq_w, cq_b, co_w, co_b, lnx_g, lnx_b, fc1_w, fc1_b, fc2_w, fc2_b, ln2_g,
        ln2_b;
};

// ---- what a pass is asked to do, and where its results go -------------------------------------------------------------
struct NsAsk {  // the no-speech probe a pass carries; token < 0: none
    int token = -1, n_init = 0;
};
struct LangAsk {  // language detection a pass carries; ids == null: none.  only: no transcription (wm_detect_language)
    const int32_t* ids = nullptr;  // host [n]
    int n = 0, n_init = 0, sot = -1;
    bool only = false;
};
struct RowPrompts {
    const int32_t* ids;  // host [B][stride]
    const int32_t* len;  // host [B]
    int stride, Lmax;
};
struct ScoreAsk {  // a score pass, already validated by score_check
    const int32_t* ids;  // host [B][stride]
    const int32_t* len;  // host [B]
    const int32_t* ctx;  // host [B] or null (= 1)
    int stride, pos_mode;
    // an align pass: cols non-null = the columns kept per row (align_cols); lp = the vocabulary side runs too
    const std::vector<int32_t>* cols = nullptr;
    bool lp = true;
    // an n-best pass: n_utt > 0 = the rows are the candidates of n_utt clips, n_cand[u] consecutive rows each; the mel
    // holds n_utt clips.  normalize: rank by avg_logprob instead of sum_logprob
    int n_utt = 0;
    const int32_t* n_cand = nullptr;  // host [n_utt]
    bool normalize = false;
};
struct WinAsk {  // the windows a long-form timestamp pass decodes
    const int32_t* items;  // device [B][3]: (utterance, seek, frames) per row
    int n_real;            // rows [n_real, B) repeat row 0: no align rows, zero times
};
struct RepeatAsk {  // the logits processors of a greedy pass, as wm_set_repeat_options / wm_set_sequence_bias left them when the pass was asked for
    float penalty = 1.f;
    int ngram = 0;
    std::shared_ptr<const SeqTable> sb;  // sequence bias / bad words: null = off
    std::shared_ptr<const ConstraintTable> ct;  // phrase-list constraint: null = off
    int sb_gen() const { return sb ? sb->gen : 0; }
    int ct_gen() const { return ct ? ct->gen : 0; }
    bool on() const { return penalty != 1.f || ngram > 0 || sb || ct; }
    bool operator==(const RepeatAsk& o) const { return penalty == o.penalty && ngram == o.ngram && sb_gen() == o.sb_gen() && ct_gen() == o.ct_gen(); }
};
// One pass: encoder, prefill, greedy loop (or the teacher-forced pass of `score`) for B utterances.  The entry points validate, fill
// one of these and hand it to a driver (run_now / submit_slot); nothing in it is owned, it lives on the caller's stack.
struct PassAsk {
    const float* mel = nullptr;
    int mel_on_device = 0, B = 0;
    const wm_decode_opts* opts = nullptr;  // null for a score / align pass and for lang.only
    bool allow_poll = false;               // the synchronous entries pump their own loop (run_now sets it, nobody else)
    const float* mel2 = nullptr;           // a coalesced pair: utterances [B/2, B) come from mel2
    int mel2_on_device = 0;
    const std::vector<int32_t>* cols = nullptr;  // token timestamps: cols[b] = columns kept for row b (n_frames[b] // 2, or n_audio_ctx)
    const RowPrompts* rows = nullptr;            // per-row prompts (opts->n_prompt = rows->Lmax, opts->prompt unused)
    bool lp = false;                             // per-token log-probabilities
    NsAsk ns;
    LangAsk lang;
    const ScoreAsk* score = nullptr;
    const WinAsk* win = nullptr;  // with cols: a long-form window pass whose times are finished on the device
    RepeatAsk rp;                 // filled by the drivers (run_now / submit_slot / the long-form scheduler) from the model's setting
    int top_k = 0;                // top-k alternatives of a greedy log-prob pass, filled by run_now / submit_slot likewise; 0 = off
};
static PassAsk lang_only_ask(const float* mel, int mel_on_device, int B, const int32_t* lang_ids, int n_lang, int sot) {
    PassAsk ask{mel, mel_on_device, B};
    ask.lang.ids = lang_ids;
    ask.lang.n = n_lang;
    ask.lang.sot = sot;
    ask.lang.only = true;
    return ask;
}
struct PassOut {  // where a pass's results go: the caller's buffers, null = not asked for
    int32_t *tokens = nullptr, *n_tokens = nullptr;
    float *token_times = nullptr, *token_logprobs = nullptr, *avg_logprob = nullptr, *no_speech_prob = nullptr;
    int32_t* lang_out = nullptr;
    float* lang_probs = nullptr;
    int32_t* dev_packed = nullptr;  // wm_transcribe_wait_device: the ids stay on the device, [rows_cap][1 + pack_stride]
    int rows_cap = 0, pack_stride = 0;
    float* dev_times = nullptr;  // with dev_packed, a pass with token timestamps: its times stay on the device too, [rows_cap][pack_stride]
    int32_t* top_ids = nullptr;  // score / align passes
    float* sum_logprob = nullptr;
    int32_t *order = nullptr, *best = nullptr;  // an n-best score pass: [rows], [clips], [rows]
    float* posterior = nullptr;
    double* win_times = nullptr;  // a window pass (PassAsk::win): [B][max_loop + 1] times of the generated ids, offset included
};
enum class PassKind { transcribe, score, align, nbest };  // which wait family collects a slot's pass

struct wm_model {
    wm_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    int Cp = 0;  // mel channels padded to a multiple of 32 (implicit-GEMM K)
    int K1 = 0;  // conv1 implicit-GEMM K (3*Cp rounded up to 64)
    int Vpad = 0;
    // utterances per encoder pass.  Measured (tiny, B=64, ms per 64 clips): 4 -> 12.0, 8 -> 9.0, 16 -> 7.6, 32 -> 6.8,
    // 64 -> 6.7: filling the chip (>= 4 tiles per CU per launch) matters more than keeping activations in the 256 MB L3
    int enc_chunk = 64;  // (re-measured with the row-panel GEMMs: 16 -> 6.1, 32 -> 5.0, 64 -> 4.8 ms)
    DevBuf conv1_w, conv1_b, conv2_w, conv2_b, enc_pos;
    std::vector<EncLayer> enc;
    DevBuf enc_ln_g, enc_ln_b;
    DevBuf tok_emb_f, tok_emb_t, dec_pos;
    std::vector<DecLayer> dec;
    DevBuf dec_ln_g, dec_ln_b;
    DevBuf cross_kv_w, cross_kv_b;  // [L*2*d][d] rows: layer-major, K then V
    // Cross-attention over the bf16 encoder output with the K/V projections absorbed (bf16 encoder operands + fp32 K/V, d = 64·H,
    // H <= 8): states keep X = ln_post rows in bf16 instead of an fp32 cross K/V cache, a quarter of the bytes per decode step
    // (DESIGN §3).  Chosen at load time and used by every entry point of the model; WM_XATTN_OFF (developer build) keeps the cache.
    bool xattn = false;
    DevBuf ts_buf;     // developer timeline (WM_TRACE_EVENTS=<file>): count + (tag, clock) pairs
    // log-mel front end (lazy): constants + scratch sized for max_batch utterances
    struct Frontend {
        bool ready = false;
        int chunk = 16;  // utterances per DFT GEMM
        DevBuf window, dft, fb, band, pcm, lens, frames, spec, logtmp, mel;
        struct Resampler {  // the sinc table of one input rate, built on first use and kept like the filter bank
            int sr = 0, orig = 0, nw = 0, width = 0, frames = 0;
            DevBuf taps, span;
        };
        std::vector<Resampler*> rs;
    } fe;
    static const int NSLOT = 8;
    wm_state* cached = nullptr;           // slot 0: the state behind wm_transcribe / wm_transcribe_submit(slot 0)
    wm_state* slots[NSLOT - 1] = {};  // slots 1..7: further pipeline stages (wm_transcribe_submit)
    std::unordered_set<wm_state*> states;  // every state created on this model (wm_state_new), freed with it
    // Coalescing (wm_config.coalesce == 2): two consecutive wm_transcribe_submit calls of the same batch size and options share ONE
    // decode state of 2·B rows — the 33 latency-bound launches of a decode step cost the same for 128 rows as for 64.  The first
    // call of a pair is held (`held`) until its partner arrives (or until it is waited for: then it runs alone); each call still
    // returns exactly its own ids.
    struct Held {
        bool active = false;
        int slot = 0;
        PassAsk ask;  // the held request; ask.opts = &o and ask.cols = &cols (when asked for): the only owning copy of a request
        wm_decode_opts o{};
        std::vector<int32_t> prompt, sup, bsup, cols;  // deep copies: the caller's arrays need not outlive the call
    } held;
    struct SlotRef {  // what a submitted slot holds and where its rows live (filled by record_pass alone)
        bool pending = false;
        wm_state* st = nullptr;  // null while the slot is only held
        int row0 = 0, rows = 0;
        int total = 0;  // ids per utterance; a score / align pass: the caller's ids_stride
        PassKind kind = PassKind::transcribe;
        bool tt = false;    // the pass computes token timestamps (wm_transcribe_wait_tt may collect them)
        bool lp = false;    // ... log-probabilities (wm_transcribe_wait_lp; an align pass: wm_align_wait's log-prob outputs)
        bool ns = false;    // ... the no-speech probe (wm_transcribe_wait_lp_ns)
        bool lang = false;  // ... the language (wm_transcribe_wait_lang)
    } slot_ref[8];
    wm_state* pairs[4] = {};  // 2·B-row states of coalesced pairs
    int last_steps[8] = {-1, -1, -1, -1, -1, -1, -1, -1};  // loop iterations enqueued for each slot's last collected pass
    // Loop pump (natural-stop passes of wm_transcribe_submit): one host thread per model that keeps each pending pass's greedy loop
    // two sub-chunks ahead of the GPU and stops enqueueing once the device reports every utterance finished (whisper.mojo:206-207).
    std::thread pump;
    std::mutex pump_mu;
    std::condition_variable pump_cv;
    std::vector<wm_state*> pump_work;  // passes whose loop is not fully enqueued yet
    bool pump_quit = false;
    // token-level timestamps: HF generation_config.alignment_heads, (layer, head) pairs in the caller's order; empty = off
    std::vector<int32_t> align_pairs;
    RepeatAsk repeat;  // wm_set_repeat_options / wm_set_sequence_bias: what every greedy pass asked for from now on carries (a held submit keeps its own)
    int seq_gen = 0;   // tables built so far by wm_set_sequence_bias
    int ct_gen = 0;    // ... by wm_set_constraint
    int top_k = 0;     // wm_set_top_k: what every log-prob pass asked for from now on carries (a held submit keeps its own)
    struct AlignRef {  // where a slot's last timestamp pass left its alignment weights (wm_alignment_weights)
        wm_state* st = nullptr;
        int row0 = 0, rows = 0, gen = 0;
    } align_ref[8];
    struct TopkRef {  // where a slot's last collected log-prob pass left its top-k tables (wm_transcribe_top_k)
        wm_state* st = nullptr;
        int row0 = 0, rows = 0, total = 0, k = 0, gen = 0;
    } topk_ref[8];
    struct ConstraintRef {  // where a slot's last collected constrained pass left its matches (wm_transcribe_constraint_match)
        wm_state* st = nullptr;
        int row0 = 0, rows = 0, gen = 0;
    } ct_ref[8];
    // sequential long-form decoding: the long log-mel and its scratch (frames / spec hold one chunk of frames, the
    // rest grows with the audio), and two internal decode states, apart from the caller's slots, with each one's gathered
    // windows and work items
    struct LongForm {
        DevBuf pcm, lens, frames, spec, part, mel, in_mel;
        wm_state* st[2] = {nullptr, nullptr};
        DevBuf win[2], items[2];
        std::vector<int32_t> h_items[2];
    } lf;
};

struct wm_state {
    wm_model* m = nullptr;
    int B = 0;
    int Bc = 0;  // encoder chunk
    int nsplit = 1;
    int out_stride = 0;
    bool has_enc = false, has_cross = false;
    int host_len = 0;
    // Decode lanes: the batch is cut into independent sub-batches, each decoding on its own HIP stream with its own
    // control block and captured step graph, so one lane's latency-bound launches overlap another's K/V streaming.
    struct Lane {
        int b0 = 0, nb = 0;
        hipStream_t st = nullptr;
        StepCtl* ctl = nullptr;
        static const int NEXEC = 3;  // instances of the same captured step, launched round-robin
        hipGraphExec_t graph[3] = {nullptr, nullptr, nullptr};
        hipEvent_t done = nullptr;
    };
    std::vector<Lane> lanes;
    hipEvent_t enc_done = nullptr;
    hipStream_t enc_stream = nullptr;  // stream the pending pass's encoder was enqueued on
    bool graphs_valid = false;  // the lanes' graphs hold graph_step (false also after invalidate_step_graphs)
    bool pending = false;   // a submitted pass has not been waited for yet
    int halves_left = 0;    // coalesced pair: slots that have not collected their rows yet
    bool synced = false;    // the pending pass's completion has been waited for (second half of a pair does not wait again)
    bool shares_chip = false;  // this state's passes run beside other passes (pipelined entry): K/V stream at two workgroups per CU
    int trace_id = 1;       // slot + 1: tags this state's entries in the developer timeline
    int pend_total = 0;     // ids per utterance of the pending pass
    // Greedy loop of the pending pass, enqueued in sub-chunks of LOOP_CHUNK steps with at most two sub-chunks queued ahead of the GPU
    // (natural stop only; a fixed-length pass is enqueued whole).  h_prog: pinned, device-mapped [finished utterances, cache length],
    // written by every step's argmax launch.
    volatile int* h_prog = nullptr;
    int* d_prog = nullptr;
    int loop_total = 0, loop_enq = 0;  // steps the loop may run / steps enqueued so far
    int chunk_k = 0;                   // sub-chunks enqueued
    hipEvent_t chunk_ev[2] = {nullptr, nullptr};
    std::atomic<bool> enq_done{true};  // the pending pass is fully enqueued (its `done` events are recorded)
    int enq_rc = 0;                    // status of the pump's enqueues
    std::string enq_err;
    int last_steps = -1;               // loop steps enqueued for the most recent completed pass (wm_transcribe_steps)
    // Everything a step of the greedy loop depends on beside the device buffers: loop_step runs `step`, the lanes' graphs
    // hold `graph_step`, a pass recaptures when they differ.  Whatever loop_step reads from the state must be a field here.
    struct StepKey {
        int eot = 0, ignore_eot = 0;
        TsRules rules{};           // timestamp rules (tb <= 0: off)
        bool shares_chip = false;  // K/V stream at two workgroups per CU
        struct Cap {               // the alignment-head capture: al.cap.p, al.L, al.n_prompt, al.pairs of a timestamp pass, else empty
            const void* buf = nullptr;
            int L = 0, n_prompt = 0;
            std::vector<int32_t> pairs;
            bool operator==(const Cap& o) const { return buf == o.buf && L == o.L && n_prompt == o.n_prompt && pairs == o.pairs; }
        } cap;
        bool rows = false, lp = false;  // self-attention in the key-window form (rw.on); log-probabilities (lp.on)
        bool rp = false;                // repetition processors (rp.on): the flag only — penalty and n-gram size are read on the device
        bool sb = false;                // sequence bias / bad words (rp.sb): the flag only — the table is reached through the control block
        bool ct = false;                // phrase-list constraint (rp.ct): the flag only, likewise
        int top_k = 0;                  // top-k alternatives (tk.k): the logits store, the argmax instantiation and the selection launch
        bool operator==(const StepKey& o) const {
            return eot == o.eot && ignore_eot == o.ignore_eot && rules.tb == o.rules.tb && rules.eos == o.rules.eos &&
                   rules.max_init == o.rules.max_init && rules.vocab == o.rules.vocab && shares_chip == o.shares_chip && cap == o.cap &&
                   rows == o.rows && lp == o.lp && rp == o.rp && sb == o.sb && ct == o.ct && top_k == o.top_k;
        }
    };
    StepKey step, graph_step;
    const float* last_mel = nullptr;  // device pointer of the last encoded batch (bench replays the encoder on it)
    // encoder arena (sized for Bc utterances)
    DevBuf mel_dev, mel_t, h1, x, xn, qkv, ao, hid, enc_t;
    DevBuf enc_f;            // [B*n_ctx][d] fp32
    DevBuf cross_kv;         // [L][2][B][n_ctx][d] kv dtype (not allocated when m->xattn)
    DevBuf enc_x;            // m->xattn: [B][n_ctx][d] bf16 ln_post rows, what the cross-attention streams
    DevBuf xq, part_y;       // m->xattn: q' images [rows][3][H][d] bf16; chunk partials [rows][nsplit][H][d] fp32
    DevBuf self_kv;          // [L][2][B][n_text_ctx][d]
    // decode arena
    DevBuf mask_steady, mask_begin;  // [Vpad] additive logit masks (0 / -inf) for the fused argmax
    std::vector<int32_t> sup_cached, bsup_cached;
    bool masks_valid = false;
    static const int PREFILL_MAX = 16;  // prompt positions decoded in one pass (= the n_prompt bound of wm_decode_opts)
    DevBuf ts_state, ts_val, ts_idx, ts_m, ts_s;  // timestamp rules: per-utterance history / ranges, per-part timestamp partials
    int no_ts_cached = -1;
    DevBuf dx, dq, dattn, dhid, part_o, part_ml, logits, amax_val, amax_idx, tok, pos, tok_rows, pos_rows, ctl, out_tokens, n_tokens, finished;
    int npart = 0;  // fused-argmax partials per utterance = workgroups per row block of the logits kernel
    // token-level timestamps of the pending pass (on = asked for): the loop's cross-q launches of the alignment layers also store the
    // selected heads' query rows (cap), the post-loop kernels (kernels_align.hip) turn them into times.  Buffers grow on demand.
    struct Align {
        bool on = false;
        int L = 0, n_prompt = 0, gen = 0;         // rows per utterance (= max_loop), prompt length, pass counter
        std::vector<int32_t> pairs;               // (layer, head) pairs of the pass
        std::vector<int32_t> cols;                // [B] columns kept per utterance (n_frames // 2, or n_audio_ctx)
        DevBuf cap, kh, probs, mean, stdv, M, trace, times, ncols;
        // forced alignment (ragged = the pending or last pass was an align pass): every utterance has its own row count
        // R_b and first timed id; L = max R_b; map [Lmax][B]: where a position-major prefill row's query rows go in cap, as a row of
        // [B][L] (-1: left padding or context); times is [B][stride] with the caller's ids_stride
        bool ragged = false;
        int stride = 0;
        std::vector<int32_t> h_rows, h_row0, h_map;
        DevBuf rows, row0, map;
        // a long-form window pass (win = the pending pass is one): rows / row0 are made on the device from n_tokens and the
        // prompt lengths, wtimes [B][L + 1] float64 is what the pass hands back.  wtimes is allocated by the first such pass.
        bool win = false;
        int n_real = 0;
        const int32_t* items = nullptr;
        DevBuf wtimes;
    } al;
    // per-row prompts of the pending pass (on = wm_transcribe_rows and its kin).  Buffers are allocated by the first such
    // pass: table [B][n_text_ctx] ids, len [B], key_lo [B] (first cache row of each utterance's own keys).
    struct Rows {
        bool on = false;
        int Lmax = 0, stride = 0;
        DevBuf table, len, key_lo;
        std::vector<int32_t> h_table, h_len;
    } rw;
    // log-probabilities of the pending pass (on = wm_transcribe_lp and its kin): stage 1's text-side sums [B][npart], the
    // table [B][out_stride] that mirrors out_tokens (zeroed by the init-tokens launch) and the per-row sums.  Part of the arena.
    struct Lp {
        bool on = false;
        DevBuf part_s, table, sum;
        std::vector<int32_t> n_prompt;  // [B] prompt length of each row of the pending pass
    } lp;
    // top-k alternatives of the pending pass (k > 0 = a log-prob pass asked for with wm_set_top_k in force): each step's
    // TopkRow per row, and the [B][out_stride][k] id / log-prob tables beside out_tokens (sized for k = TOPK_MAX; entries of generated
    // positions only are ever written).  Part of the arena.  gen counts the state's passes of any kind.
    struct Tk {
        int k = 0, gen = 0;
        DevBuf rows, ids, lps;
    } tk;
    // repetition processors of the pending pass (on = the pass was asked for with wm_set_repeat_options in force): the
    // rows' two bit sets [B][words] and the control block the kernels read (penalty, n-gram size).  Allocated by the first such pass.
    struct Rp {
        bool on = false;
        RepeatAsk ask;
        int words = 0;
        DevBuf seen, ban, ctl;
        // sequence bias / bad words (sb = ask.sb non-null, always with on): the rows' hit bits [B][words], their slots
        // [B][SEQ_BIAS_MAX] and the control block that names the table.  Allocated by the first such pass.
        bool sb = false;
        DevBuf hit, val, sbctl;
        // phrase-list constraint (ct = ask.ct non-null, always with on): the rows' trie nodes [B], the phrase each row
        // ended on [B] and the control block that names the table.  Allocated by the first such pass.
        bool ct = false;
        int ct_gen = 0;  // counts the passes of this state: a ConstraintRef of another pass is stale
        DevBuf node, match, ctctl;
    } rp;
    // no-speech probe of the pending pass (on = wm_transcribe_lp_ns and its kin, always with lp.on): the residual rows
    // of the <|startoftranscript|> position [B][d], the probe's OWN sweep partials [B][npart] (the step's amax / lp_s partials and
    // the control block are not touched) and the results [B].  Part of the arena; runs outside the captured step graph.
    struct Ns {
        bool on = false;
        int token = -1, n_init = 0;
        DevBuf x, pmax, pidx, psum, prob, lse;
    } ns;
    // language detection of the pending pass (on = wm_transcribe_lang and its kin, always with rw.on; wm_detect_language
    // uses the buffers without a pass): the residual rows of the [<|startoftranscript|>] pass [B][d] (NOT ns.x: the probe's row of the
    // same pass comes from the real prefill, behind any previous text), the candidate ids, each row's language slot in the prompt
    // table and the results.  Part of the arena; runs outside the captured step graph.
    struct Lang {
        bool on = false;
        int n = 0, n_init = 0, sot = -1;
        DevBuf x, ids, col, out, probs;  // [B][d] fp32, [LANG_DETECT_MAX], [B], [B], [B][LANG_DETECT_MAX] (used as [B][n])
        std::vector<int32_t> h_ids, h_col;
    } lg;
    // transcript scoring (on = the pending pass is a score pass).  Everything here is allocated by the first score pass of
    // the state and grows on demand, never in state_new: the arenas of a state that is never scored are what they always were.
    // rows [M][d]: the last layer's residual rows of the real inputs, utterance-major; a: their LayerNorm in the sweep's operand
    // form; the sweep's partials [M][parts]; per row the target id and the slot of its results in the [B][stride] tables; dst
    // [Lmax][B]: where a position-major prefill row goes in `rows` (-1: left padding).
    struct Score {
        bool on = false;
        int M = 0, stride = 0, Lmax = 0;
        DevBuf rows, a, pmax, psum, pidx, ztgt, target, slot, dst, len, ctx, lp, top, sum, avg;
        std::vector<int32_t> h_tok, h_pos, h_key_lo, h_dst, h_target, h_slot, h_len, h_ctx;
        // phase marks of the last score pass (wm_score_phases): before the encoder, behind it, behind the prefill chunks, the
        // LayerNorm, the sweep, the merge + sums.  Created by the first score pass.
        // An align pass adds ev[6] behind its align chain (wm_align_phases).
        hipEvent_t ev[7] = {};
        bool timed = false;  // a completed pass's marks are all recorded
        bool timed_al = false;  // ... and it was an align pass: ev[6] too
    } sc;
    // n-best scoring (on = the pending pass is an n-best score pass): utt_of [B] = the clip each row's cross-attention
    // reads, row0 / n_cand [U] = each clip's rows, and the ranking's results.  Allocated by the first n-best pass of the state, never
    // in state_new; every pass clears `on` before it reads anything.
    struct Nbest {
        bool on = false;
        int U = 0;
        DevBuf utt_of, row0, n_cand, order, best, post;
        std::vector<int32_t> h_utt_of, h_row0, h_n_cand;
    } nb;
};

// A view of `nb` utterances starting at b0, decoding on stream st under control block ctl.
struct DecView {
    int b0, nb;
    hipStream_t st;
    StepCtl* ctl;
};
static DecView whole_batch(wm_model* m, wm_state* s) { return DecView{0, s->B, m->stream, s->ctl.as<StepCtl>()}; }
static void invalidate_step_graphs(wm_state* s) { s->graphs_valid = false; }  // the next greedy pass captures its step anew

// What one decode_core call does: by default a single-position step that embeds its input and produces no logits.
enum class Logits { none, partials, full };  // partials: the fused-argmax partials only (the greedy loop); full: also [B, vocab] fp32
struct DecPass {
    // P > 1: prompt prefill — P positions of every utterance in ONE pass (whisper.mojo:195: the q_len = n_prompt block).  Rows are
    // position-major (row = t * B + b), tokens / positions come from tok_rows / pos_rows, K/V rows go to cache rows len + t, position
    // t sees keys 0..len+t (the causal mask of layers.mojo:309-318), logits only for the last position.  Every row's arithmetic is
    // what the single-position pass does for it, so the ids are the same bit for bit.
    int P = 1;
    int t0 = -1;        // t0 >= 0: a chunk of a per-row prefill — tokens / positions are rows [t0, t0 + P) of tok_rows / pos_rows
    bool embed = true;  // false: the input rows are in dx already (the greedy loop: written by the previous step's argmax launch)
    Logits logits = Logits::none;   // the final LN + vocabulary projection
    const float* mask = nullptr;    // additive logit mask of the fused argmax
    const TsRules* rules = nullptr;  // timestamp rules (null or tb <= 0: off)
    bool capture = false;           // a timestamp pass (al.on) also stores the alignment heads' cross-q rows
    bool key_window = true;         // false: no per-row key windows even on a per-row pass (the language pass, §19)
};
#pragma GCC visibility pop

#pragma GCC visibility push(hidden)

// ---- whisper_mi.cpp: errors and trace, states, the encoder, the decoder pass, the slot protocol (each commented where it is defined)
extern thread_local std::string g_err;
void trace_mark(hipStream_t st, const char* fmt, ...);
bool state_is_live(const void* s);
int dec_lanes_for(int B);
int run_encoder(wm_model* m, wm_state* s, const float* mel_dev, int B, hipStream_t st, const float* mel2, int split_at, bool want_f32);
int check_state(wm_model* m, wm_state* s, int B);
VocabHead vocab_head(const wm_model* m);
int cross_attn_merge(wm_model* m, wm_state* s, int l, const DecView& v, int P, void* out, int out_dtype);
int launch_cross_attn(wm_model* m, wm_state* s, int l, const DecView& v, int P);
// the decoder blocks that wm_bench_kernel's developer chains time one at a time
DecLinearParams qkv_block(wm_model* m, wm_state* s, const DecView& v, int l, int P);
DecLinearParams proj_residual_block(wm_model* m, wm_state* s, const DecView& v, int P, const float* in, int K, const DevBuf& W, const DevBuf& bias);
int decode_core(wm_model* m, wm_state* s, const DecView& v, const DecPass& a);
int check_opts(wm_model* m, const wm_decode_opts* o, int B);
int submit_on(wm_model* m, wm_state** slot, const PassAsk& ask);
int wait_on(wm_model* m, wm_state* s, int row0, int rows, const PassOut& out);
wm_state** slot_state(wm_model* m, int slot);
int flush_held(wm_model* m);
int run_now(wm_model* m, PassAsk ask, const PassOut& out);
int submit_slot(wm_model* m, int slot, const PassAsk& asked);
int collect_slot(wm_model* m, int slot, PassKind kind, const PassOut& out);
int align_cols(wm_model* m, const int32_t* n_frames, int B, std::vector<int32_t>& cols);
int rows_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* prompts, const int32_t* prompt_len, int prompt_stride,
               wm_decode_opts& o2, RowPrompts& rows);
int lang_entry(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
               const int32_t* prompt_len, int prompt_stride, bool lp, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
               const PassOut& out);
// ---- wm_align.cpp
int align_buffers(wm_model* m, wm_state* s, size_t Lr, size_t times_stride);
int align_setup(wm_model* m, wm_state* s, const wm_decode_opts* o, const std::vector<int32_t>* cols, const WinAsk* win);
int enqueue_align(wm_model* m, wm_state* s);
// ---- wm_frontend.cpp
int frontend_init(wm_model* m);
int frontend_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride);
int frontend_compute(wm_model* m, int B, float* mel_out);
int frontend_long_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int32_t* n_frames_out);
// ---- wm_score.cpp
int score_pass(wm_model* m, wm_state* s, const ScoreAsk& a);
int score_collect(wm_model* m, wm_state* s, const PassOut& out);
// ---- wm_long.cpp
void long_release(wm_model* m);

#pragma GCC visibility pop
