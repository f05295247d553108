// whisper_mi.cpp — host runtime behind the C-ABI of include/whisper_mi.h (compiled with hipcc).
//
// One wm_model per GPU: weights resident in HBM in kernel-friendly layouts, one HIP stream, no per-op allocation
// (the reference zero-fills a fresh heap Tensor for every intermediate, whisper_tensor.mojo:17-23; here every
// buffer belongs to a preallocated per-state arena).  The greedy loop of Whisper.transcribe (whisper.mojo:184-223)
// runs with the token feedback entirely on the device.
#include "../../include/whisper_mi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <set>
#include <thread>
#include <string>
#include <unordered_set>
#include <vector>

#include "wm_host.h"

using namespace wm;

// ------------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

extern "C" const char* wm_last_error(void) { return g_err.c_str(); }
extern "C" int wm_abi_version(void) { return WM_ABI_VERSION; }

int launch_rc(int st) {
    if (st == wm::WM_LAUNCH_OK) return 0;
    return fail(st == wm::WM_LAUNCH_HIP ? WM_E_HIP : WM_E_ARG, "%s", wm::launch_last_refusal());
}

// Developer timeline (WM_TRACE_EVENTS=1): HIP events recorded on the library's streams at pass / phase boundaries and
// printed, sorted on the GPU clock, when the model is freed.  The profiler serialises concurrent queues; events do not.
struct TraceMark {
    hipEvent_t ev;
    std::string label;
};
static std::vector<TraceMark> g_trace;
static bool trace_events_on() {
    static const bool on = wm_env("WM_TRACE_EVENTS") != nullptr;
    return on;
}
static void trace_mark(hipStream_t st, const char* fmt, ...) {
    if (!trace_events_on() || g_trace.size() > 200000) return;
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    g_trace.push_back({e, buf});
}
static void trace_dump() {
    if (g_trace.empty()) return;
    (void)hipDeviceSynchronize();
    std::vector<std::pair<float, std::string>> rows;
    for (auto& t : g_trace) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, g_trace[0].ev, t.ev);
        if (e == hipSuccess)
            rows.push_back({ms, t.label});
        else
            fprintf(stderr, "[wm-trace] %s: %s\n", t.label.c_str(), hipGetErrorString(e));
    }
    for (auto& t : g_trace) (void)hipEventDestroy(t.ev);
    g_trace.clear();
    std::sort(rows.begin(), rows.end());
    for (auto& r : rows) fprintf(stderr, "[wm-trace] %10.3f ms  %s\n", r.first, r.second.c_str());
}

static int dec_dtype(const wm_config& c) { return c.decoder_fp32 ? WM_F32 : c.compute_dtype; }  // operand dtype of the decoder

static int grow(DevBuf& b, size_t bytes) { return b.p && b.bytes >= bytes ? 0 : b.alloc(bytes); }

int upload(DevBuf& b, const float* h, size_t n, int dt) {
    WMCHK(b.alloc(n * dt_size(dt)));
    if (dt == WM_F32) {
        HIPCHK(hipMemcpy(b.p, h, n * 4, hipMemcpyHostToDevice));
    } else {
        std::vector<uint16_t> tmp(n);
        if (dt == WM_BF16)
            for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_bf16_host(h[i]);
        else
            for (size_t i = 0; i < n; ++i) tmp[i] = f32_to_f16_host(h[i]);
        HIPCHK(hipMemcpy(b.p, tmp.data(), n * 2, hipMemcpyHostToDevice));
    }
    return 0;
}

// Every live wm_state: a handle that is not in here (already freed — e.g. by wm_model_free, which owns the states created
// on it — or never valid) is rejected instead of dereferenced.
static std::mutex g_states_mu;
static std::unordered_set<const void*> g_live_states;
static bool state_is_live(const void* s) {
    std::lock_guard<std::mutex> lk(g_states_mu);
    return s && g_live_states.count(s) != 0;
}

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
};
struct WinAsk {  // the windows a long-form timestamp pass decodes
    const int32_t* items;  // device [B][3]: (utterance, seek, frames) per row
    int n_real;            // rows [n_real, B) repeat row 0: no align rows, zero times
};
struct RepeatAsk {  // the logits processors of a greedy pass, as wm_set_repeat_options / wm_set_sequence_bias left them when the pass was asked for
    float penalty = 1.f;
    int ngram = 0;
    std::shared_ptr<const SeqTable> sb;  // sequence bias / bad words: null = off
    int sb_gen() const { return sb ? sb->gen : 0; }
    bool on() const { return penalty != 1.f || ngram > 0 || sb; }
    bool operator==(const RepeatAsk& o) const { return penalty == o.penalty && ngram == o.ngram && sb_gen() == o.sb_gen(); }
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
    double* win_times = nullptr;  // a window pass (PassAsk::win): [B][max_loop + 1] times of the generated ids, offset included
};
enum class PassKind { transcribe, score, align };  // which wait family collects a slot's pass

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
    int top_k = 0;     // wm_set_top_k: what every log-prob pass asked for from now on carries (a held submit keeps its own)
    struct AlignRef {  // where a slot's last timestamp pass left its alignment weights (wm_alignment_weights)
        wm_state* st = nullptr;
        int row0 = 0, rows = 0, gen = 0;
    } align_ref[8];
    struct TopkRef {  // where a slot's last collected log-prob pass left its top-k tables (wm_transcribe_top_k)
        wm_state* st = nullptr;
        int row0 = 0, rows = 0, total = 0, k = 0, gen = 0;
    } topk_ref[8];
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
        int top_k = 0;                  // top-k alternatives (tk.k): the logits store, the argmax instantiation and the selection launch
        bool operator==(const StepKey& o) const {
            return eot == o.eot && ignore_eot == o.ignore_eot && rules.tb == o.rules.tb && rules.eos == o.rules.eos &&
                   rules.max_init == o.rules.max_init && rules.vocab == o.rules.vocab && shares_chip == o.shares_chip && cap == o.cap &&
                   rows == o.rows && lp == o.lp && rp == o.rp && sb == o.sb && top_k == o.top_k;
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
};

// ------------------------------------------------------------------------------------------------------------
// C = LN(x) W^T (+ epilogue of p): p.A names the scratch for the normalised rows.  The A-stationary GEMM normalises the fp32 rows
// while it loads them (no LayerNorm launch, no 16-bit copy through HBM); every other shape runs layernorm_rows first.
int ln_then_gemm(int dt_in, int dt_out, GemmParams p, const float* x, const float* g, const float* b, hipStream_t st) {
    if (gemm_nt_fuses_layernorm(dt_in == WM_F32 ? 4 : 2, p, 1)) {
        p.A = x;
        p.ln_g = g;
        p.ln_b = b;
    } else {
        DISPATCH_DT(dt_in, TT, launch_layernorm_rows<TT>(x, g, b, const_cast<void*>(p.A), nullptr, p.M, p.K, 1e-5f, st));
    }
    return gemm_dispatch(dt_in, dt_out, p, 1, st);
}
// 0 or a WM_E_* status with wm_last_error set (a shape the kernels refuse: nothing was launched)
int gemm_dispatch(int dt_in, int dt_out, const GemmParams& p, int batch, hipStream_t st) {
    int rc;
    if (dt_in == WM_F32) {
        rc = launch_gemm_nt<float, float>(p, batch, st);
    } else if (dt_in == WM_BF16) {
        rc = dt_out == WM_F32 ? launch_gemm_nt<bf16, float>(p, batch, st) : launch_gemm_nt<bf16, bf16>(p, batch, st);
    } else {
        rc = dt_out == WM_F32 ? launch_gemm_nt<f16, float>(p, batch, st) : launch_gemm_nt<f16, f16>(p, batch, st);
    }
    return launch_rc(rc);
}

extern "C" size_t wm_weight_count(const wm_dims* c) { return wm_synth_count(c); }
extern "C" size_t wm_synth_weights(const wm_dims* dims, uint64_t seed, float* out) { return wm_synth_fill(dims, seed, out); }
extern "C" void wm_synth_mel_host(uint64_t seed, int n_mels, int n_frames, float* out) {
    wm_synth_mel(seed, n_mels, n_frames, out);
}

static int check_cfg(const wm_config* c) {
    const wm_dims& d = c->dims;
    if (d.d_model <= 0 || d.n_heads <= 0 || d.d_model != d.n_heads * 64)
        return fail(WM_E_ARG, "d_model must equal n_heads*64 (got %d, %d)", d.d_model, d.n_heads);
    // Whisper-small (d_model 768, 12 heads, ffn 3072) and Whisper-medium (d_model 1024, 16 heads, ffn 4096) are the two shapes past 8
    // heads: their cross-attention runs on the K/V cache (m->xattn stays <= 8 heads), their fc2 on the K-long form of the skinny linear
    // (launch_dec_linear_long)
    const bool small = d.d_model == 768 && d.n_heads == 12, medium = d.d_model == 1024 && d.n_heads == 16;
    if (d.n_heads > 8 && !small && !medium)
        return fail(WM_E_ARG, "n_heads > 8 not supported (except 12 heads at d_model 768 and 16 heads at d_model 1024)");
    if (d.d_model % 128 || d.ffn % 128) return fail(WM_E_ARG, "d_model and ffn must be multiples of 128");
    // what the decode kernels are instantiated for: the logits kernel keeps d_model/128 in {1, 3, 4, 6, 8} k-panels
    // (kernels_decoder.hip launch_dec_logits), the skinny linears split K/32 k-steps over <= 16 waves x <= 4 steps
    if (d.d_model != 128 && d.d_model != 384 && d.d_model != 512 && !small && !medium)
        return fail(WM_E_ARG, "d_model %d not supported (128, 384, 512, 768 or 1024)", d.d_model);
    if (small && d.ffn != 3072) return fail(WM_E_ARG, "ffn %d not supported (d_model 768 takes ffn 3072 only)", d.ffn);
    if (medium && d.ffn != 4096) return fail(WM_E_ARG, "ffn %d not supported (d_model 1024 takes ffn 4096 only)", d.ffn);
    // dec_linear_model_supports_k is what admits 3072 and 4096 (the K-long form of fc2); below d_model 768 the K-long form stays closed
    if (!dec_linear_model_supports_k(d.ffn) || (!small && !medium && d.ffn > 2048))
        return fail(WM_E_ARG, "ffn %d not supported (ffn/32 must split into <= 16 waves x <= 4 k-steps, ffn <= 2048; 3072 with d_model 768, 4096 with d_model 1024)", d.ffn);
    if ((d.n_layers * 2 * d.d_model) % 128) return fail(WM_E_ARG, "n_layers*2*d_model must be a multiple of 128");
    if (d.n_text_ctx > 512) return fail(WM_E_ARG, "n_text_ctx > 512 not supported");
    if (d.n_mels <= 0 || d.n_audio_ctx <= 0 || d.vocab <= 0 || d.n_layers <= 0) return fail(WM_E_ARG, "bad dims");
    if (c->compute_dtype < 0 || c->compute_dtype > 2) return fail(WM_E_ARG, "bad compute_dtype");
    if (!(c->kv_dtype == WM_F32 || c->kv_dtype == c->compute_dtype))
        return fail(WM_E_ARG, "kv_dtype must be WM_F32 or equal compute_dtype");
    if (c->decoder_fp32 != 0 && c->decoder_fp32 != 1) return fail(WM_E_ARG, "decoder_fp32 must be 0 or 1");
    if (c->coalesce < 0 || c->coalesce > 2) return fail(WM_E_ARG, "coalesce must be 0, 1 (both: off) or 2");
    if (c->max_batch <= 0) return fail(WM_E_ARG, "max_batch must be > 0");
    if (c->gelu_mode != 0 && c->gelu_mode != 1) return fail(WM_E_ARG, "bad gelu_mode");
    return 0;
}

// ---- model load: loader.mojo:10-27 + whisper.mojo:60-69,122-128 + layers.mojo:96-103,418-433 -------------------
struct Reader {
    const float* p;
    size_t off = 0;
    const float* take(size_t n) {
        const float* r = p + off;
        off += n;
        return r;
    }
};
struct AttnW {
    const float *q_w, *q_b, *k_w, *v_w, *v_b, *o_w, *o_b;
};
static AttnW read_attn(Reader& r, size_t d) {
    AttnW a;
    a.q_w = r.take(d * d);
    a.q_b = r.take(d);
    a.k_w = r.take(d * d);
    a.v_w = r.take(d * d);
    a.v_b = r.take(d);
    a.o_w = r.take(d * d);
    a.o_b = r.take(d);
    return a;
}
// [co][ci][3] -> [co][3][ci_pad]   (transpose_conv_weights, whisper_tensor.mojo:358-364, plus channel padding)
std::vector<float> conv_relayout(const float* w, int co, int ci, int cip) {
    std::vector<float> o((size_t)co * 3 * cip, 0.f);
    for (int a = 0; a < co; ++a)
        for (int c = 0; c < ci; ++c)
            for (int k = 0; k < 3; ++k) o[((size_t)a * 3 + k) * cip + c] = w[(size_t)a * ci * 3 + (size_t)c * 3 + k];
    return o;
}

extern "C" void wm_state_free(wm_state* s);

extern "C" void wm_model_free(wm_model* m) {
    if (m && trace_events_on()) {
        trace_dump();
        {
            const char* path = wm_env("WM_TRACE_EVENTS");
            if (m->ts_buf.p && path) {
                std::vector<long long> h((2u << 20) + 1);
                if (hipMemcpy(h.data(), m->ts_buf.p, h.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                    if (FILE* f = fopen(path, "w")) {
                        const long long n = std::min<long long>(h[0], 1ll << 20);
                        for (long long i = 0; i < n; ++i) fprintf(f, "%lld %lld %lld\n", h[1 + 2 * i] >> 8, h[1 + 2 * i] & 255, h[2 + 2 * i]);
                        fclose(f);
                    }
                }
            }
        }
    }
    if (!m) return;
    (void)hipSetDevice(m->device);
    if (m->pump.joinable()) {
        {
            std::lock_guard<std::mutex> lk(m->pump_mu);
            m->pump_quit = true;
        }
        m->pump_cv.notify_all();
        m->pump.join();
    }
    // the model owns every state created on it (pipeline slots and the caller's KVCaches): a handle the caller still holds
    // becomes stale — wm_state_free / wm_decode_step on it is a checked no-op / error, not a use after free
    while (!m->states.empty()) wm_state_free(*m->states.begin());
    {
        DevBuf* fb[] = {&m->fe.window, &m->fe.dft, &m->fe.fb, &m->fe.band, &m->fe.pcm, &m->fe.lens, &m->fe.frames, &m->fe.spec, &m->fe.logtmp, &m->fe.mel};
        for (DevBuf* b : fb) b->release();
        for (auto* r : m->fe.rs) {
            r->taps.release();
            r->span.release();
            delete r;
        }
        DevBuf* lb[] = {&m->lf.pcm, &m->lf.lens, &m->lf.frames, &m->lf.spec, &m->lf.part, &m->lf.mel, &m->lf.in_mel,
                        &m->lf.win[0], &m->lf.win[1], &m->lf.items[0], &m->lf.items[1]};
        for (DevBuf* b : lb) b->release();
    }
    DevBuf* top[] = {&m->conv1_w, &m->conv1_b, &m->conv2_w, &m->conv2_b, &m->enc_pos, &m->enc_ln_g, &m->enc_ln_b,
                     &m->tok_emb_f, &m->tok_emb_t, &m->dec_pos, &m->dec_ln_g, &m->dec_ln_b, &m->cross_kv_w, &m->cross_kv_b};
    for (DevBuf* b : top) b->release();
    for (EncLayer& l : m->enc) {
        DevBuf* bs[] = {&l.qkv_w, &l.qkv_b, &l.o_w, &l.o_b, &l.ln1_g, &l.ln1_b, &l.fc1_w, &l.fc1_b, &l.fc2_w, &l.fc2_b, &l.ln2_g, &l.ln2_b};
        for (DevBuf* b : bs) b->release();
    }
    for (DecLayer& l : m->dec) {
        DevBuf* bs[] = {&l.sqkv_w, &l.sqkv_b, &l.so_w, &l.so_b, &l.ln1_g, &l.ln1_b, &l.cq_w, &l.cq_b, &l.co_w, &l.co_b,
                        &l.lnx_g, &l.lnx_b, &l.fc1_w, &l.fc1_b, &l.fc2_w, &l.fc2_b, &l.ln2_g, &l.ln2_b};
        for (DevBuf* b : bs) b->release();
    }
    if (m->stream) (void)hipStreamDestroy(m->stream);
    delete m;
}

static int model_build(wm_model* m, const float* w) {
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, f = c.ffn;
    const int T = m->cfg.compute_dtype;  // encoder-side operands (incl. the cross-K/V projection of the encoder output)
    const int TD = dec_dtype(m->cfg);    // decoder-side operands
    Reader r{w};
    m->Cp = (c.n_mels + 31) / 32 * 32;
    m->Vpad = (c.vocab + 15) / 16 * 16;
    {
        // conv1 as implicit GEMM: K = 3*Cp, rounded up to a multiple of 64 with zero weights (the extra window elements
        // read the start of the next token row and are multiplied by 0) so the 16-bit path takes the LDS-staged kernel
        auto c1r = conv_relayout(r.take(d * c.n_mels * 3), c.d_model, c.n_mels, m->Cp);
        m->K1 = (3 * m->Cp + 63) / 64 * 64;
        std::vector<float> c1((size_t)c.d_model * m->K1, 0.f);
        for (int a = 0; a < c.d_model; ++a) memcpy(&c1[(size_t)a * m->K1], &c1r[(size_t)a * 3 * m->Cp], (size_t)3 * m->Cp * 4);
        WMCHK(upload(m->conv1_w, c1.data(), c1.size(), T));
        WMCHK(upload(m->conv1_b, r.take(d), d, WM_F32));
        auto c2 = conv_relayout(r.take(d * d * 3), c.d_model, c.d_model, c.d_model);
        WMCHK(upload(m->conv2_w, c2.data(), c2.size(), T));
        WMCHK(upload(m->conv2_b, r.take(d), d, WM_F32));
        WMCHK(upload(m->enc_pos, r.take((size_t)c.n_audio_ctx * d), (size_t)c.n_audio_ctx * d, WM_F32));
    }
    std::vector<float> qkv(3 * d * d), qkvb(3 * d);
    auto pack_qkv = [&](const AttnW& a) {
        memcpy(qkv.data(), a.q_w, d * d * 4);
        memcpy(qkv.data() + d * d, a.k_w, d * d * 4);
        memcpy(qkv.data() + 2 * d * d, a.v_w, d * d * 4);
        memcpy(qkvb.data(), a.q_b, d * 4);
        memset(qkvb.data() + d, 0, d * 4);  // k_proj has no bias (layers.mojo:96-103)
        memcpy(qkvb.data() + 2 * d, a.v_b, d * 4);
    };
    m->enc.resize(c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) {
        EncLayer& l = m->enc[i];
        AttnW a = read_attn(r, d);
        pack_qkv(a);
        WMCHK(upload(l.qkv_w, qkv.data(), qkv.size(), T));
        WMCHK(upload(l.qkv_b, qkvb.data(), qkvb.size(), WM_F32));
        WMCHK(upload(l.o_w, a.o_w, d * d, T));
        WMCHK(upload(l.o_b, a.o_b, d, WM_F32));
        WMCHK(upload(l.ln1_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln1_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.fc1_w, r.take(f * d), f * d, T));
        WMCHK(upload(l.fc1_b, r.take(f), f, WM_F32));
        WMCHK(upload(l.fc2_w, r.take(d * f), d * f, T));
        WMCHK(upload(l.fc2_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_b, r.take(d), d, WM_F32));
    }
    WMCHK(upload(m->enc_ln_g, r.take(d), d, WM_F32));
    WMCHK(upload(m->enc_ln_b, r.take(d), d, WM_F32));
    {
        const float* te = r.take((size_t)c.vocab * d);
        WMCHK(upload(m->tok_emb_f, te, (size_t)c.vocab * d, WM_F32));
        if (TD != WM_F32) WMCHK(upload(m->tok_emb_t, te, (size_t)c.vocab * d, TD));
        WMCHK(upload(m->dec_pos, r.take((size_t)c.n_text_ctx * d), (size_t)c.n_text_ctx * d, WM_F32));
    }
    std::vector<float> ckv((size_t)c.n_layers * 2 * d * d), ckvb((size_t)c.n_layers * 2 * d, 0.f);
    m->dec.resize(c.n_layers);
    for (int i = 0; i < c.n_layers; ++i) {
        DecLayer& l = m->dec[i];
        AttnW a = read_attn(r, d);
        pack_qkv(a);
        WMCHK(upload(l.sqkv_w, qkv.data(), qkv.size(), TD));
        WMCHK(upload(l.sqkv_b, qkvb.data(), qkvb.size(), WM_F32));
        WMCHK(upload(l.so_w, a.o_w, d * d, TD));
        WMCHK(upload(l.so_b, a.o_b, d, WM_F32));
        WMCHK(upload(l.ln1_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln1_b, r.take(d), d, WM_F32));
        AttnW x = read_attn(r, d);
        WMCHK(upload(l.cq_w, x.q_w, d * d, TD));
        WMCHK(upload(l.cq_b, x.q_b, d, WM_F32));
        memcpy(ckv.data() + (size_t)(2 * i) * d * d, x.k_w, d * d * 4);
        memcpy(ckv.data() + (size_t)(2 * i + 1) * d * d, x.v_w, d * d * 4);
        memcpy(ckvb.data() + (size_t)(2 * i + 1) * d, x.v_b, d * 4);
        WMCHK(upload(l.co_w, x.o_w, d * d, TD));
        WMCHK(upload(l.co_b, x.o_b, d, WM_F32));
        WMCHK(upload(l.lnx_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.lnx_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.fc1_w, r.take(f * d), f * d, TD));
        WMCHK(upload(l.fc1_b, r.take(f), f, WM_F32));
        WMCHK(upload(l.fc2_w, r.take(d * f), d * f, TD));
        WMCHK(upload(l.fc2_b, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_g, r.take(d), d, WM_F32));
        WMCHK(upload(l.ln2_b, r.take(d), d, WM_F32));
    }
    WMCHK(upload(m->dec_ln_g, r.take(d), d, WM_F32));
    WMCHK(upload(m->dec_ln_b, r.take(d), d, WM_F32));
    WMCHK(upload(m->cross_kv_w, ckv.data(), ckv.size(), T));
    WMCHK(upload(m->cross_kv_b, ckvb.data(), ckvb.size(), WM_F32));
    if (const char* tr = wm_env("WM_TRACE_EVENTS"); tr && strchr(tr, '/')) WMCHK(m->ts_buf.alloc(((2u << 20) + 1) * 8, true));
    if (r.off != wm_synth_count(&c)) return fail(WM_E_SIZE, "internal: consumed %zu floats, expected %zu", r.off, wm_synth_count(&c));
    return 0;
}

extern "C" int wm_model_load_memory(const float* weights, size_t n_floats, const wm_config* cfg, int device, wm_model** out) {
    if (!weights || !cfg || !out) return fail(WM_E_ARG, "null argument");
    WMCHK(check_cfg(cfg));
    const size_t want = wm_synth_count(&cfg->dims);
    if (n_floats != want)
        return fail(WM_E_SIZE, "weight image holds %zu floats (%zu bytes), this config needs %zu (%zu bytes)", n_floats,
                    n_floats * 4, want, want * 4);
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(WM_E_ARG, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
    wm_model* m = new wm_model();
    m->cfg = *cfg;
    m->device = device;
    if (const char* e = wm_env("WM_ENC_CHUNK")) m->enc_chunk = std::max(1, atoi(e));
    m->xattn = cfg->compute_dtype == WM_BF16 && cfg->kv_dtype == WM_F32 && cfg->dims.n_heads <= 8 &&
               cfg->dims.d_model == 64 * cfg->dims.n_heads && !wm_env("WM_XATTN_OFF");
    hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete m;
        return fail(WM_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    int rc = model_build(m, weights);
    if (rc) {
        std::string keep = g_err;
        wm_model_free(m);
        g_err = keep;
        return rc;
    }
    *out = m;
    return 0;
}

// ---- weight file formats ------------------------------------------------------------------------------------------
// v1: the reference's headerless fp32 dump (export_weights.py:19-90; loader.mojo reads it with no size check).
// v2: 64-byte header {magic "WMIWGT2", version, matrix dtype, dims, flags, payload bytes} + the same
// tensors in the same order; conv / linear matrices (and, unless flag bit 0 is set, the token embedding) stored in the
// matrix dtype, every vector and positional table in fp32.  Loading v2 expands to the fp32 image the builder takes, so a
// v2 file in the model's compute dtype gives bit-identical weights to the v1 file (16-bit rounding is idempotent).
struct WmV2Header {
    char magic[8];
    uint32_t version, matrix_dtype;
    int32_t dims[8];
    uint32_t flags, reserved;
    uint64_t payload_bytes;
};
static_assert(sizeof(WmV2Header) == 64, "v2 header is 64 bytes");
static const char WM_V2_MAGIC[8] = {'W', 'M', 'I', 'W', 'G', 'T', '2', '\0'};
enum { WM_V2_EMB_F32 = 1 };

struct TensorSpan {
    int kind;
    size_t count;
};
static void collect_tensor(void* user, int, int kind, size_t count) { ((std::vector<TensorSpan>*)user)->push_back({kind, count}); }
static bool v2_is_matrix(int kind, uint32_t flags) { return kind == WM_K_WEIGHT || kind == WM_K_QK || (kind == WM_K_EMB && !(flags & WM_V2_EMB_F32)); }
static size_t v2_payload_bytes(const wm_dims* d, int dtype, uint32_t flags) {
    std::vector<TensorSpan> t;
    wm_synth_walk(d, collect_tensor, &t);
    size_t n = 0;
    for (auto& s : t) n += s.count * (v2_is_matrix(s.kind, flags) ? dt_size(dtype) : 4);
    return n;
}
static inline float bf16_to_f32_host(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static inline float f16_to_f32_host(uint16_t h) {
    _Float16 x;
    memcpy(&x, &h, 2);
    return (float)x;
}

extern "C" int wm_weights_convert_v2(const char* v1_path, const char* v2_path, const wm_dims* dims, int dtype, int emb_f32) {
    if (!v1_path || !v2_path || !dims || dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad argument");
    const size_t n = wm_synth_count(dims);
    FILE* f = fopen(v1_path, "rb");
    if (!f) return fail(WM_E_IO, "cannot open %s", v1_path);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (sz < 0 || (size_t)sz != n * 4) {
        fclose(f);
        return fail(WM_E_SIZE, "%s is %ld bytes, these dims need %zu", v1_path, sz, n * 4);
    }
    std::vector<float> w(n);
    const size_t got = fread(w.data(), 4, n, f);
    fclose(f);
    if (got != n) return fail(WM_E_IO, "short read on %s", v1_path);
    WmV2Header h{};
    memcpy(h.magic, WM_V2_MAGIC, 8);
    h.version = 2;
    h.matrix_dtype = (uint32_t)dtype;
    memcpy(h.dims, dims, sizeof h.dims);
    h.flags = emb_f32 ? WM_V2_EMB_F32 : 0;
    h.payload_bytes = v2_payload_bytes(dims, dtype, h.flags);
    FILE* o = fopen(v2_path, "wb");
    if (!o) return fail(WM_E_IO, "cannot create %s", v2_path);
    bool ok = fwrite(&h, sizeof h, 1, o) == 1;
    std::vector<TensorSpan> t;
    wm_synth_walk(dims, collect_tensor, &t);
    size_t off = 0;
    std::vector<uint16_t> tmp;
    for (auto& s : t) {
        if (v2_is_matrix(s.kind, h.flags) && dtype != WM_F32) {
            tmp.resize(s.count);
            for (size_t i = 0; i < s.count; ++i) tmp[i] = dtype == WM_BF16 ? f32_to_bf16_host(w[off + i]) : f32_to_f16_host(w[off + i]);
            ok = ok && fwrite(tmp.data(), 2, s.count, o) == s.count;
        } else {
            ok = ok && fwrite(w.data() + off, 4, s.count, o) == s.count;
        }
        off += s.count;
    }
    ok = (fclose(o) == 0) && ok;
    return ok ? 0 : fail(WM_E_IO, "write error on %s", v2_path);
}

// Reads a v1 or v2 file into an fp32 image of wm_weight_count(dims) floats, validating size / header against dims.
extern "C" int wm_weights_read(const char* path, const wm_dims* dims, float* out) {
    if (!path || !dims || !out) return fail(WM_E_ARG, "null argument");
    const size_t n = wm_synth_count(dims);
    FILE* f = fopen(path, "rb");
    if (!f) return fail(WM_E_IO, "cannot open %s", path);
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    WmV2Header h{};
    const bool v2 = sz >= (long)sizeof h && fread(&h, sizeof h, 1, f) == 1 && memcmp(h.magic, WM_V2_MAGIC, 8) == 0;
    if (!v2) {
        fseek(f, 0, SEEK_SET);
        if (sz < 0 || (size_t)sz != n * 4) {
            fclose(f);
            return fail(WM_E_SIZE, "%s is %ld bytes, this config needs %zu", path, sz, n * 4);
        }
        const size_t got = fread(out, 4, n, f);
        fclose(f);
        return got == n ? 0 : fail(WM_E_IO, "short read on %s", path);
    }
    int rc = 0;
    if (h.version != 2 || h.matrix_dtype > 2)
        rc = fail(WM_E_SIZE, "%s: unsupported v2 header (version %u, dtype %u)", path, h.version, h.matrix_dtype);
    else if (memcmp(h.dims, dims, sizeof h.dims) != 0)
        rc = fail(WM_E_SIZE, "%s was written for other dims (d_model %d, layers %d, vocab %d)", path, h.dims[0], h.dims[2], h.dims[7]);
    else if (h.payload_bytes != v2_payload_bytes(dims, (int)h.matrix_dtype, h.flags) || (size_t)sz != sizeof h + h.payload_bytes)
        rc = fail(WM_E_SIZE, "%s: payload size does not match its header", path);
    if (!rc) {
        std::vector<TensorSpan> t;
        wm_synth_walk(dims, collect_tensor, &t);
        size_t off = 0;
        std::vector<uint16_t> tmp;
        for (auto& s : t) {
            if (v2_is_matrix(s.kind, h.flags) && h.matrix_dtype != WM_F32) {
                tmp.resize(s.count);
                if (fread(tmp.data(), 2, s.count, f) != s.count) {
                    rc = fail(WM_E_IO, "short read on %s", path);
                    break;
                }
                for (size_t i = 0; i < s.count; ++i) out[off + i] = h.matrix_dtype == WM_BF16 ? bf16_to_f32_host(tmp[i]) : f16_to_f32_host(tmp[i]);
            } else if (fread(out + off, 4, s.count, f) != s.count) {
                rc = fail(WM_E_IO, "short read on %s", path);
                break;
            }
            off += s.count;
        }
    }
    fclose(f);
    return rc;
}

extern "C" int wm_model_load(const char* path, const wm_config* cfg, int device, wm_model** out) {
    if (!path || !cfg || !out) return fail(WM_E_ARG, "null argument");
    WMCHK(check_cfg(cfg));
    std::vector<float> buf(wm_synth_count(&cfg->dims));
    WMCHK(wm_weights_read(path, &cfg->dims, buf.data()));
    return wm_model_load_memory(buf.data(), buf.size(), cfg, device, out);
}

// ---- state ---------------------------------------------------------------------------------------------------
extern "C" void wm_state_free(wm_state* s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_states_mu);
        if (!g_live_states.erase(s)) return;  // stale handle: its model was freed (and took the state with it)
    }
    {  // the loop pump must not touch this state any more (it works under this mutex)
        std::lock_guard<std::mutex> lk(s->m->pump_mu);
        auto& wq = s->m->pump_work;
        wq.erase(std::remove(wq.begin(), wq.end(), s), wq.end());
    }
    s->m->states.erase(s);
    if (s->m->cached == s) s->m->cached = nullptr;
    for (auto& sl : s->m->slots)
        if (sl == s) sl = nullptr;
    for (auto& pr : s->m->pairs)
        if (pr == s) pr = nullptr;
    for (auto& ls : s->m->lf.st)
        if (ls == s) ls = nullptr;
    for (auto& r : s->m->slot_ref)
        if (r.st == s) r = wm_model::SlotRef{};
    for (auto& r : s->m->align_ref)
        if (r.st == s) r = wm_model::AlignRef{};
    for (auto& r : s->m->topk_ref)
        if (r.st == s) r = wm_model::TopkRef{};
    (void)hipSetDevice(s->m->device);
    // nothing of this state may still be running when its graphs, streams and arenas go away (a submitted pass that was
    // never waited for, or the model stream's last wm_decode_step)
    for (auto& ln : s->lanes)
        if (ln.st) (void)hipStreamSynchronize(ln.st);
    if (s->m->stream) (void)hipStreamSynchronize(s->m->stream);
    for (auto& ln : s->lanes) {
        for (auto& g : ln.graph)
            if (g) (void)hipGraphExecDestroy(g);
        if (ln.st) (void)hipStreamDestroy(ln.st);
        if (ln.done) (void)hipEventDestroy(ln.done);
    }
    if (s->enc_done) (void)hipEventDestroy(s->enc_done);
    for (auto& ev : s->sc.ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : s->chunk_ev)
        if (ev) (void)hipEventDestroy(ev);
    if (s->h_prog) (void)hipHostFree((void*)s->h_prog);
    DevBuf* bs[] = {&s->mel_dev, &s->mel_t, &s->h1, &s->x, &s->xn, &s->qkv, &s->ao, &s->hid, &s->enc_t, &s->enc_f,
                    &s->cross_kv, &s->enc_x, &s->xq, &s->part_y, &s->self_kv, &s->dx, &s->dq, &s->dattn, &s->dhid, &s->part_o, &s->part_ml, &s->logits, &s->amax_val, &s->amax_idx, &s->ts_state, &s->ts_val, &s->ts_idx, &s->ts_m, &s->ts_s, &s->mask_steady, &s->mask_begin,
                    &s->tok, &s->pos, &s->tok_rows, &s->pos_rows, &s->ctl, &s->out_tokens, &s->n_tokens, &s->finished,
                    &s->al.cap, &s->al.kh, &s->al.probs, &s->al.mean, &s->al.stdv, &s->al.M, &s->al.trace, &s->al.times, &s->al.ncols,
                    &s->al.rows, &s->al.row0, &s->al.map, &s->sc.rows, &s->sc.a, &s->sc.pmax, &s->sc.psum, &s->sc.pidx, &s->sc.ztgt, &s->sc.target,
                    &s->sc.slot, &s->sc.dst, &s->sc.len, &s->sc.ctx, &s->sc.lp, &s->sc.top, &s->sc.sum, &s->sc.avg,
                    &s->rw.table, &s->rw.len, &s->rw.key_lo, &s->lp.part_s, &s->lp.table, &s->lp.sum, &s->tk.rows, &s->tk.ids, &s->tk.lps,
                    &s->ns.x, &s->ns.pmax, &s->ns.pidx, &s->ns.psum, &s->ns.prob, &s->ns.lse,
                    &s->lg.x, &s->lg.ids, &s->lg.col, &s->lg.out, &s->lg.probs, &s->rp.seen, &s->rp.ban, &s->rp.ctl, &s->rp.hit, &s->rp.val, &s->rp.sbctl};
    for (DevBuf* b : bs) b->release();
    delete s;
}

static const int OUT_STRIDE_MAX = 1024;

static int state_new(wm_model* m, int B, wm_state** out, bool pair);
// decode lanes a state of B utterances gets (1 unless the developer build's WM_DEC_LANES asks for more)
static int dec_lanes_for(int B) {
    int nl = 1;
    if (const char* e = wm_env("WM_DEC_LANES")) nl = std::max(1, std::min(4, atoi(e)));
    return std::min(nl, (B + 15) / 16);
}
extern "C" int wm_state_new(wm_model* m, int B, wm_state** out) { return state_new(m, B, out, false); }
// pair: the 2·B-row state of a coalesced pair of submits (B <= max_batch each)
static int state_new(wm_model* m, int B, wm_state** out, bool pair) {
    if (!m || !out || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch * (pair ? 2 : 1)) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    HIPCHK(hipSetDevice(m->device));
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, L = 2 * (size_t)c.n_audio_ctx, T = c.n_audio_ctx;
    const size_t ts = dt_size(m->cfg.compute_dtype), ks = dt_size(m->cfg.kv_dtype);
    wm_state* s = new wm_state();
    s->m = m;
    s->B = B;
    {
        std::lock_guard<std::mutex> lk(g_states_mu);
        g_live_states.insert(s);
    }
    m->states.insert(s);
    s->Bc = std::min(pair ? B / 2 : B, m->enc_chunk);  // (pair: an encoder chunk never straddles the two batches)
    // key chunks per utterance for the cross-attention kernel: a function of the MODEL's max_batch, never of this call's
    // B, so that an utterance's result does not depend on how it was batched (bitwise batch invariance within a model).
    // Aim for 1024 workgroups at full batch (4 per CU, one full round): 16 chunks at max_batch 64 (measured, µs per launch /
    // per whole step: 12 chunks 26.4 / 280, 16: 25.2 / 273, 20: 25.5 / 278, 24: 26.4 / 278), up to 48 for small-batch /
    // latency models (B = 1: 12.1 -> 4 us per launch).  WM_NSPLIT overrides for tuning.
    {
        const int min_split = (int)((T + 511) / 512);
        // fp32 K/V rows are twice as wide: half the chunks move the same bytes per workgroup, the stream runs as fast (46.6 vs 46.5 us
        // per launch at B = 64) and the merge reads half the partials (decode step 406 -> 402 us; 10 / 12 chunks: 418 / 412 us)
        const int target = ks == 4 ? 512 : 1024;
        int ns = (target + m->cfg.max_batch - 1) / m->cfg.max_batch;
        ns = std::max(ks == 4 ? 8 : 12, std::min(48, ns));
        ns = std::max(min_split, std::min(ns, (int)((T + 31) / 32)));
        if (m->xattn) {
            // absorbed cross-attention: a chunk carries fixed costs the K/V stream did not have (q' images into LDS, an H·d partial,
            // its share of the merge), so fewer, longer chunks: ~128 per max_batch rows, at least 64 keys (one tile per wave).
            // Measured, headline (128-row states), ms per 64-clip pass: 32 chunks 32.1, 24: 28.3, 16: 26.0, 8: 23.5, 6: 23.5,
            // 4: 22.3-22.5, 3: 21.8, 2: 21.4
            ns = (128 + m->cfg.max_batch - 1) / m->cfg.max_batch;
            ns = std::max(1, std::min({ns, 48, (int)T / 64}));
        }
        if (const char* e = wm_env("WM_NSPLIT")) ns = std::max(m->xattn ? 1 : min_split, std::min(64, atoi(e)));
        s->nsplit = ns;
    }
    s->out_stride = OUT_STRIDE_MAX;
    const size_t Bc = s->Bc;
    const size_t Mp = (Bc * T + 255) / 256 * 256 + 256;  // padded rows: tail tiles (up to 256 rows) read, never store, past M
    int rc = 0;
    auto A = [&](DevBuf& b, size_t bytes, bool zero = false) {
        if (!rc) rc = b.alloc(bytes, zero);
    };
    A(s->mel_dev, (size_t)B * c.n_mels * L * 4);
    A(s->mel_t, (Bc * (L + 2) + 256) * m->Cp * ts, true);
    A(s->h1, (Bc * (L + 2) + 256) * d * ts, true);  // rows 0 and L+1 of each utterance stay zero = conv padding
    A(s->x, Mp * d * 4, true);
    A(s->xn, Mp * d * ts, true);
    A(s->qkv, Mp * 3 * d * ts, true);
    A(s->ao, Mp * d * ts, true);
    A(s->hid, Mp * c.ffn * ts, true);
    A(s->enc_f, (size_t)B * T * d * 4);
    if (m->xattn) {  // X rows are written in place by the encoder's last LayerNorm: no chunk-sized operand buffer, no cross cache
        A(s->enc_x, (size_t)B * T * d * 2);
    } else {
        A(s->enc_t, Mp * d * ts, true);
        A(s->cross_kv, (size_t)c.n_layers * 2 * B * T * d * ks);
    }
    A(s->self_kv, (size_t)c.n_layers * 2 * B * c.n_text_ctx * d * ks, true);
    // decode activations: rows for one token per utterance, or — prompt prefill — for up to PREFILL_MAX positions at once
    const size_t R = (size_t)B * wm_state::PREFILL_MAX;
    A(s->dx, R * d * 4);
    A(s->dq, R * d * 4);
    A(s->dattn, R * d * 4);
    A(s->dhid, R * c.ffn * 4);
    if (m->xattn) {
        A(s->xq, R * 3 * c.n_heads * d * 2);
        A(s->part_y, R * s->nsplit * c.n_heads * d * 4);
    } else {
        A(s->part_o, R * s->nsplit * d * 4);
    }
    A(s->part_ml, R * s->nsplit * c.n_heads * 2 * 4);
    A(s->tok_rows, R * 4, true);
    A(s->pos_rows, R * 4, true);
    A(s->logits, (size_t)B * m->Vpad * 4);
    s->npart = dec_logits_parts(c.vocab);
    A(s->amax_val, (size_t)B * s->npart * 4);
    A(s->amax_idx, (size_t)B * s->npart * 4);
    A(s->ts_val, (size_t)B * s->npart * 4, true);
    A(s->ts_idx, (size_t)B * s->npart * 4, true);
    A(s->ts_m, (size_t)B * s->npart * 4, true);
    A(s->ts_s, (size_t)B * s->npart * 4, true);
    A(s->ts_state, (size_t)B * sizeof(TsState), true);
    A(s->mask_steady, (size_t)m->Vpad * 4, true);
    A(s->mask_begin, (size_t)m->Vpad * 4, true);
    A(s->tok, (size_t)B * 4, true);
    A(s->pos, (size_t)B * 4, true);
    A(s->ctl, sizeof(StepCtl) * 8, true);  // [0] whole-batch control (wm_decode_step), [1..] one per decode lane
    A(s->out_tokens, (size_t)B * s->out_stride * 4, true);
    A(s->n_tokens, (size_t)B * 4, true);
    A(s->finished, (size_t)B * 4, true);
    A(s->lp.part_s, (size_t)B * s->npart * 4, true);
    A(s->lp.table, (size_t)B * s->out_stride * 4, true);
    A(s->lp.sum, (size_t)B * 4, true);
    A(s->tk.rows, (size_t)B * sizeof(TopkRow), true);
    A(s->tk.ids, (size_t)B * s->out_stride * TOPK_MAX * 4, true);
    A(s->tk.lps, (size_t)B * s->out_stride * TOPK_MAX * 4, true);
    A(s->ns.x, (size_t)B * d * 4, true);
    A(s->ns.pmax, (size_t)B * s->npart * 4, true);
    A(s->ns.pidx, (size_t)B * s->npart * 4, true);
    A(s->ns.psum, (size_t)B * s->npart * 4, true);
    A(s->ns.prob, (size_t)B * 4, true);
    A(s->ns.lse, (size_t)B * 4, true);
    A(s->lg.x, (size_t)B * d * 4, true);
    A(s->lg.ids, (size_t)LANG_DETECT_MAX * 4, true);
    A(s->lg.col, (size_t)B * 4, true);
    A(s->lg.out, (size_t)B * 4, true);
    A(s->lg.probs, (size_t)B * LANG_DETECT_MAX * 4, true);
    if (rc) {
        std::string keep = g_err;
        wm_state_free(s);
        g_err = keep;
        return rc;
    }
    {  // decode lanes
        // measured on MI355X (round 1): 2 lanes 49.1 ms vs 1 lane 47.4 ms per 64-clip pass — kernel boundaries of one
        // queue also stall the other queue's kernels, so extra lanes stay opt-in (WM_DEC_LANES)
        const int nl = dec_lanes_for(B);
        s->lanes.resize(nl);
        const int per = ((B + nl - 1) / nl + 15) / 16 * 16;  // whole MFMA row blocks per lane
        int b0 = 0;
        for (int i = 0; i < nl; ++i) {
            wm_state::Lane& ln = s->lanes[i];
            ln.b0 = b0;
            ln.nb = std::max(0, std::min(per, B - b0));
            b0 += ln.nb;
            ln.ctl = s->ctl.as<StepCtl>() + 1 + i;
            // decode launches are latency-critical (34 dependent sub-5-us kernels per token); the encoder stream carries
            // throughput work.  WM_DEC_PRIORITY=1 puts the lane streams on the highest HIP stream priority.
            int lo_p = 0, hi_p = 0;
            (void)hipDeviceGetStreamPriorityRange(&lo_p, &hi_p);
            static const bool prio = wm_env("WM_DEC_PRIORITY") != nullptr;
            hipError_t e = prio ? hipStreamCreateWithPriority(&ln.st, hipStreamNonBlocking, hi_p)
                                : hipStreamCreateWithFlags(&ln.st, hipStreamNonBlocking);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.done, hipEventDisableTiming);
            if (e != hipSuccess) {
                wm_state_free(s);
                return fail(WM_E_HIP, "lane stream: %s", hipGetErrorString(e));
            }
        }
        while (!s->lanes.empty() && s->lanes.back().nb == 0) {
            (void)hipStreamDestroy(s->lanes.back().st);
            (void)hipEventDestroy(s->lanes.back().done);
            s->lanes.pop_back();
        }
        hipError_t e = hipEventCreateWithFlags(&s->enc_done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipHostMalloc((void**)&s->h_prog, 64, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&s->d_prog, (void*)s->h_prog, 0);
        for (auto& ev : s->chunk_ev)
            if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) {
            wm_state_free(s);
            return fail(WM_E_HIP, "event: %s", hipGetErrorString(e));
        }
    }
    *out = s;
    return 0;
}

extern "C" int wm_state_reset(wm_state* s) {
    if (!state_is_live(s)) return fail(WM_E_ARG, "null or stale state handle");
    HIPCHK(hipSetDevice(s->m->device));
    hipStream_t st = s->m->stream;
    HIPCHK(hipMemsetAsync(s->ctl.p, 0, s->ctl.bytes, st));
    HIPCHK(hipMemsetAsync(s->n_tokens.p, 0, s->n_tokens.bytes, st));
    HIPCHK(hipMemsetAsync(s->finished.p, 0, s->finished.bytes, st));
    s->has_enc = s->has_cross = false;
    s->host_len = 0;
    return 0;
}
extern "C" int wm_state_len(const wm_state* s) { return state_is_live(s) ? s->host_len : -1; }

// ---- encoder: whisper.mojo:71-99 ------------------------------------------------------------------------------------
static void* off_bytes(const DevBuf& b, size_t bytes) { return (char*)b.p + bytes; }

static int cross_kv_chunk(wm_model* m, wm_state* s, int c0, int bc, hipStream_t st) {
    // cross K/V for utterances [c0, c0+bc) from enc_t (rows 0..bc*T): layers.mojo:150-154, all layers in one GEMM
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, T = c.n_audio_ctx;
    GemmParams p{};
    p.A = s->enc_t.p;
    p.W = m->cross_kv_w.p;
    p.C = off_bytes(s->cross_kv, (size_t)c0 * T * d * dt_size(m->cfg.kv_dtype));
    p.M = (int)(bc * T);
    p.N = c.n_layers * 2 * c.d_model;
    p.K = c.d_model;
    p.lda = d;
    p.ldw = d;
    p.ldc = d;
    p.bias = m->cross_kv_b.as<float>();
    p.group_n = c.d_model;
    p.group_stride = (long)((size_t)s->B * T * d);
    return gemm_dispatch(m->cfg.compute_dtype, m->cfg.kv_dtype, p, 1, st);
}

// mel2 / split_at (coalesced pairs): utterances [split_at, B) come from mel2 (their own batch's buffer); split_at is a multiple of Bc
// want_f32: also produce the fp32 encoder output (s->enc_f, what wm_encode returns).  The decoder never reads it — the cross-K/V
// projection consumes the operand-dtype rows s->enc_t — so the transcribe paths skip it, and where the last fc2 can carry a
// LayerNorm in its epilogue (16-bit operands, d = 384) `ln_post` rides there: no LayerNorm launch, no 147 MB fp32 write per pass.
// BOTH kinds of caller take the operand rows from the same epilogue, so wm_encode + wm_decode_step and wm_transcribe see
// bit-identical cross-K/V (round 2 had fused it for the transcribe paths only and reverted: the two entry points parted at a near-tie).
static int run_encoder(wm_model* m, wm_state* s, const float* mel_dev, int B, hipStream_t st, const float* mel2, int split_at,
                       bool want_f32) {
    const wm_dims& c = m->cfg.dims;
    const int T = m->cfg.compute_dtype;
    const size_t d = c.d_model, L = 2 * (size_t)c.n_audio_ctx, NT = c.n_audio_ctx, ts = dt_size(T);
    for (int c0 = 0; c0 < B; c0 += s->Bc) {
        const int bc = std::min(s->Bc, B - c0);
        const int M = (int)(bc * NT);
        const int opb = T == WM_F32 ? 4 : 2;
        bool xn_is_ln1 = false;  // xn holds LN1(x) of the coming block, written by the epilogue of the GEMM that produced x
        bool post_fused = false;  // enc_t was written by the last fc2's epilogue
        // operand rows of ln_post: the chunk-sized enc_t that the cross-K/V projection consumes, or (m->xattn) this chunk's rows
        // of the state's X, which the decoder's cross-attention streams itself
        void* post_rows = m->xattn ? off_bytes(s->enc_x, (size_t)c0 * NT * d * 2) : s->enc_t.p;
        const float* mel_c = (mel2 && c0 >= split_at) ? mel2 + (size_t)(c0 - split_at) * c.n_mels * L : mel_dev + (size_t)c0 * c.n_mels * L;
        DISPATCH_DT(T, TT, launch_mel_transpose_pad<TT>(mel_c, s->mel_t.p, bc, c.n_mels, (int)L, m->Cp, st));
        {  // conv1 + GELU -> h1 rows 1..L (token-major)   whisper.mojo:73-75
            GemmParams p{};
            p.A = s->mel_t.p;
            p.W = m->conv1_w.p;
            p.C = off_bytes(s->h1, d * ts);
            p.M = (int)L;
            p.N = c.d_model;
            p.K = m->K1;
            p.lda = m->Cp;
            p.ldw = m->K1;
            p.ldc = d;
            p.strideA = (long)((L + 2) * m->Cp);
            p.strideC = (long)((L + 2) * d);
            p.bias = m->conv1_b.as<float>();
            p.act = 1;
            p.gelu_mode = m->cfg.gelu_mode;
            WMCHK(gemm_dispatch(T, T, p, bc, st));
        }
        {  // conv2 (stride 2) + GELU + pos_emb -> x   whisper.mojo:78-89
            GemmParams p{};
            p.A = s->h1.p;
            p.W = m->conv2_w.p;
            p.C = s->x.p;
            p.M = (int)NT;
            p.N = c.d_model;
            p.K = 3 * c.d_model;
            p.lda = 2 * d;
            p.ldw = 3 * d;
            p.ldc = d;
            p.strideA = (long)((L + 2) * d);
            p.strideC = (long)(NT * d);
            p.bias = m->conv2_b.as<float>();
            p.act = 1;
            p.gelu_mode = m->cfg.gelu_mode;
            p.pos = m->enc_pos.as<float>();
            if (gemm_nt_fuses_layernorm_out(opb, p)) {  // the first block's LN1 rides conv2's epilogue
                p.lno_g = m->enc[0].ln1_g.as<float>();
                p.lno_b = m->enc[0].ln1_b.as<float>();
                p.lno_out = s->xn.p;
                xn_is_ln1 = true;
            }
            WMCHK(gemm_dispatch(T, WM_F32, p, bc, st));
        }
        for (int l = 0; l < c.n_layers; ++l) {  // layers.mojo:435-519 with is_decoder=False
            EncLayer& w = m->enc[l];
            GemmParams p{};
            p.A = s->xn.p;
            p.W = w.qkv_w.p;
            p.C = s->qkv.p;
            p.M = M;
            p.N = 3 * c.d_model;
            p.K = c.d_model;
            p.lda = d;
            p.ldw = d;
            p.ldc = 3 * d;
            p.bias = w.qkv_b.as<float>();
            if (xn_is_ln1)  // the producer of x wrote LN1(x) next to it
                WMCHK(gemm_dispatch(T, T, p, 1, st));
            else
                WMCHK(ln_then_gemm(T, T, p, s->x.as<float>(), w.ln1_g.as<float>(), w.ln1_b.as<float>(), st));
            DISPATCH_DT(T, TT, launch_flash_attn_enc<TT>(s->qkv.p, s->ao.p, bc, c.n_heads, c.n_audio_ctx, ATTN_SCALE, st));
            GemmParams o{};
            o.A = s->ao.p;
            o.W = w.o_w.p;
            o.C = s->x.p;
            o.M = M;
            o.N = c.d_model;
            o.K = c.d_model;
            o.lda = d;
            o.ldw = d;
            o.ldc = d;
            o.bias = w.o_b.as<float>();
            o.residual = s->x.as<float>();
            o.ldr = d;
            const bool xn_is_ln2 = gemm_nt_fuses_layernorm_out(opb, o);
            if (xn_is_ln2) {
                o.lno_g = w.ln2_g.as<float>();
                o.lno_b = w.ln2_b.as<float>();
                o.lno_out = s->xn.p;
            }
            WMCHK(gemm_dispatch(T, WM_F32, o, 1, st));
            GemmParams f1{};
            f1.A = s->xn.p;
            f1.W = w.fc1_w.p;
            f1.C = s->hid.p;
            f1.M = M;
            f1.N = c.ffn;
            f1.K = c.d_model;
            f1.lda = d;
            f1.ldw = d;
            f1.ldc = c.ffn;
            f1.bias = w.fc1_b.as<float>();
            f1.act = 1;
            f1.gelu_mode = m->cfg.gelu_mode;
            if (xn_is_ln2)
                WMCHK(gemm_dispatch(T, T, f1, 1, st));
            else
                WMCHK(ln_then_gemm(T, T, f1, s->x.as<float>(), w.ln2_g.as<float>(), w.ln2_b.as<float>(), st));
            GemmParams f2{};
            f2.A = s->hid.p;
            f2.W = w.fc2_w.p;
            f2.C = s->x.p;
            f2.M = M;
            f2.N = c.d_model;
            f2.K = c.ffn;
            f2.lda = c.ffn;
            f2.ldw = c.ffn;
            f2.ldc = d;
            f2.bias = w.fc2_b.as<float>();
            f2.residual = s->x.as<float>();
            f2.ldr = d;
            const bool fuse_out = gemm_nt_fuses_layernorm_out(opb, f2);
            xn_is_ln1 = l + 1 < c.n_layers && fuse_out;
            if (xn_is_ln1) {  // the next block's LN1
                f2.lno_g = m->enc[l + 1].ln1_g.as<float>();
                f2.lno_b = m->enc[l + 1].ln1_b.as<float>();
                f2.lno_out = s->xn.p;
            } else if (fuse_out) {  // last block: ln_post (whisper.mojo:97-98) as operand rows for the cross-K/V projection
                f2.lno_g = m->enc_ln_g.as<float>();
                f2.lno_b = m->enc_ln_b.as<float>();
                f2.lno_out = post_rows;
                post_fused = true;
            }
            WMCHK(gemm_dispatch(T, WM_F32, f2, 1, st));
        }
        float* encf = s->enc_f.as<float>() + (size_t)c0 * NT * d;
        if (!post_fused)  // operand rows (and the fp32 copy) from the LayerNorm kernel
            DISPATCH_DT(T, TT, launch_layernorm_rows<TT>(s->x.as<float>(), m->enc_ln_g.as<float>(), m->enc_ln_b.as<float>(), post_rows, want_f32 ? encf : nullptr, M, c.d_model, 1e-5f, st));
        else if (want_f32)  // the fp32 copy only
            DISPATCH_DT(T, TT, launch_layernorm_rows<TT>(s->x.as<float>(), m->enc_ln_g.as<float>(), m->enc_ln_b.as<float>(), nullptr, encf, M, c.d_model, 1e-5f, st));
        if (!m->xattn) WMCHK(cross_kv_chunk(m, s, c0, bc, st));
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// B < 0: any batch size (the caller takes it from the state AFTER this check — a stale handle is never dereferenced)
static int check_state(wm_model* m, wm_state* s, int B) {
    if (!m || !s) return fail(WM_E_ARG, "null handle");
    if (!state_is_live(s)) return fail(WM_E_ARG, "stale state handle (its model was freed or reloaded)");
    if (s->m != m) return fail(WM_E_ARG, "state belongs to another model");
    if (B >= 0 && B != s->B) return fail(WM_E_ARG, "B=%d but the state was created for %d", B, s->B);
    return 0;
}

extern "C" int wm_encode(wm_model* m, wm_state* s, const float* mel, int mel_on_device, int B, float* enc_out) {
    WMCHK(check_state(m, s, B));
    if (!mel) return fail(WM_E_ARG, "null mel");
    HIPCHK(hipSetDevice(m->device));
    WMCHK(wm_state_reset(s));
    const wm_dims& c = m->cfg.dims;
    const float* mel_dev = mel;
    if (!mel_on_device) {
        HIPCHK(hipMemcpyAsync(s->mel_dev.p, mel, (size_t)B * c.n_mels * 2 * c.n_audio_ctx * 4, hipMemcpyHostToDevice, m->stream));
        mel_dev = s->mel_dev.as<float>();
    }
    WMCHK(run_encoder(m, s, mel_dev, B, m->stream, nullptr, 0, enc_out != nullptr));
    s->has_enc = s->has_cross = true;
    s->last_mel = mel_dev;
    if (enc_out) HIPCHK(hipMemcpyAsync(enc_out, s->enc_f.p, (size_t)B * c.n_audio_ctx * c.d_model * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

extern "C" int wm_state_set_encoder_output(wm_model* m, wm_state* s, const float* enc_out, int B) {
    WMCHK(check_state(m, s, B));
    if (!enc_out) return fail(WM_E_ARG, "null enc_out");
    HIPCHK(hipSetDevice(m->device));
    WMCHK(wm_state_reset(s));
    const wm_dims& c = m->cfg.dims;
    const size_t NT = c.n_audio_ctx, d = c.d_model;
    HIPCHK(hipMemcpyAsync(s->enc_f.p, enc_out, (size_t)B * NT * d * 4, hipMemcpyHostToDevice, m->stream));
    for (int c0 = 0; c0 < B; c0 += s->Bc) {
        const int bc = std::min(s->Bc, B - c0);
        if (m->xattn) {  // the cross-attention reads the bf16 rows themselves
            launch_convert<bf16>(s->enc_f.as<float>() + (size_t)c0 * NT * d, off_bytes(s->enc_x, (size_t)c0 * NT * d * 2), (size_t)bc * NT * d, m->stream);
            continue;
        }
        DISPATCH_DT(m->cfg.compute_dtype, TT, launch_convert<TT>(s->enc_f.as<float>() + (size_t)c0 * NT * d, s->enc_t.p, (size_t)bc * NT * d, m->stream));
        WMCHK(cross_kv_chunk(m, s, c0, bc, m->stream));
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    s->has_enc = s->has_cross = true;
    return 0;
}

// ---- one decode step for all B utterances: whisper.mojo:130-167 with L_tgt = 1 ------------------------------------
int dec_linear_dispatch(int dt, const DecLinearParams& p, hipStream_t st) {
    int rc = 0;
    DISPATCH_DT(dt, TT, rc = launch_dec_linear<TT>(p, st));
    return launch_rc(rc);
}
int attn_decode_dispatch(int dt, const AttnDecParams& p, hipStream_t st, const int* key_lo) {
    int rc = 0;
    DISPATCH_DT(dt, TT, rc = launch_attn_decode<TT>(p, st, key_lo));
    return launch_rc(rc);
}

// A view of `nb` utterances starting at b0, decoding on stream st under control block ctl.
struct DecView {
    int b0, nb;
    hipStream_t st;
    StepCtl* ctl;
};
static DecView whole_batch(wm_model* m, wm_state* s) { return DecView{0, s->B, m->stream, s->ctl.as<StepCtl>()}; }
template <typename T> static T* lane_ptr(const DevBuf& buf, const DecView& v, size_t stride) { return buf.as<T>() + (size_t)v.b0 * stride; }  // view v's rows

static VocabHead vocab_head(const wm_model* m) {
    return VocabHead{m->dec_ln_g.as<float>(), m->dec_ln_b.as<float>(), dec_dtype(m->cfg) == WM_F32 ? m->tok_emb_f.p : m->tok_emb_t.p,
                     m->cfg.dims.vocab, m->cfg.dims.d_model};
}

// m->xattn: the cross-attention of layer l over X for the rows of view v (P positions each): absorb + X sweep (launch_cross_attn),
// then merge + V-apply into out (cross_attn_merge).  Rows are position-major as everywhere in decode_core.
static XAttnParams xattn_params(wm_model* m, wm_state* s, int l, const DecView& v, int P) {
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model;
    XAttnParams x{};
    x.q = lane_ptr<float>(s->dq, v, d);
    x.Wk = off_bytes(m->cross_kv_w, (size_t)(2 * l) * d * d * 2);
    x.Wv = off_bytes(m->cross_kv_w, (size_t)(2 * l + 1) * d * d * 2);
    x.bv = m->cross_kv_b.as<float>() + (size_t)(2 * l + 1) * d;
    x.X = off_bytes(s->enc_x, (size_t)v.b0 * c.n_audio_ctx * d * 2);
    x.x_stride = (long)((size_t)c.n_audio_ctx * d);
    x.n_keys = c.n_audio_ctx;
    x.nsplit = s->nsplit;
    x.H = c.n_heads;
    x.d = c.d_model;
    x.rows = v.nb * P;
    x.q_B = P > 1 ? v.nb : 0;
    x.scale = ATTN_SCALE;
    x.qs = off_bytes(s->xq, (size_t)v.b0 * 3 * c.n_heads * d * 2);
    x.part_y = lane_ptr<float>(s->part_y, v, s->nsplit * c.n_heads * d);
    x.part_ml = lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2);
    return x;
}
static int cross_attn_merge(wm_model* m, wm_state* s, int l, const DecView& v, int P, void* out, int out_dtype) {
    XAttnParams x = xattn_params(m, s, l, v, P);
    x.out = out;
    x.out_dtype = out_dtype;
    return launch_rc(launch_xattn_merge(x, v.st));
}

static int launch_cross_attn(wm_model* m, wm_state* s, int l, const DecView& v, int P) {
    if (m->xattn) {
        const XAttnParams x = xattn_params(m, s, l, v, P);
        WMCHK(launch_rc(launch_xattn_absorb(x, v.st)));
        return launch_rc(launch_xattn(x, v.st));
    }
    const wm_dims& c = m->cfg.dims;
    const size_t d = c.d_model, ks = dt_size(m->cfg.kv_dtype);
    const size_t cross_l = (size_t)s->B * c.n_audio_ctx * d;
    const size_t boff = (size_t)v.b0 * c.n_audio_ctx * d;
    AttnDecParams a{};
    a.q = lane_ptr<float>(s->dq, v, d);
    a.K = off_bytes(s->cross_kv, ((size_t)(2 * l) * cross_l + boff) * ks);
    a.V = off_bytes(s->cross_kv, ((size_t)(2 * l + 1) * cross_l + boff) * ks);
    a.batch_stride = (long)((size_t)c.n_audio_ctx * d);
    a.n_keys = c.n_audio_ctx;
    a.ctl = v.ctl;
    a.nsplit = s->nsplit;
    a.scale = ATTN_SCALE;
    a.part_o = lane_ptr<float>(s->part_o, v, s->nsplit * d);
    a.part_ml = lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2);
    a.H = c.n_heads;
    a.d = c.d_model;
    a.B = v.nb * P;
    a.q_B = P > 1 ? v.nb : 0;
    static const bool no_mq = wm_env("WM_NO_MQ_PREFILL") != nullptr;
    a.nq = (P == 4 && !no_mq) ? 4 : 0;  // the reference's 4-token prompt: one K/V sweep for the four positions
    a.ts = (long long*)m->ts_buf.p;
    a.ts_id = s->trace_id;
    // fewer K/V-streaming workgroups per CU when passes share the chip (AttnDecParams.lds_pad).  16-bit K/V: 34 KB of pad (+ 20 KB
    // static) = two per CU.  fp32 K/V (12 KB static): ONE per CU measured best with four 128-row passes in flight — pipelined ms per
    // 64-clip pass: pad 0 (four per CU) 28.2, 20 KB 28.4, 34 KB (three) 27.8, 42 / 50 / 60 KB (two) 27.3 / 27.5 / 27.4, 90 KB (one) 27.05
    a.lds_pad = s->shares_chip ? (m->cfg.kv_dtype == WM_F32 ? 90000 : 34 * 1024) : 0;
    return attn_decode_dispatch(m->cfg.kv_dtype, a, v.st);
}

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
// What every linear launch of a decoder pass sets (ln_g null: no LayerNorm prologue); each block's special part is added by name below
DecLinearParams linear_block(const float* x, const float* ln_g, const float* ln_b, const void* W, const float* bias, int N, int K, int B,
                             float* out, int ldo) {
    DecLinearParams p{};
    p.x = x;
    p.ldx = K;
    p.ln_g = ln_g;
    p.ln_b = ln_b;
    p.W = W;
    p.N = N;
    p.K = K;
    p.B = B;
    p.bias = bias;
    p.out = out;
    p.ldo = ldo;
    return p;
}
static void* self_kv_rows(wm_model* m, wm_state* s, const DecView& v, int l, int k_or_v) {  // layer l's cached K (0) / V (1) rows of view v
    const size_t per_utt = (size_t)m->cfg.dims.n_text_ctx * m->cfg.dims.d_model;
    return off_bytes(s->self_kv, ((size_t)(2 * l + k_or_v) * s->B + v.b0) * per_utt * dt_size(m->cfg.kv_dtype));
}
static void add_cache_append(DecLinearParams& p, wm_model* m, wm_state* s, const DecView& v, int l, int P) {  // k, v to cache row len (+ t)
    const wm_dims& c = m->cfg.dims;
    p.kcache = self_kv_rows(m, s, v, l, 0);
    p.vcache = self_kv_rows(m, s, v, l, 1);
    p.kv_batch_stride = (long)((size_t)c.n_text_ctx * c.d_model);
    p.d_model = c.d_model;
    p.kv_dtype = m->cfg.kv_dtype;
    p.kv_B = P > 1 ? v.nb : 0;
    p.ctl = v.ctl;
}
static void add_align_capture(DecLinearParams& p, const wm_state::Align& al, int l, const DecView& v, int t0) {  // layer l's alignment heads
    for (int h = 0; h < 32; ++h) p.cap_sel[h] = -1;
    const int n_sel = (int)al.pairs.size() / 2;
    bool any = false;
    for (int k = 0; k < n_sel; ++k)
        if (al.pairs[2 * k] == l) {
            p.cap_sel[al.pairs[2 * k + 1]] = (signed char)k;
            any = true;
        }
    if (any && al.ragged) {  // an align pass's chunk: rows [t0, t0 + P) of the row map (single-lane: b0 = 0)
        p.cap = al.cap.as<float>();
        p.cap_map = al.map.as<int>() + (size_t)std::max(t0, 0) * v.nb;
        p.cap_nsel = n_sel;
    } else if (any) {
        p.cap_row_stride = (long)al.L * n_sel * 64;
        p.cap = al.cap.as<float>() + (size_t)v.b0 * p.cap_row_stride;
        p.cap_step0 = al.n_prompt;
        p.cap_steps = al.L;
        p.cap_nsel = n_sel;
        p.ctl = v.ctl;  // the step index comes from the cache length (the row map needs none)
    }
}
static void add_gelu_t(DecLinearParams& p, int gelu_mode) {  // GELU, stored in the operand dtype for the next MFMA
    p.act = 1;
    p.gelu_mode = gelu_mode;
    p.out_is_t = 1;
}
static void add_argmax_partials(DecLinearParams& p, wm_state* s, const DecView& v, const float* mask, const TsRules* rules) {
    p.amax_val = lane_ptr<float>(s->amax_val, v, s->npart);
    p.amax_idx = lane_ptr<int>(s->amax_idx, v, s->npart);
    p.amax_stride = s->npart;
    p.amax_mask = mask;
    if (rules && rules->tb > 0) {  // timestamp rules: split the candidates by the utterances' admissible ranges
        p.ts_state = lane_ptr<TsState>(s->ts_state, v, 1);
        p.ts_begin = rules->tb;
        p.ts_val = lane_ptr<float>(s->ts_val, v, s->npart);
        p.ts_idx = lane_ptr<int>(s->ts_idx, v, s->npart);
        p.ts_m = lane_ptr<float>(s->ts_m, v, s->npart);
        p.ts_s = lane_ptr<float>(s->ts_s, v, s->npart);
    }
    if (s->lp.on) p.lp_s = lane_ptr<float>(s->lp.part_s, v, s->npart);
    if (s->rp.on) {  // repetition processors: the rows' sets, ahead of the mask and the ranges
        p.rp_seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
        p.rp_ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
        p.rp_ctl = s->rp.ctl.as<RepeatCtl>();
        p.rp_words = s->rp.words;
        if (s->rp.sb) {
            p.sb_hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
            p.sb_val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
            p.sb_ctl = s->rp.sbctl.as<SeqBiasCtl>();
        }
    }
}
// start of a pass with the repetition processors, behind the lane's init-tokens launch
static void repeat_init(wm_state* s, const DecView& v) {
    RepeatInitParams r{};
    r.seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
    r.ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
    r.words = s->rp.words;
    r.B = v.nb;
    r.ctl = s->rp.ctl.as<RepeatCtl>();
    r.penalty = s->rp.ask.penalty;
    r.ngram = s->rp.ask.ngram;
    r.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    r.out_stride = s->out_stride;
    r.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    launch_repeat_init(r, v.st);
}
// start of a pass with sequence bias / bad words, behind the lane's init-tokens launch; eot: the pass's, whose length-1 ban is dropped
static int seq_bias_init(wm_state* s, const DecView& v, int eot) {
    SeqBiasInitParams r{};
    r.hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
    r.val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
    r.words = s->rp.words;
    r.B = v.nb;
    r.ctl = s->rp.sbctl.as<SeqBiasCtl>();
    r.table = s->rp.ask.sb->ctl(eot);
    r.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    r.out_stride = s->out_stride;
    r.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    LCHK(launch_seq_bias_init(r, v.st));
    return 0;
}
// LN1 -> q | k,v appended to the cache   (layers.mojo:118-147)
static DecLinearParams qkv_block(wm_model* m, wm_state* s, const DecView& v, int l, int P) {
    const wm_dims& c = m->cfg.dims;
    const DecLayer& w = m->dec[l];
    DecLinearParams p = linear_block(lane_ptr<float>(s->dx, v, c.d_model), w.ln1_g.as<float>(), w.ln1_b.as<float>(), w.sqkv_w.p, w.sqkv_b.as<float>(),
                                  3 * c.d_model, c.d_model, v.nb * P, lane_ptr<float>(s->dq, v, c.d_model), c.d_model);
    add_cache_append(p, m, s, v, l, P);
    return p;
}
// x += in·Wᵀ + b, `in` in operand dtype (what the attention / fc1 launches hand over)
static DecLinearParams proj_residual_block(wm_model* m, wm_state* s, const DecView& v, int P, const float* in, int K, const DevBuf& W, const DevBuf& bias) {
    const wm_dims& c = m->cfg.dims;
    float* dx = lane_ptr<float>(s->dx, v, c.d_model);
    DecLinearParams p = linear_block(in, nullptr, nullptr, W.p, bias.as<float>(), c.d_model, K, v.nb * P, dx, c.d_model);
    p.x_is_t = 1;
    p.residual = dx;
    p.ldr = c.d_model;
    return p;
}

static int decode_core(wm_model* m, wm_state* s, const DecView& v, const DecPass& a) {
    const wm_dims& c = m->cfg.dims;
    const int T = dec_dtype(m->cfg), KV = m->cfg.kv_dtype;  // T: the decoder's operand dtype
    const int P = a.P, B = v.nb * P;  // B: activation rows of this pass
    const int qB = P > 1 ? v.nb : 0;  // position-major row mapping on
    const size_t d = c.d_model;
    hipStream_t st = v.st;
    float* dx = lane_ptr<float>(s->dx, v, d);
    float* dq = lane_ptr<float>(s->dq, v, d);
    // attention output / MLP hidden rows: operand dtype T (fp32 buffers, used at T's width)
    float* dattn = (float*)off_bytes(s->dattn, (size_t)v.b0 * d * dt_size(T));
    float* dhid = (float*)off_bytes(s->dhid, (size_t)v.b0 * c.ffn * dt_size(T));
    if (a.embed) {
        const size_t row0 = a.t0 >= 0 ? (size_t)a.t0 * v.nb : 0;  // the pass's first row of tok_rows / pos_rows
        const bool rows = a.t0 >= 0 || P > 1;
        launch_dec_embed(m->tok_emb_f.as<float>(), m->dec_pos.as<float>(), rows ? s->tok_rows.as<int>() + row0 : lane_ptr<int>(s->tok, v, 1),
                         rows ? s->pos_rows.as<int>() + row0 : lane_ptr<int>(s->pos, v, 1), dx, B, c.d_model, st);
    }
    for (int l = 0; l < c.n_layers; ++l) {
        DecLayer& w = m->dec[l];
        WMCHK(dec_linear_dispatch(T, qkv_block(m, s, v, l, P), st));
        {  // self-attention over current_len+1 cached rows   (layers.mojo:186-272)
            AttnDecParams q{};
            q.q = dq;
            q.K = self_kv_rows(m, s, v, l, 0);
            q.V = self_kv_rows(m, s, v, l, 1);
            q.batch_stride = (long)((size_t)c.n_text_ctx * d);
            q.n_keys = -1;
            q.q_B = qB;
            q.ctl = v.ctl;
            q.nsplit = 1;
            q.scale = ATTN_SCALE;
            q.direct_out = dattn;
            q.out_dtype = T;
            q.H = c.n_heads;
            q.d = c.d_model;
            q.B = B;
            // per-row prompts: every utterance sweeps its own key window [key_lo, len + 1 (+ t))
            WMCHK(attn_decode_dispatch(KV, q, st, s->rw.on && a.key_window ? lane_ptr<int>(s->rw.key_lo, v, 1) : nullptr));
        }
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dattn, c.d_model, w.so_w, w.so_b), st));
        {  // LNx -> cross q
            DecLinearParams p = linear_block(dx, w.lnx_g.as<float>(), w.lnx_b.as<float>(), w.cq_w.p, w.cq_b.as<float>(), c.d_model, c.d_model, B, dq, c.d_model);
            if (a.capture && s->al.on) add_align_capture(p, s->al, l, v, a.t0);
            WMCHK(dec_linear_dispatch(T, p, st));
        }
        WMCHK(launch_cross_attn(m, s, l, v, P));
        // (merging the chunk partials inside the projection's prologue was measured 14 us per layer SLOWER than this
        // 3 us launch: 96 workgroups each re-reading 295 KB of partials)
        if (m->xattn)
            WMCHK(cross_attn_merge(m, s, l, v, P, dattn, T));
        else
            launch_attn_combine(lane_ptr<float>(s->part_o, v, s->nsplit * d), lane_ptr<float>(s->part_ml, v, (size_t)s->nsplit * c.n_heads * 2), dattn, T, B,
                                s->nsplit, c.n_heads, c.d_model, st, (long long*)m->ts_buf.p, s->trace_id);
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dattn, c.d_model, w.co_w, w.co_b), st));
        {  // LN2 -> fc1 + GELU
            DecLinearParams p = linear_block(dx, w.ln2_g.as<float>(), w.ln2_b.as<float>(), w.fc1_w.p, w.fc1_b.as<float>(), c.ffn, c.d_model, B, dhid, c.ffn);
            add_gelu_t(p, m->cfg.gelu_mode);
            WMCHK(dec_linear_dispatch(T, p, st));
        }
        WMCHK(dec_linear_dispatch(T, proj_residual_block(m, s, v, P, dhid, c.ffn, w.fc2_w, w.fc2_b), st));
    }
    if (a.logits != Logits::none) {  // final LN + tied-embedding logits (whisper.mojo:156-166), no bias, rows of the last position
        const VocabHead h = vocab_head(m);
        DecLinearParams p = linear_block(dx + (size_t)(P - 1) * v.nb * d, h.ln_g, h.ln_b, h.emb, nullptr, h.vocab, h.d_model, v.nb,
                                      a.logits == Logits::full || s->tk.k > 0 ? lane_ptr<float>(s->logits, v, m->Vpad) : nullptr, m->Vpad);
        add_argmax_partials(p, s, v, a.mask, a.rules);  // (top-k alternatives: the selection launch reads the stored, processed rows)
        p.ts = (long long*)m->ts_buf.p;
        p.ts_id = s->trace_id;
        int lrc = 0;
        DISPATCH_DT(T, TT, lrc = launch_dec_logits<TT>(p, st));
        LCHK(lrc);
    }
    return 0;
}

// The fused argmax's second stage, in its three uses.  wm_decode_step: the next id of every row, nothing recorded, no stop rule
static ArgmaxParams argmax_peek(wm_model* m, wm_state* s, const DecView& v) {
    ArgmaxParams a{};
    a.logits = lane_ptr<float>(s->logits, v, m->Vpad);
    a.pval = lane_ptr<float>(s->amax_val, v, s->npart);
    a.pidx = lane_ptr<int>(s->amax_idx, v, s->npart);
    a.npart = s->npart;
    a.ldl = m->Vpad;
    a.V = m->cfg.dims.vocab;
    a.B = v.nb;
    a.next = lane_ptr<int>(s->tok, v, 1);
    a.out_stride = s->out_stride;
    a.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
    a.finished = lane_ptr<int>(s->finished, v, 1);
    a.ctl = v.ctl;
    a.pos = lane_ptr<int>(s->pos, v, 1);
    a.ts = (long long*)m->ts_buf.p;
    a.ts_id = s->trace_id;
    a.eot = -1;
    a.ignore_eot = 1;
    return a;
}
// the end of a prefill: the first id goes into the pass's outputs (ids, log-probs, timestamp history); the cache length stays
static ArgmaxParams argmax_first_id(wm_model* m, wm_state* s, const DecView& v, int eot, int ignore_eot, const TsRules* rules) {
    ArgmaxParams a = argmax_peek(m, s, v);
    if (rules && rules->tb > 0) {
        a.ts_state = lane_ptr<TsState>(s->ts_state, v, 1);
        a.rules = *rules;
        a.ts_val = lane_ptr<float>(s->ts_val, v, s->npart);
        a.ts_idx = lane_ptr<int>(s->ts_idx, v, s->npart);
        a.ts_m = lane_ptr<float>(s->ts_m, v, s->npart);
        a.ts_s = lane_ptr<float>(s->ts_s, v, s->npart);
        a.ts_part0 = rules->tb / dec_logits_ids_per_part(m->cfg.dims.vocab);
    }
    a.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
    if (s->lp.on) {
        a.lp_s = lane_ptr<float>(s->lp.part_s, v, s->npart);
        a.logprobs = lane_ptr<float>(s->lp.table, v, s->out_stride);
        a.lp_sum = lane_ptr<float>(s->lp.sum, v, 1);
        if (s->tk.k > 0) a.tk_rows = lane_ptr<TopkRow>(s->tk.rows, v, 1);
    }
    if (s->rp.on) {
        a.rp_seen = lane_ptr<unsigned>(s->rp.seen, v, s->rp.words);
        a.rp_ban = lane_ptr<unsigned>(s->rp.ban, v, s->rp.words);
        a.rp_ctl = s->rp.ctl.as<RepeatCtl>();
        a.rp_words = s->rp.words;
        if (s->rp.sb) {
            a.sb_hit = lane_ptr<unsigned>(s->rp.hit, v, s->rp.words);
            a.sb_val = lane_ptr<SeqSlot>(s->rp.val, v, SEQ_BIAS_MAX);
            a.sb_ctl = s->rp.sbctl.as<SeqBiasCtl>();
        }
    }
    a.eot = eot;
    a.ignore_eot = ignore_eot;
    return a;
}
// Top-k alternatives: the selection launch behind an argmax launch that recorded an id — the k best of each row's stored
// logits under `mask` and the ranges the argmax left in the row's TopkRow, into the tables' entry beside the id.  k = 0: nothing.
static int topk_select(wm_model* m, wm_state* s, const DecView& v, const float* mask) {
    if (s->tk.k <= 0) return 0;
    TopkSelectParams q{};
    q.logits = lane_ptr<float>(s->logits, v, m->Vpad);
    q.ldl = m->Vpad;
    q.V = m->cfg.dims.vocab;
    q.B = v.nb;
    q.mask = mask;
    q.rows = lane_ptr<TopkRow>(s->tk.rows, v, 1);
    q.k = s->tk.k;
    q.ids = lane_ptr<int>(s->tk.ids, v, (size_t)s->out_stride * s->tk.k);
    q.lps = lane_ptr<float>(s->tk.lps, v, (size_t)s->out_stride * s->tk.k);
    LCHK(launch_topk_select(q, v.st));
    return 0;
}
// a step of the greedy loop: also advances the cache length, reports progress to the host and writes the next step's input row
static ArgmaxParams argmax_loop_step(wm_model* m, wm_state* s, const DecView& v, int eot, int ignore_eot, const TsRules* rules) {
    ArgmaxParams a = argmax_first_id(m, s, v, eot, ignore_eot, rules);
    a.advance = 1;
    a.host_progress = s->d_prog;
    a.emb_tok = m->tok_emb_f.as<float>();
    a.emb_pos = m->dec_pos.as<float>();
    a.emb_out = lane_ptr<float>(s->dx, v, m->cfg.dims.d_model);
    a.d = m->cfg.dims.d_model;
    a.max_pos = m->cfg.dims.n_text_ctx - 1;
    return a;
}

extern "C" int wm_decode_step(wm_model* m, wm_state* s, const int32_t* tokens, int q_len, const int32_t* start_pos,
                              float* logits, int32_t* next) {
    if (!m || !s || !tokens || !start_pos || q_len <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_state(m, s, -1));
    if (!s->has_enc) return fail(WM_E_STATE, "no encoder output in this state (call wm_encode first)");
    const wm_dims& c = m->cfg.dims;
    const int B = s->B;
    if (s->host_len + q_len > c.n_text_ctx) return fail(WM_E_STATE, "KV cache full (%d + %d > %d)", s->host_len, q_len, c.n_text_ctx);
    for (int b = 0; b < B; ++b) {
        if (start_pos[b] < 0 || start_pos[b] + q_len > c.n_text_ctx) return fail(WM_E_ARG, "start_pos[%d]=%d out of range", b, start_pos[b]);
        for (int i = 0; i < q_len; ++i)
            if (tokens[b * q_len + i] < 0 || tokens[b * q_len + i] >= c.vocab) return fail(WM_E_ARG, "token id out of range");
    }
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    const DecView v = whole_batch(m, s);
    std::vector<int32_t> col(B), pos(B);
    DecPass pass;
    pass.logits = Logits::full;  // for the caller, of the last position
    if (q_len > 1 && q_len <= wm_state::PREFILL_MAX) {  // the q_len block of whisper.mojo:195 as ONE position-major pass
        std::vector<int32_t> trow((size_t)q_len * B), prow((size_t)q_len * B);
        for (int i = 0; i < q_len; ++i)
            for (int b = 0; b < B; ++b) {
                trow[(size_t)i * B + b] = tokens[b * q_len + i];
                prow[(size_t)i * B + b] = start_pos[b] + i;
            }
        HIPCHK(hipMemcpyAsync(s->tok_rows.p, trow.data(), trow.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->pos_rows.p, prow.data(), prow.size() * 4, hipMemcpyHostToDevice, st));
        launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
        pass.P = q_len;
        WMCHK(decode_core(m, s, v, pass));
        HIPCHK(hipGetLastError());         // a launch that failed (bad configuration, LDS attribute) is reported here
        HIPCHK(hipStreamSynchronize(st));  // trow / prow go out of scope
        s->host_len += q_len;
        q_len = 0;
    }
    for (int i = 0; i < q_len; ++i) {
        for (int b = 0; b < B; ++b) {
            col[b] = tokens[b * q_len + i];
            pos[b] = start_pos[b] + i;
        }
        HIPCHK(hipMemcpyAsync(s->tok.p, col.data(), B * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(s->pos.p, pos.data(), B * 4, hipMemcpyHostToDevice, st));
        launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
        pass.logits = i == q_len - 1 ? Logits::full : Logits::none;
        WMCHK(decode_core(m, s, v, pass));
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));  // col/pos are reused next iteration
        s->host_len += 1;
    }
    launch_set_step(v.ctl, s->host_len, 1, nullptr, 0, nullptr, 0, B, st);
    if (next) {
        launch_argmax_step(argmax_peek(m, s, v), st);
        HIPCHK(hipMemcpyAsync(next, s->tok.p, B * 4, hipMemcpyDeviceToHost, st));
    }
    if (logits)
        HIPCHK(hipMemcpy2DAsync(logits, (size_t)c.vocab * 4, s->logits.p, (size_t)m->Vpad * 4, (size_t)c.vocab * 4, B, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- greedy-loop enqueue machinery (used by transcribe_decode and the loop pump) -----------------------------------------------
static const int LOOP_CHUNK = 8;  // graph replays per sub-chunk; two sub-chunks (16 steps) are queued ahead of the GPU

// One step of the greedy loop for view v as s->step describes it: the decoder pass and its argmax.  The only place that pairs
// them — transcribe_decode captures this into the lanes' graphs, enqueue_loop_steps launches it where there is no graph.
static int loop_step(wm_model* m, wm_state* s, const DecView& v) {
    const wm_state::StepKey& k = s->step;
    DecPass step;
    step.embed = false;
    step.logits = Logits::partials;
    step.mask = s->mask_steady.as<float>();
    step.rules = &k.rules;  // (tb <= 0: off, as every reader of the rules checks)
    step.capture = true;
    WMCHK(decode_core(m, s, v, step));
    LCHK(launch_argmax_step(argmax_loop_step(m, s, v, k.eot, k.ignore_eot, &k.rules), v.st));
    if (k.top_k > 0) WMCHK(topk_select(m, s, v, step.mask));
    return 0;
}
static void invalidate_step_graphs(wm_state* s) { s->graphs_valid = false; }  // the next greedy pass captures its step anew

// n more steps of the pending pass's loop on the state's lane streams (captured graph, or eager launches in the developer build)
static int enqueue_loop_steps(wm_model* m, wm_state* s, int n) {
    for (int k = 0; k < n; ++k, ++s->loop_enq) {
        const int it = s->loop_enq;
        for (auto& ln : s->lanes) {
            if (trace_events_on() && it % 10 == 9) trace_mark(ln.st, "state %p lane %d step %d", (void*)s, ln.b0, it);
            if (ln.graph[0] && s->graphs_valid) {
                const hipError_t e = hipGraphLaunch(ln.graph[it % wm_state::Lane::NEXEC], ln.st);
                if (e != hipSuccess) return fail(WM_E_HIP, "hipGraphLaunch: %s", hipGetErrorString(e));
            } else {
                WMCHK(loop_step(m, s, DecView{ln.b0, ln.nb, ln.st, ln.ctl}));
            }
        }
    }
    return 0;
}
// the pending pass is fully enqueued: its completion events go behind the last step
static int enqueue_align(wm_model* m, wm_state* s);
static int finish_enqueue(wm_model* m, wm_state* s) {
    int rc = 0;
    if (s->al.on) {  // token timestamps: the post-loop kernels go behind the last step, before the pass's completion events
        for (size_t i = 1; i < s->lanes.size() && !rc; ++i) {
            hipError_t e = hipEventRecord(s->lanes[i].done, s->lanes[i].st);
            if (e == hipSuccess) e = hipStreamWaitEvent(s->lanes[0].st, s->lanes[i].done, 0);
            if (e != hipSuccess) rc = fail(WM_E_HIP, "align wait: %s", hipGetErrorString(e));
        }
        if (!rc) rc = enqueue_align(m, s);
    }
    for (auto& ln : s->lanes) {
        trace_mark(ln.st, "state %p lane %d decode end", (void*)s, ln.b0);
        const hipError_t e = hipEventRecord(ln.done, ln.st);
        if (e != hipSuccess && !rc) rc = fail(WM_E_HIP, "hipEventRecord: %s", hipGetErrorString(e));
    }
    if (!rc && hipGetLastError() != hipSuccess) rc = fail(WM_E_HIP, "a launch of the greedy loop failed");
    s->last_steps = s->loop_enq;
    if (rc && !s->enq_rc) {
        s->enq_rc = rc;
        s->enq_err = g_err;
    }
    s->enq_done.store(true);
    return rc;
}
static int enqueue_chunk(wm_model* m, wm_state* s) {
    const int n = std::min(LOOP_CHUNK, s->loop_total - s->loop_enq);
    WMCHK(enqueue_loop_steps(m, s, n));
    HIPCHK(hipEventRecord(s->chunk_ev[s->chunk_k & 1], s->lanes[0].st));
    ++s->chunk_k;
    return 0;
}
// One decision of the loop pump for state s: once sub-chunk k-2 has completed, either stop (every utterance finished, or the loop
// bound reached) or enqueue sub-chunk k.  Returns 1 when it did something, 0 when sub-chunk k-2 is still running (non-blocking
// form), < 0 on error (the pass is then closed with enq_rc set).
static int pump_step(wm_model* m, wm_state* s, bool block) {
    hipEvent_t ev = s->chunk_ev[s->chunk_k & 1];  // recorded behind sub-chunk chunk_k - 2
    hipError_t e = block ? hipEventSynchronize(ev) : hipEventQuery(ev);
    if (e == hipErrorNotReady) return 0;
    int rc = e == hipSuccess ? 0 : fail(WM_E_HIP, "loop pump: %s", hipGetErrorString(e));
    if (!rc) {
        const bool all_done = s->h_prog[0] >= s->B;  // a lower bound of the finished count: never stops a running utterance
        if (all_done || s->loop_enq >= s->loop_total) {
            rc = finish_enqueue(m, s);
            return rc ? -1 : 1;
        }
        rc = enqueue_chunk(m, s);
        if (!rc) return 1;
    }
    s->enq_rc = rc;
    s->enq_err = g_err;
    (void)finish_enqueue(m, s);
    return -1;
}
static void pump_main(wm_model* m) {
    (void)hipSetDevice(m->device);
    std::unique_lock<std::mutex> lk(m->pump_mu);
    for (;;) {
        m->pump_cv.wait(lk, [&] { return m->pump_quit || !m->pump_work.empty(); });
        if (m->pump_quit) return;
        bool progressed = false;
        for (size_t i = 0; i < m->pump_work.size();) {
            wm_state* s = m->pump_work[i];
            if (pump_step(m, s, false) != 0) progressed = true;
            if (s->enq_done.load()) {
                m->pump_work.erase(m->pump_work.begin() + (long)i);
                m->pump_cv.notify_all();  // wm_transcribe_wait may be waiting for this pass to be fully enqueued
            } else {
                ++i;
            }
        }
        if (!progressed) {  // every pending sub-chunk still running: they take milliseconds
            lk.unlock();
            std::this_thread::sleep_for(std::chrono::microseconds(100));
            lk.lock();
        }
    }
}

// No-speech probe.  capture: after the prefill pass that holds the <|startoftranscript|> position, keep that position's
// residual rows (row_off: its first row in the pass's position-major activations).  probe: after the prefill, one vocabulary sweep
// over the kept rows — the log-prob instantiation of the logits kernel a decode step of this state picks, no mask, no ranges, its
// partials in the probe's own buffers — and the finish kernel.  Both go on the lane's stream, outside the captured step graph.
static void ns_capture(wm_model* m, wm_state* s, const DecView& v, size_t row_off) {
    const size_t d = m->cfg.dims.d_model;
    launch_no_speech_capture(lane_ptr<float>(s->dx, v, d) + row_off * d, lane_ptr<float>(s->ns.x, v, d), v.nb, (int)d, v.st);
}
int ns_sweep(int T, const float* x, const VocabHead& h, int B, int npart, float* pmax, int* pidx, float* psum, int token, float* prob,
             float* lse, hipStream_t st) {
    DecLinearParams p = linear_block(x, h.ln_g, h.ln_b, h.emb, nullptr, h.vocab, h.d_model, B, nullptr, (h.vocab + 3) / 4 * 4);
    p.amax_val = pmax;
    p.amax_idx = pidx;
    p.amax_stride = npart;
    p.lp_s = psum;
    int lrc = 0;
    DISPATCH_DT(T, TT, lrc = launch_dec_logits<TT>(p, st));
    LCHK(lrc);
    NoSpeechParams q{};
    q.x = x;
    q.ldx = h.d_model;
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.K = h.d_model;
    q.token = token;
    q.B = B;
    q.pmax = pmax;
    q.psum = psum;
    q.npart = npart;
    q.stride = npart;
    q.prob = prob;
    q.lse = lse;
    DISPATCH_DT(T, TT, launch_no_speech_finish<TT>(q, st));
    return 0;
}
static int ns_probe(wm_model* m, wm_state* s, const DecView& v) {
    const wm_state::Ns& ns = s->ns;
    return ns_sweep(dec_dtype(m->cfg), lane_ptr<float>(ns.x, v, m->cfg.dims.d_model), vocab_head(m), v.nb, s->npart, lane_ptr<float>(ns.pmax, v, s->npart),
                    lane_ptr<int>(ns.pidx, v, s->npart), lane_ptr<float>(ns.psum, v, s->npart), ns.token, lane_ptr<float>(ns.prob, v, 1),
                    lane_ptr<float>(ns.lse, v, 1), v.st);
}

// Language detection, after the encoder on a single-lane state: one decoder pass over [sot] at position 0 for all rows
// (cache length 0, every row attends only to itself, no key window, no logits; its K/V rows in cache slot 0 are overwritten by the
// prefill that follows), its residual rows kept in lg.x, then lang_detect_kernel.  patch: the device prompt table whose language
// slots (lg.col) receive the ids, or null.  All on the lane's stream; nothing is read back.
static int lang_pass(wm_model* m, wm_state* s, const DecView& v, int* patch, int patch_stride) {
    const wm_dims& c = m->cfg.dims;
    const int T = dec_dtype(m->cfg);
    wm_state::Lang& lg = s->lg;
    HIPCHK(hipMemcpyAsync(lg.ids.p, lg.h_ids.data(), (size_t)lg.n * 4, hipMemcpyHostToDevice, v.st));
    if (patch) HIPCHK(hipMemcpyAsync(lane_ptr<int>(lg.col, v, 1), lg.h_col.data() + v.b0, (size_t)v.nb * 4, hipMemcpyHostToDevice, v.st));
    launch_set_step(v.ctl, 0, 1, lane_ptr<int>(s->pos, v, 1), 0, lane_ptr<int>(s->tok, v, 1), lg.sot, v.nb, v.st);
    DecPass sot;
    sot.key_window = false;
    WMCHK(decode_core(m, s, v, sot));
    launch_no_speech_capture(lane_ptr<float>(s->dx, v, c.d_model), lane_ptr<float>(lg.x, v, c.d_model), v.nb, c.d_model, v.st);
    const VocabHead h = vocab_head(m);
    LangDetectParams q{};
    q.x = lane_ptr<float>(lg.x, v, c.d_model);
    q.ldx = c.d_model;
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.lang_ids = lg.ids.as<int>();
    q.n_lang = lg.n;
    q.K = h.d_model;
    q.B = v.nb;
    q.lang_out = lane_ptr<int>(lg.out, v, 1);
    q.probs = lane_ptr<float>(lg.probs, v, lg.n);
    q.patch = patch ? patch + (size_t)v.b0 * patch_stride : nullptr;
    q.patch_stride = patch_stride;
    q.patch_col = lane_ptr<int>(lg.col, v, 1);
    DISPATCH_DT(T, TT, launch_lang_detect<TT>(q, v.st));
    return 0;
}

// Per-row prompts, the start of a pass on a single-lane state: prompt table and lengths to the device, tokens /
// key windows / prefill rows from them, the prefill in chunks of PREFILL_MAX positions through the position-major pass (the rows
// end together at position Lmax; logits for the last chunk only: every row's last position is real), the first id, and the per-row
// positions of the first loop step.  ip: the pass's InitTokensParams without the prompt.
static int prefill_rows(wm_model* m, wm_state* s, const DecView& v, InitTokensParams ip, const wm_decode_opts* o, const TsRules* rp) {
    wm_state::Rows& rw = s->rw;
    const int Lmax = rw.Lmax;
    HIPCHK(hipMemcpyAsync(rw.table.p, rw.h_table.data(), rw.h_table.size() * 4, hipMemcpyHostToDevice, v.st));
    HIPCHK(hipMemcpyAsync(rw.len.p, rw.h_len.data(), rw.h_len.size() * 4, hipMemcpyHostToDevice, v.st));
    if (s->lg.on) WMCHK(lang_pass(m, s, v, rw.table.as<int>(), rw.stride));  // the table's language slots come from the device (§19)
    ip.tok_rows = s->tok_rows.as<int>();
    ip.pos_rows = s->pos_rows.as<int>();
    launch_init_tokens_rows(ip, RowPromptParams{rw.table.as<int>(), rw.len.as<int>(), rw.stride, Lmax, rw.key_lo.as<int>()}, v.st);
    if (s->rp.on) repeat_init(s, v);  // each row's own prompt, a detected language included
    if (s->rp.sb) WMCHK(seq_bias_init(s, v, o->eot));
    for (int t0 = 0; t0 < Lmax; t0 += wm_state::PREFILL_MAX) {
        const int P = std::min<int>(wm_state::PREFILL_MAX, Lmax - t0);
        if (t0) launch_set_step(v.ctl, t0, 1, nullptr, 0, nullptr, 0, v.nb, v.st);
        DecPass chunk;
        chunk.P = P;
        chunk.t0 = t0;
        chunk.logits = t0 + P == Lmax ? Logits::partials : Logits::none;
        chunk.mask = s->mask_begin.as<float>();
        chunk.rules = rp;
        WMCHK(decode_core(m, s, v, chunk));
        // the rows end together, so every row's <|startoftranscript|> sits in cache slot Lmax - n_init, whatever its own length
        const int t_sot = Lmax - s->ns.n_init;
        if (s->ns.on && t_sot >= t0 && t_sot < t0 + P) ns_capture(m, s, v, (size_t)(t_sot - t0) * v.nb);
    }
    LCHK(launch_argmax_step(argmax_first_id(m, s, v, o->eot, o->ignore_eot, rp), v.st));
    WMCHK(topk_select(m, s, v, s->mask_begin.as<float>()));
    trace_mark(v.st, "state %p lane %d prefill end", (void*)s, v.b0);
    launch_set_rows_step(v.ctl, Lmax, lane_ptr<int>(s->pos, v, 1), rw.len.as<int>(), o->pos_mode == WM_POS_REF ? -1 : 0, v.nb, v.st);
    return 0;
}

// ---- Whisper.transcribe: whisper.mojo:184-223 ------------------------------------------------------------------------
// Enqueues the prompt prefill and the greedy loop for state s on its decode lane streams; returns without waiting.  The lanes
// first wait for the encoder (recorded on the stream it ran on).  Both entry points stop once every utterance has emitted eot
// (whisper.mojo:206-207): allow_poll = the synchronous one feeds its loop itself, sub-chunk by sub-chunk; the pipelined one
// hands the rest of the loop to the model's pump thread (see the enqueue machinery above).
static int transcribe_decode(wm_model* m, wm_state* s, const wm_decode_opts* o, bool allow_poll) {
    HIPCHK(hipEventRecord(s->enc_done, s->enc_stream ? s->enc_stream : m->stream));  // encoder + cross K/V of this state
    static const bool trace_phase = wm_env("WM_TRACE_HOST") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    static const bool no_graph = wm_env("WM_NO_GRAPH") != nullptr;
    s->step = wm_state::StepKey{};      // the loop step of this pass
    TsRules& rules = s->step.rules;  // timestamp rules of this pass (tb <= 0: off)
    rules.tb = o->timestamp_begin > 0 ? o->timestamp_begin : 0;
    rules.eos = o->eot;
    rules.max_init = o->max_initial_timestamp_index;
    rules.vocab = m->cfg.dims.vocab;
    const TsRules* rp = rules.tb > 0 ? &rules : nullptr;
    const int no_ts = rp ? o->no_timestamps_token : -1;
    s->shares_chip = !allow_poll;  // the pipelined entry (wm_transcribe_submit): other passes are, or will be, in flight
    s->step.eot = o->eot;
    s->step.ignore_eot = o->ignore_eot;
    s->step.shares_chip = s->shares_chip;
    if (s->al.on) s->step.cap = wm_state::StepKey::Cap{s->al.cap.p, s->al.L, s->al.n_prompt, s->al.pairs};
    s->step.rows = s->rw.on;
    s->step.lp = s->lp.on;
    s->step.rp = s->rp.on;
    s->step.sb = s->rp.sb;
    s->step.top_k = s->tk.k;
    const bool recapture = !s->graphs_valid || !(s->graph_step == s->step);
    const int first_pos = o->pos_mode == WM_POS_REF ? o->n_prompt - 1 : o->n_prompt;
    // logit masks (§8f rank 4): rebuilt only when the id lists change; always passed (all-zero = the reference's raw argmax)
    {
        std::vector<int32_t> sup(o->suppress_tokens, o->suppress_tokens + (o->suppress_tokens ? o->n_suppress : 0));
        std::vector<int32_t> bsup(o->begin_suppress_tokens, o->begin_suppress_tokens + (o->begin_suppress_tokens ? o->n_begin_suppress : 0));
        if (!s->masks_valid || sup != s->sup_cached || bsup != s->bsup_cached || no_ts != s->no_ts_cached) {
            std::vector<float> ms(m->Vpad, 0.f), mb(m->Vpad, 0.f);
            if (no_ts >= 0 && no_ts < m->cfg.dims.vocab) ms[no_ts] = mb[no_ts] = -INFINITY;  // <|notimestamps|> is never emitted under the timestamp rules
            s->no_ts_cached = no_ts;
            for (int32_t id : sup)
                if (id >= 0 && id < m->cfg.dims.vocab) ms[id] = mb[id] = -INFINITY;
            for (int32_t id : bsup)
                if (id >= 0 && id < m->cfg.dims.vocab) mb[id] = -INFINITY;
            HIPCHK(hipMemcpy(s->mask_steady.p, ms.data(), ms.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(s->mask_begin.p, mb.data(), mb.size() * 4, hipMemcpyHostToDevice));
            s->sup_cached = sup;
            s->bsup_cached = bsup;
            s->masks_valid = true;
        }
    }
    InitTokensParams ip{};
    ip.n_prompt = o->n_prompt;
    if (!s->rw.on)  // (per-row prompts: o->n_prompt is the longest row's length, the ids come from the device table)
        for (int i = 0; i < o->n_prompt; ++i) ip.prompt[i] = o->prompt[i];
    for (auto& ln : s->lanes) {
        const DecView v{ln.b0, ln.nb, ln.st, ln.ctl};
        HIPCHK(hipStreamWaitEvent(v.st, s->enc_done, 0));
        trace_mark(v.st, "state %p lane %d decode start", (void*)s, v.b0);
        // tokens = prompt (whisper.mojo:187-191, 200-202); finished = 0; control block = 0
        ip.out_tokens = lane_ptr<int>(s->out_tokens, v, s->out_stride);
        ip.out_stride = s->out_stride;
        ip.n_tokens = lane_ptr<int>(s->n_tokens, v, 1);
        ip.finished = lane_ptr<int>(s->finished, v, 1);
        ip.ctl = v.ctl;
        ip.B = v.nb;
        ip.tok_rows = s->lanes.size() == 1 ? s->tok_rows.as<int>() : nullptr;
        ip.pos_rows = s->pos_rows.as<int>();
        ip.ts_state = rp ? lane_ptr<TsState>(s->ts_state, v, 1) : nullptr;
        ip.rules = rules;
        ip.logprobs = s->lp.on ? lane_ptr<float>(s->lp.table, v, s->out_stride) : nullptr;
        ip.lp_sum = s->lp.on ? lane_ptr<float>(s->lp.sum, v, 1) : nullptr;
        if (s->rw.on) {
            WMCHK(prefill_rows(m, s, v, ip, o, rp));
        } else {
            launch_init_tokens(ip, v.st);
            if (s->rp.on) repeat_init(s, v);
            if (s->rp.sb) WMCHK(seq_bias_init(s, v, o->eot));
            // prefill (whisper.mojo:195, start_pos=0): the q_len = n_prompt causal block equals n_prompt single-token steps
            static const bool seq_prefill = wm_env("WM_SEQ_PREFILL") != nullptr;  // A/B: one pass per prompt position
            DecPass prompt;  // the last prompt position's logits, under the begin mask
            prompt.logits = Logits::partials;
            prompt.mask = s->mask_begin.as<float>();
            prompt.rules = rp;
            if (!seq_prefill && s->lanes.size() == 1 && o->n_prompt > 1 && o->n_prompt <= wm_state::PREFILL_MAX) {
                prompt.P = o->n_prompt;  // init_tokens filled tok_rows / pos_rows
                WMCHK(decode_core(m, s, v, prompt));
                if (s->ns.on) ns_capture(m, s, v, (size_t)(o->n_prompt - s->ns.n_init) * v.nb);
            } else {
                for (int i = 0; i < o->n_prompt; ++i) {
                    launch_set_step(v.ctl, i, 1, lane_ptr<int>(s->pos, v, 1), i, lane_ptr<int>(s->tok, v, 1), o->prompt[i], v.nb, v.st);
                    prompt.logits = i == o->n_prompt - 1 ? Logits::partials : Logits::none;
                    WMCHK(decode_core(m, s, v, prompt));
                    if (s->ns.on && i == o->n_prompt - s->ns.n_init) ns_capture(m, s, v, 0);
                }
            }
            LCHK(launch_argmax_step(argmax_first_id(m, s, v, o->eot, o->ignore_eot, rp), v.st));  // :198-203
            WMCHK(topk_select(m, s, v, prompt.mask));
            trace_mark(v.st, "state %p lane %d prefill end", (void*)s, v.b0);
            // incremental steps: start_pos = current_len - 1 (reference, :217) or current_len (HF)
            launch_set_step(v.ctl, o->n_prompt, 1, lane_ptr<int>(s->pos, v, 1), first_pos, nullptr, 0, v.nb, v.st);
        }
        // input row of the first loop step; every later step's row is written by the preceding step's argmax launch
        launch_dec_embed(m->tok_emb_f.as<float>(), m->dec_pos.as<float>(), lane_ptr<int>(s->tok, v, 1), lane_ptr<int>(s->pos, v, 1),
                         lane_ptr<float>(s->dx, v, m->cfg.dims.d_model), v.nb, m->cfg.dims.d_model, v.st);
        if (s->ns.on) WMCHK(ns_probe(m, s, v));  // between prefill and loop, outside the captured step
        // steady state: one captured graph per lane = [37 decode-step launches + argmax/bookkeeping]; every per-step
        // quantity (token, position, cache length) lives in HBM, so the same graph is replayed for every token
        if (!no_graph && (recapture || !ln.graph[0])) {
            for (auto& ge : ln.graph) {
                if (ge) (void)hipGraphExecDestroy(ge);
                ge = nullptr;
            }
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(v.st, hipStreamCaptureModeThreadLocal));
            const int crc = loop_step(m, s, v);
            const hipError_t cap = hipStreamEndCapture(v.st, &g);  // always closed, also when a launcher refused
            if (crc) {
                if (g) (void)hipGraphDestroy(g);
                return crc;
            }
            HIPCHK(cap);
            hipError_t ge = hipSuccess;
            for (int k = 0; k < wm_state::Lane::NEXEC && ge == hipSuccess; ++k) ge = hipGraphInstantiate(&ln.graph[k], g, nullptr, nullptr, 0);
            (void)hipGraphDestroy(g);
            if (ge != hipSuccess) return fail(WM_E_HIP, "hipGraphInstantiate: %s", hipGetErrorString(ge));
        }
    }
    s->graphs_valid = !no_graph;
    s->graph_step = s->step;
    if (trace_phase) {
        for (auto& ln : s->lanes) (void)hipStreamSynchronize(ln.st);
        fprintf(stderr, "[wm] encoder wait + prefill (+graph capture if any): %.3f ms\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - tp0).count() * 1e3);
    }
    // The loop itself.  Fixed-length passes (ignore_eot: the bench's "fixed" mode) and short loops are enqueued whole.  With the
    // reference's stop rule the loop goes out in sub-chunks of LOOP_CHUNK graph replays, two sub-chunks ahead of the GPU; before
    // each further sub-chunk the host reads the (finished, length) pair the argmax launches write to pinned memory — no stream
    // synchronisation, the GPU never runs dry — and stops enqueueing once every utterance has emitted eot: "if next_token == eot:
    // break" (whisper.mojo:206-207) for the whole batch, at most two sub-chunks late.
    s->loop_total = o->max_loop;
    s->loop_enq = 0;
    s->chunk_k = 0;
    s->enq_rc = 0;
    s->enq_err.clear();
    s->h_prog[0] = 0;
    s->h_prog[1] = 0;
    const bool natural = !o->ignore_eot && s->lanes.size() == 1 && o->max_loop > 2 * LOOP_CHUNK && !no_graph;
    s->enq_done.store(false);
    if (!natural) {
        WMCHK(enqueue_loop_steps(m, s, o->max_loop));
        return finish_enqueue(m, s);
    }
    WMCHK(enqueue_chunk(m, s));
    WMCHK(enqueue_chunk(m, s));
    if (allow_poll) {  // the synchronous entry pumps its own loop
        while (!s->enq_done.load()) WMCHK(pump_step(m, s, true) < 0 ? s->enq_rc : 0);
        return 0;
    }
    {  // pipelined entry: the model's pump thread carries on; wm_transcribe_wait waits for it
        std::lock_guard<std::mutex> lk(m->pump_mu);
        if (!m->pump.joinable()) m->pump = std::thread(pump_main, m);
        m->pump_work.push_back(s);
    }
    m->pump_cv.notify_all();
    return 0;
}

static int check_opts(wm_model* m, const wm_decode_opts* o, int B) {
    if (!o || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (!o->prompt || o->n_prompt <= 0 || o->n_prompt > 16 || o->max_loop < 0) return fail(WM_E_ARG, "bad decode options (1 <= n_prompt <= 16)");
    if (o->n_suppress < 0 || o->n_begin_suppress < 0 || (o->n_suppress > 0 && !o->suppress_tokens) || (o->n_begin_suppress > 0 && !o->begin_suppress_tokens))
        return fail(WM_E_ARG, "bad suppress-token lists");
    const wm_dims& c = m->cfg.dims;
    if (o->timestamp_begin > 0) {
        if (o->timestamp_begin >= c.vocab) return fail(WM_E_ARG, "timestamp_begin %d is not a vocabulary id", o->timestamp_begin);
        if (o->no_timestamps_token >= c.vocab) return fail(WM_E_ARG, "no_timestamps_token out of range");
        if (o->eot < 0 || o->eot > o->timestamp_begin) return fail(WM_E_ARG, "timestamp rules need 0 <= eot <= timestamp_begin (eot is the processor's eos id)");
    }
    const int total = o->n_prompt + 1 + o->max_loop;
    if (total > c.n_text_ctx + 1 || total > OUT_STRIDE_MAX)
        return fail(WM_E_ARG, "n_prompt + 1 + max_loop = %d exceeds the decoder context %d", total, c.n_text_ctx);
    for (int i = 0; i < o->n_prompt; ++i)
        if (o->prompt[i] < 0 || o->prompt[i] >= c.vocab) return fail(WM_E_ARG, "prompt id out of range");
    return 0;
}

static int align_setup(wm_model* m, wm_state* s, const wm_decode_opts* o, const std::vector<int32_t>* cols, const WinAsk* win);
static int score_pass(wm_model* m, wm_state* s, const ScoreAsk& a);
static int rows_setup(wm_model* m, wm_state* s, const RowPrompts* rows) {
    wm_state::Rows& rw = s->rw;
    rw.on = rows != nullptr;
    if (!rw.on) return 0;
    if (s->lanes.size() != 1) {
        rw.on = false;
        return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    }
    const size_t B = s->B, ctx = m->cfg.dims.n_text_ctx;
    WMCHK(grow(rw.table, B * ctx * 4));
    WMCHK(grow(rw.len, B * 4));
    WMCHK(grow(rw.key_lo, B * 4));
    WMCHK(grow(s->tok_rows, B * ctx * 4));  // the whole prompt's position-major rows [Lmax][B], consumed chunk by chunk
    WMCHK(grow(s->pos_rows, B * ctx * 4));
    rw.Lmax = rows->Lmax;
    rw.stride = rows->Lmax;
    rw.h_table.assign(B * (size_t)rw.stride, 0);
    rw.h_len.assign(rows->len, rows->len + B);
    for (size_t b = 0; b < B; ++b) std::copy(rows->ids + b * rows->stride, rows->ids + b * rows->stride + rows->len[b], rw.h_table.begin() + b * rw.stride);
    return 0;
}
// Enqueues one whole pass (encoder, prefill, greedy loop) for ask.B utterances on state *slot (created / re-created on demand).
// ask.mel2 != null: a coalesced pair — *slot is a 2·(B/2)-row pair state.
static int submit_on(wm_model* m, wm_state** slot, const PassAsk& ask) {
    const wm_dims& c = m->cfg.dims;
    const int B = ask.B;
    const wm_decode_opts* o = ask.opts;
    const bool lp = ask.lp;
    const std::vector<int32_t>* cols = ask.cols;
    const RowPrompts* rows = ask.rows;
    const NsAsk& ns = ask.ns;
    const LangAsk& lang = ask.lang;
    const ScoreAsk* score = ask.score;
    if (score && (ask.mel2 || cols || rows || lp || ns.token >= 0 || lang.ids || dec_lanes_for(B) != 1))  // (refused by the entry points first)
        return fail(WM_E_ARG, "a score pass runs alone on a single-lane decode state");
    if (lang.ids && (ask.mel2 || cols || dec_lanes_for(B) != 1 || (!lang.only && !rows)))  // (refused by the entry points first)
        return fail(WM_E_ARG, "language detection needs a single-lane decode state and a per-row-prompt pass without token timestamps");
    if (ns.token >= 0 && (!lp || ns.token >= c.vocab || ns.n_init < 1 || ns.n_init > o->n_prompt))  // (refused by the entry points first)
        return fail(WM_E_ARG, "the no-speech probe needs a log-prob pass, a vocabulary id and 1 <= n_init <= prompt length");
    if (lp && (cols || dec_lanes_for(B) != 1))  // (the entry points refuse both before anything is touched; kept for internal callers)
        return fail(WM_E_ARG, "log-probabilities need a single-lane decode state and a pass without token timestamps");
    if ((ask.win && (!cols || ask.mel2)) || (rows && cols && !ask.win))  // (no entry point asks for either)
        return fail(WM_E_ARG, "per-row prompts take token timestamps in a long-form window pass only, and a window pass runs alone");
    HIPCHK(hipSetDevice(m->device));
    const bool pair = ask.mel2 != nullptr;
    // a pass that was submitted and not yet waited for owns the slot's state: refuse BEFORE touching it (re-creating the
    // state for another batch size would destroy graphs, streams and arenas under its running kernels)
    if (*slot && (*slot)->pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    if (!*slot || (*slot)->B != B) {
        if (*slot) wm_state_free(*slot);
        *slot = nullptr;
        WMCHK(state_new(m, B, slot, pair));
    }
    wm_state* s = *slot;
    WMCHK(rows_setup(m, s, rows));
    s->ns.on = ns.token >= 0;
    s->ns.token = ns.token;
    s->ns.n_init = ns.n_init;
    s->lg.on = lang.ids != nullptr && !lang.only;
    if (lang.ids) {
        s->lg.n = lang.n;
        s->lg.n_init = lang.n_init;
        s->lg.sot = lang.sot;
        s->lg.h_ids.assign(lang.ids, lang.ids + lang.n);
        s->lg.h_col.resize(B);
        for (int b = 0; b < B; ++b) s->lg.h_col[b] = rows ? rows->len[b] - lang.n_init + 1 : 0;
    }
    s->sc.on = false;
    s->sc.timed = s->sc.timed_al = false;
    s->rp.on = ask.rp.on() && !score && !lang.only;  // greedy passes only: score / align are teacher-forced, detection reads raw logits
    if (s->rp.on) {
        s->rp.ask = ask.rp;
        s->rp.words = repeat_words(c.vocab);
        WMCHK(grow(s->rp.seen, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.ban, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.ctl, sizeof(RepeatCtl)));
    }
    s->rp.sb = s->rp.on && ask.rp.sb;
    if (s->rp.sb) {
        WMCHK(grow(s->rp.hit, (size_t)B * s->rp.words * 4));
        WMCHK(grow(s->rp.val, (size_t)B * SEQ_BIAS_MAX * sizeof(SeqSlot)));
        WMCHK(grow(s->rp.sbctl, sizeof(SeqBiasCtl)));
    } else {
        s->rp.ask.sb.reset();  // (a pass without the table holds no reference to one)
    }
    s->lp.on = lp;
    s->tk.k = lp && !score && !lang.only ? ask.top_k : 0;  // the alternatives of a greedy log-prob pass; every other pass ignores the setting
    s->tk.gen += 1;
    if (lp) {
        if (rows)
            s->lp.n_prompt.assign(rows->len, rows->len + B);
        else
            s->lp.n_prompt.assign(B, o->n_prompt);
    }
    s->trace_id = slot == &m->cached ? 1 : (slot >= m->slots && slot < m->slots + (wm_model::NSLOT - 1)) ? 2 + (int)(slot - m->slots)
                : (slot == &m->lf.st[0] || slot == &m->lf.st[1]) ? 20 + (int)(slot - m->lf.st) : 10 + (int)(slot - m->pairs);
    // The whole pass — encoder, prefill, greedy loop — goes on the slot's own stream: four slots are then four hardware
    // queues, which is what the chip runs concurrently (a fifth queue, e.g. a shared encoder stream, lands on a pipe that
    // already serves one of them and the two take turns: 22.3 vs 20.8 ms per pass at four passes in flight).
    // WM_ENC_ON_MODEL_STREAM=1 restores the shared encoder stream for A/B runs.
    static const bool enc_on_lane = wm_env("WM_ENC_ON_MODEL_STREAM") == nullptr;
    hipStream_t est = enc_on_lane ? s->lanes[0].st : m->stream;
    s->has_enc = s->has_cross = false;
    s->host_len = 0;
    if (est != m->stream) {  // whatever produced the mel on the model stream (the log-mel front end) comes first
        HIPCHK(hipEventRecord(s->enc_done, m->stream));
        HIPCHK(hipStreamWaitEvent(est, s->enc_done, 0));
    }
    const size_t mel_floats = (size_t)c.n_mels * 2 * c.n_audio_ctx;  // per utterance
    const int B1 = pair ? B / 2 : B;
    const float* mel_dev = ask.mel;
    if (!ask.mel_on_device) {
        HIPCHK(hipMemcpyAsync(s->mel_dev.p, ask.mel, (size_t)B1 * mel_floats * 4, hipMemcpyHostToDevice, est));
        mel_dev = s->mel_dev.as<float>();
    }
    const float* mel2_dev = ask.mel2;
    if (pair && !ask.mel2_on_device) {
        float* dst = s->mel_dev.as<float>() + (size_t)B1 * mel_floats;
        HIPCHK(hipMemcpyAsync(dst, ask.mel2, (size_t)B1 * mel_floats * 4, hipMemcpyHostToDevice, est));
        mel2_dev = dst;
    }
    if (score) {
        for (auto& e : s->sc.ev)
            if (!e) HIPCHK(hipEventCreate(&e));
        s->sc.timed = false;
        HIPCHK(hipEventRecord(s->sc.ev[0], est));
    }
    const auto tt0 = std::chrono::steady_clock::now();
    trace_mark(est, "state %p encoder start", (void*)s);
    WMCHK(run_encoder(m, s, mel_dev, B, est, mel2_dev, B1, false));
    trace_mark(est, "state %p encoder end", (void*)s);
    s->enc_stream = est;
    s->has_enc = s->has_cross = true;
    s->last_mel = pair ? nullptr : mel_dev;
    if (wm_env("WM_TRACE_HOST")) {
        const auto tt1 = std::chrono::steady_clock::now();
        (void)hipStreamSynchronize(m->stream);
        fprintf(stderr, "[wm] encoder: enqueue %.3f ms, done after %.3f ms\n", std::chrono::duration<double>(tt1 - tt0).count() * 1e3,
                std::chrono::duration<double>(std::chrono::steady_clock::now() - tt0).count() * 1e3);
    }
    if (lang.only) {  // wm_detect_language: the [sot] pass and the kernel behind the encoder, no transcription
        const wm_state::Lane& ln = s->lanes[0];
        HIPCHK(hipEventRecord(s->enc_done, est));
        HIPCHK(hipStreamWaitEvent(ln.st, s->enc_done, 0));
        WMCHK(lang_pass(m, s, DecView{ln.b0, ln.nb, ln.st, ln.ctl}, nullptr, 0));
        HIPCHK(hipGetLastError());
        s->has_enc = false;  // cache slot 0 holds the [sot] pass: a new wm_encode is needed before wm_decode_step
        return 0;
    }
    if (score) {  // teacher-forced prefill + the vocabulary side on the lane's stream: no loop, no graph, no pump
        s->al.on = false;
        s->shares_chip = !ask.allow_poll;
        WMCHK(score_pass(m, s, *score));
        s->pending = true;
        s->synced = false;
        s->halves_left = 1;
        s->pend_total = score->stride;
        return 0;
    }
    s->al.ragged = false;
    WMCHK(align_setup(m, s, o, cols, ask.win));
    WMCHK(transcribe_decode(m, s, o, ask.allow_poll));
    s->pending = true;
    s->synced = false;
    s->halves_left = pair ? 2 : 1;
    s->pend_total = o->n_prompt + 1 + o->max_loop;
    s->host_len = 0;
    return 0;
}

// Blocks until the state's pending pass is complete, then copies `rows` utterances starting at row0 out.  The pass stays pending
// until every slot that shares the state (one, or the two of a coalesced pair) has collected its rows.
static int wait_on(wm_model* m, wm_state* s, int row0, int rows, const PassOut& out) {
    if (!s || !s->pending) return fail(WM_E_STATE, "nothing was submitted on this slot");
    HIPCHK(hipSetDevice(m->device));
    if (rows < 0) rows = s->B;
    if (!s->synced) {
        if (!s->enq_done.load()) {  // the loop pump is still feeding this pass
            std::unique_lock<std::mutex> lk(m->pump_mu);
            m->pump_cv.wait(lk, [&] { return s->enq_done.load(); });
        }
        if (s->enq_rc) {
            s->pending = false;
            for (auto& ln : s->lanes) (void)hipStreamSynchronize(ln.st);
            return fail(s->enq_rc, "%s", s->enq_err.c_str());
        }
        for (auto& ln : s->lanes) HIPCHK(hipEventSynchronize(ln.done));
        s->synced = true;
    }
    const int total = s->pend_total;
    if (out.dev_packed) {  // the gather buffer, built on the device in the caller's DEVICE memory (no host round trip before the collective)
        launch_pack_tokens(s->out_tokens.as<int>() + (size_t)row0 * s->out_stride, s->n_tokens.as<int>() + row0, s->out_stride, rows, out.rows_cap,
                           out.pack_stride, out.dev_packed, s->lanes[0].st);
        HIPCHK(hipGetLastError());
        if (out.dev_times)
            HIPCHK(hipMemcpy2DAsync(out.dev_times, (size_t)out.pack_stride * 4, s->al.times.as<float>() + (size_t)row0 * s->out_stride,
                                    (size_t)s->out_stride * 4, (size_t)total * 4, rows, hipMemcpyDeviceToDevice, s->lanes[0].st));
        HIPCHK(hipStreamSynchronize(s->lanes[0].st));  // the caller's collective runs on another stream
    } else {
        HIPCHK(hipMemcpy2D(out.tokens, (size_t)total * 4, s->out_tokens.as<int>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4, (size_t)total * 4, rows,
                           hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out.n_tokens, s->n_tokens.as<int>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.win_times)  // (the caller's pass was a window pass)
            HIPCHK(hipMemcpy(out.win_times, (const double*)s->al.wtimes.p + (size_t)row0 * (s->al.L + 1), (size_t)rows * (s->al.L + 1) * 8, hipMemcpyDeviceToHost));
        if (out.token_times)
            HIPCHK(hipMemcpy2D(out.token_times, (size_t)total * 4, s->al.times.as<float>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4,
                               (size_t)total * 4, rows, hipMemcpyDeviceToHost));
        if (out.token_logprobs) {  // (the callers checked that the pass computed them)
            HIPCHK(hipMemcpy2D(out.token_logprobs, (size_t)total * 4, s->lp.table.as<float>() + (size_t)row0 * s->out_stride, (size_t)s->out_stride * 4,
                               (size_t)total * 4, rows, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(out.avg_logprob, s->lp.sum.as<float>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
            for (int b = 0; b < rows; ++b) {  // HF _retrieve_avg_logprobs: sum / generated ids (eot included); nothing generated: 0
                const int gen = out.n_tokens[b] - s->lp.n_prompt[row0 + b];
                out.avg_logprob[b] = gen > 0 ? out.avg_logprob[b] / (float)gen : 0.f;
            }
        }
        if (out.no_speech_prob) HIPCHK(hipMemcpy(out.no_speech_prob, s->ns.prob.as<float>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.lang_out) HIPCHK(hipMemcpy(out.lang_out, s->lg.out.as<int>() + row0, (size_t)rows * 4, hipMemcpyDeviceToHost));
        if (out.lang_probs)
            HIPCHK(hipMemcpy(out.lang_probs, s->lg.probs.as<float>() + (size_t)row0 * s->lg.n, (size_t)rows * s->lg.n * 4, hipMemcpyDeviceToHost));
    }
    if (--s->halves_left <= 0) {
        s->pending = false;
        s->has_enc = false;  // the KV cache now holds a finished decode: a new wm_encode is needed before wm_decode_step
    }
    return 0;
}

static wm_state** slot_state(wm_model* m, int slot) { return slot == 0 ? &m->cached : &m->slots[slot - 1]; }

// ---- the slot protocol: what a slot holds, and the three drivers every entry point ends in -----------------------------
// The one place a SlotRef is filled: the slot holds rows [row0, row0 + rows) of the pass `a`, on state st (null: only held so far).
static void record_pass(wm_model* m, int slot, const PassAsk& a, wm_state* st, int row0, int rows) {
    wm_model::SlotRef& r = m->slot_ref[slot];
    r = wm_model::SlotRef();
    r.pending = true;
    r.st = st;
    r.row0 = row0;
    r.rows = rows;
    r.kind = !a.score ? PassKind::transcribe : a.score->cols ? PassKind::align : PassKind::score;
    r.total = a.score ? a.score->stride : a.opts->n_prompt + 1 + a.opts->max_loop;
    r.tt = a.cols != nullptr;
    r.lp = a.score ? a.score->lp : a.lp;
    r.ns = a.ns.token >= 0;
    r.lang = a.lang.ids != nullptr;
}
static int score_collect(wm_model* m, wm_state* s, const PassOut& out);
// Collects the slot's rows and releases the slot.  The one place that says what the slot remembers of a collected pass: the loop
// steps of a transcribe pass, and a reference to the alignment weights of a pass that computed some (token timestamps, or an align
// pass that succeeded) — every other pass clears that reference, for its state's weights are no longer this slot's last pass's.
static int collect_pass(wm_model* m, int slot, const PassOut& out) {
    wm_model::SlotRef& r = m->slot_ref[slot];
    wm_state* s = r.st;
    const bool transcribe = r.kind == PassKind::transcribe;
    const int rc = transcribe ? wait_on(m, s, r.row0, r.rows, out) : score_collect(m, s, out);
    if (!rc && transcribe) m->last_steps[slot] = s->last_steps;
    const bool weights = !rc && (r.tt || r.kind == PassKind::align);
    m->align_ref[slot] = weights ? wm_model::AlignRef{s, r.row0, r.rows, s->al.gen} : wm_model::AlignRef();
    m->topk_ref[slot] = !rc && transcribe && r.lp && s->tk.k > 0 ? wm_model::TopkRef{s, r.row0, r.rows, r.total, s->tk.k, s->tk.gen} : wm_model::TopkRef();
    r = wm_model::SlotRef();
    return rc;
}

// ---- coalescing of consecutive submits (wm_config.coalesce == 2) ------------------------------------------------------------------
// May this submit share a pass with the held one: the same batch size, outputs asked for and options.
static bool pairs_with(const wm_model::Held& h, const PassAsk& b) {
    const PassAsk& a = h.ask;
    const wm_decode_opts &x = h.o, *o = b.opts;
    if (a.B != b.B || (a.cols != nullptr) != (b.cols != nullptr) || a.lp != b.lp || a.ns.token != b.ns.token || a.ns.n_init != b.ns.n_init)
        return false;
    if (a.top_k != b.top_k) return false;  // one step graph per state: a pair shares the top-k setting
    if (!(a.rp == b.rp)) return false;  // one control block per state: a pair shares (penalty, n-gram size) and the sequence-bias table
    if (x.n_prompt != o->n_prompt || x.eot != o->eot || x.max_loop != o->max_loop || x.pos_mode != o->pos_mode || x.ignore_eot != o->ignore_eot ||
        x.n_suppress != (o->suppress_tokens ? o->n_suppress : 0) || x.n_begin_suppress != (o->begin_suppress_tokens ? o->n_begin_suppress : 0) ||
        x.timestamp_begin != o->timestamp_begin || x.no_timestamps_token != o->no_timestamps_token ||
        x.max_initial_timestamp_index != o->max_initial_timestamp_index)
        return false;
    return std::equal(h.prompt.begin(), h.prompt.end(), o->prompt) && std::equal(h.sup.begin(), h.sup.end(), o->suppress_tokens) &&
           std::equal(h.bsup.begin(), h.bsup.end(), o->begin_suppress_tokens);
}
static void hold(wm_model* m, int slot, const PassAsk& a) {
    wm_model::Held& h = m->held;
    const wm_decode_opts* o = a.opts;
    h.active = true;
    h.slot = slot;
    h.prompt.assign(o->prompt, o->prompt + o->n_prompt);
    h.sup.assign(o->suppress_tokens, o->suppress_tokens + (o->suppress_tokens ? o->n_suppress : 0));
    h.bsup.assign(o->begin_suppress_tokens, o->begin_suppress_tokens + (o->begin_suppress_tokens ? o->n_begin_suppress : 0));
    h.cols = a.cols ? *a.cols : std::vector<int32_t>();
    h.o = *o;
    h.o.prompt = h.prompt.data();
    h.o.suppress_tokens = h.sup.empty() ? nullptr : h.sup.data();
    h.o.n_suppress = (int)h.sup.size();
    h.o.begin_suppress_tokens = h.bsup.empty() ? nullptr : h.bsup.data();
    h.o.n_begin_suppress = (int)h.bsup.size();
    h.ask = a;
    h.ask.opts = &h.o;
    h.ask.cols = a.cols ? &h.cols : nullptr;
    record_pass(m, slot, h.ask, nullptr, 0, a.B);
}
// the held submit runs alone, on its own slot's state (no partner came, or the partner did not match)
static int flush_held(wm_model* m) {
    wm_model::Held& h = m->held;
    if (!h.active) return 0;
    h.active = false;
    const int rc = submit_on(m, slot_state(m, h.slot), h.ask);
    if (rc) {
        m->slot_ref[h.slot] = wm_model::SlotRef();
        return rc;
    }
    record_pass(m, h.slot, h.ask, *slot_state(m, h.slot), 0, h.ask.B);
    return 0;
}

// ---- the drivers --------------------------------------------------------------------------------------------------------------------
// The synchronous entries run on slot 0.  A held submit goes first: this call may use its mel buffers' stream order, and slot 0.
static int slot0_ready(wm_model* m) {
    WMCHK(flush_held(m));
    if (m->slot_ref[0].pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    return 0;
}
static int run_now(wm_model* m, PassAsk ask, const PassOut& out) {
    WMCHK(slot0_ready(m));
    ask.allow_poll = true;
    ask.rp = m->repeat;
    ask.top_k = m->top_k;
    WMCHK(submit_on(m, &m->cached, ask));
    record_pass(m, 0, ask, m->cached, 0, ask.B);
    return collect_pass(m, 0, out);
}
// Pipelined form of Whisper.transcribe for back-to-back batches: submit enqueues the encoder and the greedy loop on the slot's
// stream and returns; the slot's wait blocks until its results are ready.  A pending slot is refused BEFORE a held submit is flushed.
static int submit_slot(wm_model* m, int slot, const PassAsk& asked) {
    if (m->slot_ref[slot].pending) return fail(WM_E_STATE, "this slot still holds a pass that was not waited for");
    PassAsk ask = asked;
    ask.rp = m->repeat;  // the setting in force now: a held submit runs with it even if it changes before the partner arrives
    ask.top_k = m->top_k;
    const int B = ask.B;
    // (a per-row, language or score / align pass is never held for a coalesce = 2 partner: it runs alone)
    const bool can_pair = !ask.rows && !ask.lang.ids && !ask.score && m->cfg.coalesce == 2 && B <= m->cfg.max_batch &&
                          (B <= m->enc_chunk || B % m->enc_chunk == 0);
    if (can_pair && m->held.active && pairs_with(m->held, ask)) {
        // the partner of the held submit: both batches go out as ONE pass on a 2·B-row state
        wm_state** ps = nullptr;
        for (auto& pr : m->pairs)
            if (pr && !pr->pending && pr->B == 2 * B) ps = &pr;
        for (auto& pr : m->pairs)
            if (!ps && !pr) ps = &pr;
        for (auto& pr : m->pairs)
            if (!ps && !pr->pending) ps = &pr;  // another batch size: re-created
        if (ps) {
            wm_model::Held& h = m->held;
            h.active = false;
            PassAsk both = h.ask;
            both.B = 2 * B;
            both.mel2 = ask.mel;
            both.mel2_on_device = ask.mel_on_device;
            std::vector<int32_t> pair_cols;
            if (ask.cols) {  // rows [0, B) are the held batch's, [B, 2B) this one's
                pair_cols = h.cols;
                pair_cols.insert(pair_cols.end(), ask.cols->begin(), ask.cols->end());
                both.cols = &pair_cols;
            }
            const int rc = submit_on(m, ps, both);
            if (rc) {
                m->slot_ref[h.slot] = wm_model::SlotRef();
                return rc;
            }
            record_pass(m, h.slot, h.ask, *ps, 0, B);
            record_pass(m, slot, ask, *ps, B, B);
            return 0;
        }
    }
    WMCHK(flush_held(m));
    if (can_pair) {  // wait for a partner (or for this slot's wait)
        hold(m, slot, ask);
        return 0;
    }
    WMCHK(submit_on(m, slot_state(m, slot), ask));
    record_pass(m, slot, ask, *slot_state(m, slot), 0, B);
    return 0;
}
// A wait of the `kind` family on a slot: refused (the pass stays pending, collectable by the right wait) when the slot holds another
// kind of pass or one submitted without something `out` asks for.
static int collect_slot(wm_model* m, int slot, PassKind kind, const PassOut& out) {
    const wm_model::SlotRef& r = m->slot_ref[slot];
    if (!r.pending) return fail(WM_E_STATE, "nothing was submitted on this slot");
    if (r.kind != kind) {
        if (r.kind == PassKind::score) return fail(WM_E_STATE, "this slot holds a score pass (collect it with wm_score_wait)");
        if (r.kind == PassKind::align) return fail(WM_E_STATE, "this slot holds an align pass (collect it with wm_align_wait)");
        return fail(WM_E_STATE, "this slot holds a transcribe pass (collect it with wm_transcribe_wait)");
    }
    if (kind == PassKind::align) {
        if (out.token_logprobs && !r.lp) return fail(WM_E_STATE, "this slot's align pass was submitted without log-probabilities");
    } else if (kind == PassKind::transcribe) {
        if (out.lang_out && !r.lang) return fail(WM_E_STATE, "this slot's pass was submitted without language detection (wm_transcribe_submit_lang)");
        if (out.no_speech_prob && !r.ns) return fail(WM_E_STATE, "this slot's pass was submitted without the no-speech probe (wm_transcribe_submit_lp_ns)");
        if (out.token_logprobs && !r.lp) return fail(WM_E_STATE, "this slot's pass was submitted without log-probabilities (wm_transcribe_submit_lp)");
        if ((out.token_times || out.dev_times) && !r.tt)
            return fail(WM_E_STATE, "this slot's pass was submitted without token timestamps (wm_transcribe_submit_tt)");
        if (out.dev_packed && out.rows_cap < r.rows) return fail(WM_E_ARG, "rows_cap %d is smaller than the batch (%d)", out.rows_cap, r.rows);
        if (out.dev_packed && out.pack_stride < r.total)
            return fail(WM_E_ARG, "stride %d is smaller than the pass's ids per utterance (%d)", out.pack_stride, r.total);
    }
    if (m->held.active && m->held.slot == slot) WMCHK(flush_held(m));  // no partner came: the held batch runs alone now
    return collect_pass(m, slot, out);
}

// n_frames -> columns kept per row (HF crops the attentions to n_frames // 2 encoder positions); null = every column
static int align_cols(wm_model* m, const int32_t* n_frames, int B, std::vector<int32_t>& cols) {
    const int T = m->cfg.dims.n_audio_ctx;
    if (m->align_pairs.empty()) return fail(WM_E_STATE, "token timestamps need alignment heads (wm_set_alignment_heads)");
    cols.assign(B, T);
    if (n_frames)
        for (int b = 0; b < B; ++b) {
            if (n_frames[b] < 2 || n_frames[b] > 2 * T)
                return fail(WM_E_ARG, "n_frames[%d] = %d: must lie in [2, %d] (mel frames of real audio)", b, n_frames[b], 2 * T);
            cols[b] = n_frames[b] / 2;
        }
    return 0;
}

extern "C" int wm_transcribe(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                             int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !mel || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    return run_now(m, PassAsk{mel, mel_on_device, B, o}, PassOut{tokens_out, n_tokens});
}

extern "C" int wm_transcribe_tt(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* n_frames,
                                int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_times) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, n_frames, B, cols));
    PassAsk ask{mel, mel_on_device, B, o};
    ask.cols = &cols;
    return run_now(m, ask, PassOut{tokens_out, n_tokens, token_times});
}

extern "C" int wm_transcribe_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(check_opts(m, o, B));
    return submit_slot(m, slot, PassAsk{mel, mel_on_device, B, o});
}
extern "C" int wm_transcribe_submit_tt(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                       const int32_t* n_frames) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, n_frames, B, cols));
    PassAsk ask{mel, mel_on_device, B, o};
    ask.cols = &cols;
    return submit_slot(m, slot, ask);
}
// ---- per-row prompts -----------------------------------------------------------------------------------------------
// Everything is checked before anything is launched.  o2: the options the pass runs with (n_prompt = the longest row).
static int rows_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* prompts, const int32_t* prompt_len, int prompt_stride,
                      wm_decode_opts& o2, RowPrompts& rows) {
    if (!o || B <= 0 || !prompts || !prompt_len || prompt_stride <= 0) return fail(WM_E_ARG, "bad argument");
    o2 = *o;
    o2.prompt = prompts;  // (ignored by a per-row pass; the generic checks want one valid id)
    o2.n_prompt = 1;
    const wm_dims& c = m->cfg.dims;
    int Lmax = 0;
    for (int b = 0; b < B; ++b) {
        const int L = prompt_len[b];
        if (L < 1 || L > prompt_stride) return fail(WM_E_ARG, "prompt_len[%d] = %d outside [1, prompt_stride = %d]", b, L, prompt_stride);
        for (int i = 0; i < L; ++i) {
            const int32_t id = prompts[(size_t)b * prompt_stride + i];
            if (id < 0 || id >= c.vocab) return fail(WM_E_ARG, "prompt id %d of row %d out of range", id, b);
        }
        Lmax = std::max(Lmax, L);
    }
    WMCHK(check_opts(m, &o2, B));
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    if (o->max_loop < 0 || Lmax + 1 + o->max_loop > c.n_text_ctx)
        return fail(WM_E_ARG, "longest prompt %d + 1 + max_loop %d exceeds the decoder context %d", Lmax, o->max_loop, c.n_text_ctx);
    o2.n_prompt = Lmax;
    rows = RowPrompts{prompts, prompt_len, prompt_stride, Lmax};
    return 0;
}
extern "C" int wm_transcribe_rows(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                  const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !mel || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    return run_now(m, ask, PassOut{tokens_out, n_tokens});
}
extern "C" int wm_transcribe_submit_rows(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                         const int32_t* prompts, const int32_t* prompt_len, int prompt_stride) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    return submit_slot(m, slot, ask);
}
extern "C" int wm_transcribe_wait(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !tokens_out || !n_tokens || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, PassOut{tokens_out, n_tokens});
}
extern "C" int wm_transcribe_wait_tt(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !tokens_out || !n_tokens || !token_times || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, PassOut{tokens_out, n_tokens, token_times});
}
// ---- log-probabilities -----------------------------------------------------------------------------------------------
// One family for shared (prompts == NULL: opts->prompt) and per-row prompts.  Everything is refused before anything is launched.
static int lp_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* prompts, const int32_t* prompt_len, int prompt_stride,
                    wm_decode_opts& o2, RowPrompts& rows) {
    if (prompts) {
        WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    } else {
        if (prompt_len) return fail(WM_E_ARG, "prompt_len without prompts");
        WMCHK(check_opts(m, o, B));
        o2 = *o;
    }
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "log-probabilities need a single-lane decode state");
    return 0;
}
static int ns_check(wm_model* m, const wm_decode_opts& o2, int B, const int32_t* prompts, const int32_t* prompt_len, int no_speech_token, int n_init);
// The _lp and _lp_ns entries behind their null checks: slot < 0 runs the pass now, on slot 0; ns: the _lp_ns probe, as given.
static int lp_entry(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                    const int32_t* prompt_len, int prompt_stride, const NsAsk* ns, const PassOut& out) {
    wm_decode_opts o2;
    RowPrompts rows;
    WMCHK(lp_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));
    if (ns) WMCHK(ns_check(m, o2, B, prompts, prompt_len, ns->token, ns->n_init));
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = prompts ? &rows : nullptr;
    ask.lp = true;
    if (ns) ask.ns = *ns;
    return slot < 0 ? run_now(m, ask, out) : submit_slot(m, slot, ask);
}
static PassOut lp_out(int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob) {
    PassOut out{tokens_out, n_tokens};
    out.token_logprobs = token_logprobs;
    out.avg_logprob = avg_logprob;
    out.no_speech_prob = no_speech_prob;
    return out;
}
extern "C" int wm_transcribe_lp(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                const int32_t* prompt_len, int prompt_stride, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs,
                                float* avg_logprob) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    return lp_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, nullptr,
                    lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, nullptr));
}
extern "C" int wm_transcribe_submit_lp(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                       const int32_t* prompts, const int32_t* prompt_len, int prompt_stride) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    return lp_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, nullptr, PassOut());
}
extern "C" int wm_transcribe_wait_lp(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob) {
    if (!m || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, nullptr));
}
// ---- no-speech probe: the _lp trio plus the probability of no_speech_token at each row's <|startoftranscript|>
// position, prompt length - n_init.  Everything is refused before anything is launched.
static int ns_check(wm_model* m, const wm_decode_opts& o2, int B, const int32_t* prompts, const int32_t* prompt_len, int no_speech_token, int n_init) {
    if (no_speech_token < 0 || no_speech_token >= m->cfg.dims.vocab) return fail(WM_E_ARG, "no_speech_token %d is not a vocabulary id", no_speech_token);
    if (n_init < 1) return fail(WM_E_ARG, "n_init must be >= 1 (the initial ids start at <|startoftranscript|>)");
    if (prompts) {
        for (int b = 0; b < B; ++b)
            if (n_init > prompt_len[b]) return fail(WM_E_ARG, "n_init %d exceeds prompt_len[%d] = %d", n_init, b, prompt_len[b]);
    } else if (n_init > o2.n_prompt) {
        return fail(WM_E_ARG, "n_init %d exceeds the prompt length %d", n_init, o2.n_prompt);
    }
    return 0;
}
extern "C" int wm_transcribe_lp_ns(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                   const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, int32_t* tokens_out,
                                   int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob) {
    if (!m || !mel || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || !no_speech_prob) return fail(WM_E_ARG, "bad argument");
    const NsAsk ns{no_speech_token, n_init};
    return lp_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, &ns,
                    lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob));
}
extern "C" int wm_transcribe_submit_lp_ns(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                          const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    const NsAsk ns{no_speech_token, n_init};
    return lp_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, &ns, PassOut());
}
extern "C" int wm_transcribe_wait_lp_ns(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                                        float* no_speech_prob) {
    if (!m || !tokens_out || !n_tokens || !token_logprobs || !avg_logprob || !no_speech_prob || slot < 0 || slot >= wm_model::NSLOT)
        return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::transcribe, lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob));
}
// ---- language detection ----------------------------------------------------------------------------------------------
// Everything is refused before anything is launched.
int lang_list_check(int vocab, const int32_t* lang_ids, int n_lang) {
    if (n_lang < 1 || n_lang > LANG_DETECT_MAX) return fail(WM_E_ARG, "n_lang = %d outside [1, %d]", n_lang, LANG_DETECT_MAX);
    if (!lang_ids) return fail(WM_E_ARG, "bad argument");
    for (int i = 0; i < n_lang; ++i) {
        if (lang_ids[i] < 0 || lang_ids[i] >= vocab) return fail(WM_E_ARG, "language id %d is not a vocabulary id", lang_ids[i]);
        for (int j = 0; j < i; ++j)
            if (lang_ids[j] == lang_ids[i]) return fail(WM_E_ARG, "language id %d is listed twice", lang_ids[i]);
    }
    return 0;
}
// (the synchronous sequence up to the submit; the collect is its own: no ids, and the pass leaves no pending state behind)
extern "C" int wm_detect_language(wm_model* m, const float* mel, int mel_on_device, int B, int sot_token, const int32_t* lang_ids, int n_lang,
                                  int32_t* lang_out, float* probs_out) {
    if (!m || !mel || !lang_out || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "B = %d exceeds max_batch %d", B, m->cfg.max_batch);
    if (sot_token < 0 || sot_token >= m->cfg.dims.vocab) return fail(WM_E_ARG, "sot_token %d is not a vocabulary id", sot_token);
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    WMCHK(slot0_ready(m));
    WMCHK(submit_on(m, &m->cached, lang_only_ask(mel, mel_on_device, B, lang_ids, n_lang, sot_token)));
    wm_state* s = m->cached;
    HIPCHK(hipStreamSynchronize(s->lanes[0].st));
    HIPCHK(hipMemcpy(lang_out, s->lg.out.p, (size_t)B * 4, hipMemcpyDeviceToHost));
    if (probs_out) HIPCHK(hipMemcpy(probs_out, s->lg.probs.p, (size_t)B * n_lang * 4, hipMemcpyDeviceToHost));
    return 0;
}
// The _lang entries behind their null checks: the checks of a _lang pass, then slot < 0 runs it now, on slot 0.
static int lang_entry(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                      const int32_t* prompt_len, int prompt_stride, bool lp, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
                      const PassOut& out) {
    std::vector<int32_t> tab, len;  // the per-row table built from opts->prompt when prompts == NULL
    wm_decode_opts o2;
    RowPrompts rows;
    if (!prompts) {
        if (prompt_len) return fail(WM_E_ARG, "prompt_len without prompts");
        WMCHK(check_opts(m, o, B));
        tab.resize((size_t)B * o->n_prompt);
        for (int b = 0; b < B; ++b) std::copy(o->prompt, o->prompt + o->n_prompt, tab.begin() + (size_t)b * o->n_prompt);
        len.assign(B, o->n_prompt);
        prompts = tab.data();
        prompt_len = len.data();
        prompt_stride = o->n_prompt;
    }
    WMCHK(rows_check(m, o, B, prompts, prompt_len, prompt_stride, o2, rows));  // (single lane included)
    if (no_speech_token >= 0) {
        if (!lp) return fail(WM_E_ARG, "the no-speech probe needs the log-prob outputs");
        WMCHK(ns_check(m, o2, B, prompts, prompt_len, no_speech_token, n_init));
    }
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (n_init < 2) return fail(WM_E_ARG, "n_init must be >= 2 (<|startoftranscript|> and the language slot)");
    const int32_t sot = prompts[prompt_len[0] - n_init >= 0 ? prompt_len[0] - n_init : 0];
    for (int b = 0; b < B; ++b) {
        if (n_init > prompt_len[b]) return fail(WM_E_ARG, "n_init %d exceeds prompt_len[%d] = %d", n_init, b, prompt_len[b]);
        if (prompts[(size_t)b * prompt_stride + prompt_len[b] - n_init] != sot)
            return fail(WM_E_ARG, "row %d starts its initial ids with %d, row 0 with %d: one <|startoftranscript|> per pass", b,
                        prompts[(size_t)b * prompt_stride + prompt_len[b] - n_init], sot);
    }
    PassAsk ask{mel, mel_on_device, B, &o2};
    ask.rows = &rows;
    ask.lp = lp;
    if (no_speech_token >= 0) ask.ns = NsAsk{no_speech_token, n_init};
    ask.lang.ids = lang_ids;
    ask.lang.n = n_lang;
    ask.lang.n_init = n_init;
    ask.lang.sot = sot;
    return slot < 0 ? run_now(m, ask, out) : submit_slot(m, slot, ask);
}
extern "C" int wm_transcribe_lang(wm_model* m, const float* mel, int mel_on_device, int B, const wm_decode_opts* o, const int32_t* prompts,
                                  const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init, const int32_t* lang_ids, int n_lang,
                                  int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob, float* no_speech_prob,
                                  int32_t* lang_out, float* lang_probs) {
    if (!m || !mel || !tokens_out || !n_tokens || !lang_out || !o || B <= 0) return fail(WM_E_ARG, "bad argument");
    if (!token_logprobs != !avg_logprob) return fail(WM_E_ARG, "token_logprobs and avg_logprob go together");
    if (no_speech_token >= 0 && !no_speech_prob) return fail(WM_E_ARG, "bad argument");
    PassOut out = lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_token >= 0 ? no_speech_prob : nullptr);
    out.lang_out = lang_out;
    out.lang_probs = lang_probs;
    return lang_entry(m, -1, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, token_logprobs != nullptr, no_speech_token, n_init, lang_ids,
                      n_lang, out);
}
extern "C" int wm_transcribe_submit_lang(wm_model* m, int slot, const float* mel, int mel_on_device, int B, const wm_decode_opts* o,
                                         const int32_t* prompts, const int32_t* prompt_len, int prompt_stride, int no_speech_token, int n_init,
                                         const int32_t* lang_ids, int n_lang, int want_logprobs) {
    if (!m || !mel || !o || B <= 0 || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    return lang_entry(m, slot, mel, mel_on_device, B, o, prompts, prompt_len, prompt_stride, want_logprobs != 0, no_speech_token, n_init, lang_ids,
                      n_lang, PassOut());
}
extern "C" int wm_transcribe_wait_lang(wm_model* m, int slot, int32_t* tokens_out, int32_t* n_tokens, float* token_logprobs, float* avg_logprob,
                                       float* no_speech_prob, int32_t* lang_out, float* lang_probs) {
    if (!m || !tokens_out || !n_tokens || !lang_out || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    if (!token_logprobs != !avg_logprob) return fail(WM_E_ARG, "token_logprobs and avg_logprob go together");
    PassOut out = lp_out(tokens_out, n_tokens, token_logprobs, avg_logprob, no_speech_prob);
    out.lang_out = lang_out;
    out.lang_probs = lang_probs;
    return collect_slot(m, slot, PassKind::transcribe, out);
}
// ---- repetition processors -------------------------------------------------------------------------------------
extern "C" int wm_set_repeat_options(wm_model* m, float repetition_penalty, int no_repeat_ngram_size) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    if (!(repetition_penalty > 0.f) || !std::isfinite(repetition_penalty))
        return fail(WM_E_ARG, "repetition_penalty must be a finite float > 0 (1 = off)");
    if (no_repeat_ngram_size < 0 || no_repeat_ngram_size > REPEAT_NGRAM_MAX)
        return fail(WM_E_ARG, "no_repeat_ngram_size %d outside [0, %d] (0 = off)", no_repeat_ngram_size, REPEAT_NGRAM_MAX);
    m->repeat.penalty = repetition_penalty;
    m->repeat.ngram = no_repeat_ngram_size;
    return 0;
}
// ---- top-k alternatives ----------------------------------------------------------------------------------------
extern "C" int wm_set_top_k(wm_model* m, int top_k) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    if (top_k < 0 || top_k > TOPK_MAX) return fail(WM_E_ARG, "top_k %d outside [0, %d] (0 = off)", top_k, TOPK_MAX);
    m->top_k = top_k;
    return 0;
}
extern "C" int wm_transcribe_top_k(wm_model* m, int slot, int32_t* top_ids, float* top_logprobs) {
    if (!m || !top_ids || !top_logprobs || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    const wm_model::TopkRef& r = m->topk_ref[slot];
    if (!r.st || !state_is_live(r.st) || r.st->tk.gen != r.gen || (r.st->pending && r.st->synced == false))
        return fail(WM_E_STATE, "no collected log-prob pass with top_k on this slot (wm_set_top_k; or its state has run another pass since)");
    wm_state* s = r.st;
    HIPCHK(hipSetDevice(m->device));
    const size_t k = r.k, row = (size_t)r.total * k, pitch = (size_t)s->out_stride * k;
    HIPCHK(hipMemcpy2D(top_ids, row * 4, s->tk.ids.as<int>() + (size_t)r.row0 * pitch, pitch * 4, row * 4, r.rows, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy2D(top_logprobs, row * 4, s->tk.lps.as<float>() + (size_t)r.row0 * pitch, pitch * 4, row * 4, r.rows, hipMemcpyDeviceToHost));
    std::vector<int32_t> n(r.rows);
    HIPCHK(hipMemcpy(n.data(), s->n_tokens.as<int>() + r.row0, (size_t)r.rows * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < r.rows; ++b)  // prompt and tail positions were never written: id -1, log-prob 0, as the log-prob table's 0
        for (int i = 0; i < r.total; ++i)
            if (i < s->lp.n_prompt[r.row0 + b] || i >= n[b])
                for (size_t j = 0; j < k; ++j) {
                    top_ids[b * row + i * k + j] = -1;
                    top_logprobs[b * row + i * k + j] = 0.f;
                }
    return 0;
}
// ---- sequence bias and bad words ---------------------------------------------------------------------------------
// Validates both lists and builds the device table: the sequences grouped by last id (ascending), inside a group the length-1 bias
// first, then the bias sequences in the caller's order, then the bans — the order one thread sums a group in.  Nothing is allocated
// before every argument has passed.  slot_ids (optional): the groups' ids for the op hook.
int build_seq_table(std::shared_ptr<SeqTable>& out, int vocab, const int32_t* ids, const int32_t* off, const float* bias, int n_seq,
                    const int32_t* bad_ids, const int32_t* bad_off, int n_bad, std::vector<int32_t>* slot_ids) {
    if (n_seq < 0 || n_bad < 0 || (n_seq > 0 && (!ids || !off || !bias)) || (n_bad > 0 && (!bad_ids || !bad_off))) return fail(WM_E_ARG, "bad argument");
    if ((long long)n_seq + n_bad > SEQ_BIAS_MAX) return fail(WM_E_ARG, "%d + %d sequences: at most %d over the two lists", n_seq, n_bad, SEQ_BIAS_MAX);
    struct Ent {
        const int32_t* p;
        int len, ban, order;
        float bias;
    };
    std::vector<Ent> es;
    for (int list = 0; list < 2; ++list) {
        const int n = list ? n_bad : n_seq;
        const int32_t *id = list ? bad_ids : ids, *o = list ? bad_off : off;
        const char* what = list ? "bad_words_ids" : "sequence_bias";
        std::set<std::vector<int32_t>> had;
        if (n > 0 && o[0] != 0) return fail(WM_E_ARG, "%s: offsets start at 0", what);
        for (int q = 0; q < n; ++q) {
            const long long len = (long long)o[q + 1] - o[q];
            if (len < 1 || len > SEQ_BIAS_LEN_MAX) return fail(WM_E_ARG, "%s: sequence %d has %lld ids, need 1..%d", what, q, len, SEQ_BIAS_LEN_MAX);
            for (int k = 0; k < (int)len; ++k)
                if (id[o[q] + k] < 0 || id[o[q] + k] >= vocab) return fail(WM_E_ARG, "%s: sequence %d holds id %d outside the vocabulary of %d", what, q, id[o[q] + k], vocab);
            if (!had.insert(std::vector<int32_t>(id + o[q], id + o[q + 1])).second) return fail(WM_E_ARG, "%s: sequence %d is a duplicate", what, q);
            if (!list && !(std::isfinite(bias[q]) || (std::isinf(bias[q]) && bias[q] < 0.f)))
                return fail(WM_E_ARG, "sequence_bias: the bias of sequence %d must be a finite float or -inf", q);
            es.push_back(Ent{id + o[q], (int)len, list, (int)es.size(), list ? -INFINITY : bias[q]});
        }
    }
    out.reset();
    if (es.empty()) return 0;
    std::sort(es.begin(), es.end(), [](const Ent& a, const Ent& b) {
        const int la = a.p[a.len - 1], lb = b.p[b.len - 1];
        if (la != lb) return la < lb;
        if (a.ban != b.ban) return a.ban < b.ban;
        const int ra = !a.ban && a.len == 1 ? 0 : 1, rb = !b.ban && b.len == 1 ? 0 : 1;  // HF sets the length-1 biases before it adds the others
        if (ra != rb) return ra < rb;
        return a.order < b.order;
    });
    std::vector<int32_t> h_ids, h_off{0}, h_ban, h_sid, h_soff;
    std::vector<float> h_bias;
    for (size_t q = 0; q < es.size(); ++q) {
        const Ent& e = es[q];
        if (q == 0 || es[q - 1].p[es[q - 1].len - 1] != e.p[e.len - 1]) {
            h_sid.push_back(e.p[e.len - 1]);
            h_soff.push_back((int32_t)q);
        }
        h_ids.insert(h_ids.end(), e.p, e.p + e.len);
        h_off.push_back((int32_t)h_ids.size());
        h_ban.push_back(e.ban);
        h_bias.push_back(e.bias);
    }
    h_soff.push_back((int32_t)es.size());
    auto t = std::make_shared<SeqTable>();
    (void)hipGetDevice(&t->device);  // (the callers have made the model's device current)
    t->n_seq = (int)es.size();
    t->n_slots = (int)h_sid.size();
    auto up = [](DevBuf& d, const void* src, size_t bytes) -> int {
        WMCHK(d.alloc(bytes));
        HIPCHK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    WMCHK(up(t->ids, h_ids.data(), h_ids.size() * 4));
    WMCHK(up(t->off, h_off.data(), h_off.size() * 4));
    WMCHK(up(t->bias, h_bias.data(), h_bias.size() * 4));
    WMCHK(up(t->ban, h_ban.data(), h_ban.size() * 4));
    WMCHK(up(t->slot_id, h_sid.data(), h_sid.size() * 4));
    WMCHK(up(t->slot_off, h_soff.data(), h_soff.size() * 4));
    std::vector<int32_t> h_of((size_t)vocab, -1);
    for (size_t k = 0; k < h_sid.size(); ++k) h_of[h_sid[k]] = (int32_t)k;
    WMCHK(up(t->slot_of, h_of.data(), h_of.size() * 4));
    if (slot_ids) *slot_ids = h_sid;
    out = std::move(t);
    return 0;
}
extern "C" int wm_set_sequence_bias(wm_model* m, const int32_t* ids, const int32_t* offsets, const float* bias, int n_seq, const int32_t* bad_ids,
                                    const int32_t* bad_offsets, int n_bad) {
    if (!m) return fail(WM_E_ARG, "bad argument");
    HIPCHK(hipSetDevice(m->device));
    std::shared_ptr<SeqTable> t;
    WMCHK(build_seq_table(t, m->cfg.dims.vocab, ids, offsets, bias, n_seq, bad_ids, bad_offsets, n_bad));
    if (t) t->gen = ++m->seq_gen;
    m->repeat.sb = std::move(t);  // a held submit and a pending pass keep the table they were asked for with
    return 0;
}
// ---- token-level timestamps ------------------------------------------------------------------------------------
extern "C" int wm_set_alignment_heads(wm_model* m, const int32_t* layer_head_pairs, int n_pairs) {
    if (!m || n_pairs < 0 || (n_pairs > 0 && !layer_head_pairs)) return fail(WM_E_ARG, "bad argument");
    if (n_pairs > ALIGN_MAX_HEADS) return fail(WM_E_ARG, "at most %d alignment heads (got %d)", ALIGN_MAX_HEADS, n_pairs);
    const wm_dims& c = m->cfg.dims;
    std::vector<int32_t> pairs(layer_head_pairs, layer_head_pairs + 2 * n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        const int l = pairs[2 * k], h = pairs[2 * k + 1];
        if (l < 0 || l >= c.n_layers || h < 0 || h >= c.n_heads || h >= 32)
            return fail(WM_E_ARG, "alignment head %d = (%d, %d) outside %d layers x %d heads", k, l, h, c.n_layers, c.n_heads);
        for (int q = 0; q < k; ++q)
            if (pairs[2 * q] == l && pairs[2 * q + 1] == h) return fail(WM_E_ARG, "alignment head (%d, %d) listed twice", l, h);
    }
    m->align_pairs = pairs;
    return 0;
}

// The buffers of a timestamp or align pass (they only grow) for al.pairs: Lr >= 1 rows per utterance, times_stride time columns
static int align_buffers(wm_model* m, wm_state* s, size_t Lr, size_t times_stride) {
    wm_state::Align& a = s->al;
    const size_t B = s->B, T = m->cfg.dims.n_audio_ctx, n_sel = a.pairs.size() / 2;
    WMCHK(grow(a.cap, B * Lr * n_sel * 64 * 4));
    if (m->xattn) WMCHK(grow(a.kh, B * n_sel * T * 64 * 4));
    WMCHK(grow(a.probs, B * n_sel * Lr * T * 4));
    WMCHK(grow(a.mean, B * n_sel * T * 4));
    WMCHK(grow(a.stdv, B * n_sel * T * 4));
    WMCHK(grow(a.M, B * Lr * T * 4));
    // rows past ~400 at n_audio_ctx = 1500: the 2-bit trace leaves LDS for global memory
    if (align_dtw_lds_bytes((int)Lr, (int)T) == 0) WMCHK(grow(a.trace, B * Lr * ((T + 15) / 16) * 4));
    WMCHK(grow(a.times, B * times_stride * 4));
    WMCHK(grow(a.ncols, B * 4));
    return 0;
}
// Before the pass's graphs are (re)captured: size the timestamp buffers of state s and record what the pass asked for.
static int align_setup(wm_model* m, wm_state* s, const wm_decode_opts* o, const std::vector<int32_t>* cols, const WinAsk* win) {
    wm_state::Align& a = s->al;
    a.on = cols != nullptr;
    a.win = a.on && win != nullptr;
    if (!a.on) return 0;
    if (a.win) {  // the tables the window kernel fills, and what it hands back
        a.items = win->items;
        a.n_real = win->n_real;
        WMCHK(grow(a.rows, (size_t)s->B * 4));
        WMCHK(grow(a.row0, (size_t)s->B * 4));
        WMCHK(grow(a.wtimes, (size_t)s->B * (o->max_loop + 1) * 8));
    }
    a.pairs = m->align_pairs;
    a.L = o->max_loop;
    a.n_prompt = o->n_prompt;
    a.cols = *cols;
    ++a.gen;
    WMCHK(align_buffers(m, s, std::max<size_t>(o->max_loop, 1), s->out_stride));
    // (a.cols outlives the copy: the state is not reused before this pass is waited for)
    HIPCHK(hipMemcpyAsync(a.ncols.p, a.cols.data(), (size_t)s->B * 4, hipMemcpyHostToDevice, s->lanes[0].st));
    return 0;
}

static AlignParams align_params(wm_model* m, wm_state* s) {
    const wm_dims& c = m->cfg.dims;
    const wm_state::Align& a = s->al;
    AlignParams p{};
    p.cap = a.cap.as<float>();
    p.B = s->B;
    p.L = a.L;
    p.n_sel = (int)a.pairs.size() / 2;
    p.n_prompt = a.n_prompt;
    p.T = c.n_audio_ctx;
    p.d = c.d_model;
    p.n_tokens = s->n_tokens.as<int>();
    p.n_frames = a.ncols.as<int>();
    if (m->xattn) {
        p.X = s->enc_x.p;
        p.Wk = m->cross_kv_w.p;
        p.kh = a.kh.as<float>();
    } else {
        p.kv = s->cross_kv.p;
        p.kv_dtype = m->cfg.kv_dtype;
        p.kv_layer_stride = (long)((size_t)s->B * c.n_audio_ctx * c.d_model);
    }
    for (int k = 0; k < p.n_sel; ++k) {
        p.layer[k] = a.pairs[2 * k];
        p.head[k] = a.pairs[2 * k + 1];
    }
    p.probs = a.probs.as<float>();
    p.mean = a.mean.as<float>();
    p.stdv = a.stdv.as<float>();
    p.M = a.M.as<float>();
    p.trace = align_dtw_lds_bytes(a.L, c.n_audio_ctx) ? nullptr : a.trace.as<unsigned>();
    p.times = a.times.as<float>();
    p.out_stride = s->out_stride;
    if (a.ragged) {  // an align pass: per-row row counts and offsets, the caller's table width
        p.n_tokens = nullptr;
        p.n_prompt = 0;
        p.rows = a.rows.as<int>();
        p.row0 = a.row0.as<int>();
        p.out_stride = a.stride;
        for (int b = 0; b < s->B; ++b) p.out_need = std::max(p.out_need, a.h_row0[b] + a.h_rows[b] + 1);
    } else if (a.win) {  // a window pass: the same form, the tables made on the device (row0[b] <= n_prompt, rows[b] <= L)
        p.n_tokens = nullptr;
        p.rows = a.rows.as<int>();
        p.row0 = a.row0.as<int>();
        p.out_need = a.n_prompt + a.L + 1;
    }
    return p;
}
static AlignWindowParams align_window_params(wm_state* s, int mode) {
    const wm_state::Align& a = s->al;
    AlignWindowParams w{};
    w.mode = mode;
    w.B = s->B;
    w.n_real = a.n_real;
    w.L = a.L;
    w.n_prompt = a.n_prompt;
    w.out_stride = s->out_stride;
    w.n_tokens = s->n_tokens.as<int>();
    w.prompt_len = s->rw.on ? s->rw.len.as<int>() : nullptr;
    w.items = a.items;
    w.rows = a.rows.as<int>();
    w.row0 = a.row0.as<int>();
    w.times = a.times.as<float>();
    w.out = (double*)a.wtimes.p;
    return w;
}

// the post-loop kernels of a timestamp pass, on lane 0's stream behind the last step
static int enqueue_align(wm_model* m, wm_state* s) {
    hipStream_t st = s->lanes[0].st;
    if (s->al.L == 0) {  // max_loop 0: no row ever, every time is 0 (HF's early return)
        HIPCHK(hipMemsetAsync(s->al.times.p, 0, (size_t)s->B * (s->al.ragged ? s->al.stride : s->out_stride) * 4, st));
        if (s->al.win) LCHK(launch_align_window(align_window_params(s, 1), st));  // the one id of each window, at its offset
        return 0;
    }
    const AlignParams p = align_params(m, s);
    if (s->al.win) LCHK(launch_align_window(align_window_params(s, 0), st));  // rows / row0 from the loop's counts
    LCHK(launch_align_probs(p, st));
    LCHK(launch_align_norm(p, st));
    LCHK(launch_align_dtw(p, st));
    if (s->al.win) LCHK(launch_align_window(align_window_params(s, 1), st));  // the window's result rows
    return 0;
}

extern "C" int wm_alignment_weights(wm_model* m, int slot, float* out) {
    if (!m || !out || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    const wm_model::AlignRef& r = m->align_ref[slot];
    if (!r.st || !state_is_live(r.st) || r.st->al.gen != r.gen || r.st->pending)
        return fail(WM_E_STATE, "no completed timestamp pass on this slot (or its state has run another pass since)");
    wm_state* s = r.st;
    const size_t T = m->cfg.dims.n_audio_ctx, L = s->al.L, n_sel = s->al.pairs.size() / 2;
    HIPCHK(hipSetDevice(m->device));
    const size_t per_row = n_sel * L * T;
    HIPCHK(hipMemcpy(out, s->al.probs.as<float>() + (size_t)r.row0 * per_row, (size_t)r.rows * per_row * 4, hipMemcpyDeviceToHost));
    std::vector<int32_t> n(r.rows);
    HIPCHK(hipMemcpy(n.data(), s->n_tokens.as<int>() + r.row0, (size_t)r.rows * 4, hipMemcpyDeviceToHost));
    for (int b = 0; b < r.rows; ++b) {  // rows past R_b were never computed
        const size_t R = s->al.ragged ? (size_t)s->al.h_rows[r.row0 + b] : (size_t)std::max(0, std::min<int>((int)L, n[b] - s->al.n_prompt - 1));
        for (size_t k = 0; k < n_sel; ++k) std::fill(out + b * per_row + (k * L + R) * T, out + b * per_row + (k + 1) * L * T, 0.f);
    }
    return 0;
}

extern "C" int wm_op_token_times(float* times, const float* weights, int n_sel, int R, int F, int n_prompt) {
    if (!times || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || R < 0 || R > ALIGN_MAX_ROWS || F <= 0 || n_prompt < 0 || (R > 0 && !weights))
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 0 <= R <= %d, F >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    const int total = n_prompt + R + 1;
    if (R == 0) {
        std::fill(times, times + total, 0.f);
        return 0;
    }
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &M = t.add(), &tr = t.add(), &tm = t.add(), &nt = t.add();
    WMCHK(upload(probs, weights, (size_t)n_sel * R * F, WM_F32));
    WMCHK(mean.alloc((size_t)n_sel * F * 4));
    WMCHK(sd.alloc((size_t)n_sel * F * 4));
    WMCHK(M.alloc((size_t)R * F * 4));
    WMCHK(tm.alloc((size_t)total * 4));
    WMCHK(upload_bytes(nt, &total, 4));
    AlignParams p{};
    p.B = 1;
    p.L = R;
    p.n_sel = n_sel;
    p.n_prompt = n_prompt;
    p.T = F;
    p.n_tokens = nt.as<int>();
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = M.as<float>();
    if (align_dtw_lds_bytes(R, F) == 0) {
        WMCHK(tr.alloc((size_t)R * ((F + 15) / 16) * 4));
        p.trace = tr.as<unsigned>();
    }
    p.times = tm.as<float>();
    p.out_stride = total;
    LCHK(launch_align_norm(p, nullptr));
    LCHK(launch_align_dtw(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(times, tm.p, (size_t)total * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Several weight tables through align_norm and align_dtw in ONE launch each, with per-table row counts and offsets (the ragged chain of
// an align pass): weights [n_tab][n_sel][L][T] with L >= max R and T >= max F, table b's R[b] x F[b] corner used;
// times [n_tab][out_stride], out_stride >= max(row0[b] + R[b] + 1).
extern "C" int wm_op_token_times_rows(float* times, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F,
                                      const int32_t* row0, int out_stride) {
    if (!times || !weights || !R || !F || !row0 || n_tab <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0)
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 1 <= L <= %d, T >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    int need = 0;
    for (int b = 0; b < n_tab; ++b) {
        if (R[b] < 0 || R[b] > L || F[b] < 1 || F[b] > T || row0[b] < 0) return fail(WM_E_ARG, "table %d: R in [0, L], F in [1, T], row0 >= 0", b);
        need = std::max(need, row0[b] + R[b] + 1);
    }
    if (out_stride < need) return fail(WM_E_ARG, "out_stride %d is smaller than max(row0 + R + 1) = %d", out_stride, need);
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &M = t.add(), &tr = t.add(), &tm = t.add(), &dr = t.add(), &df = t.add(), &d0 = t.add();
    WMCHK(upload(probs, weights, (size_t)n_tab * n_sel * L * T, WM_F32));
    WMCHK(mean.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(sd.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(M.alloc((size_t)n_tab * L * T * 4));
    WMCHK(tm.alloc((size_t)n_tab * out_stride * 4));
    for (auto pr : {std::make_pair(&dr, R), std::make_pair(&df, F), std::make_pair(&d0, row0)}) WMCHK(upload_bytes(*pr.first, pr.second, (size_t)n_tab * 4));
    AlignParams p{};
    p.B = n_tab;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.n_frames = df.as<int>();
    p.rows = dr.as<int>();
    p.row0 = d0.as<int>();
    p.out_need = need;
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = M.as<float>();
    if (align_dtw_lds_bytes(L, T) == 0) {
        WMCHK(tr.alloc((size_t)n_tab * L * ((T + 15) / 16) * 4));
        p.trace = tr.as<unsigned>();
    }
    p.times = tm.as<float>();
    p.out_stride = out_stride;
    LCHK(launch_align_norm(p, nullptr));
    LCHK(launch_align_dtw(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(times, tm.p, (size_t)n_tab * out_stride * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_align_probs alone.  Keys: kv (host fp32 [n_layers][2][B][T][d], the model's K/V cache with its V halves, uploaded as
// kv_dtype) or the absorbed form X [B][T][d] + Wk [n_layers][2][d][d] (both uploaded as bf16, K_h built in a scratch buffer).
// probs [B][n_sel][L][T] goes up before the launch and comes back after it: rows >= rows[b] keep what the caller put there.
extern "C" int wm_op_align_probs(float* probs, const float* q, const float* kv, int kv_dtype, const float* X, const float* Wk,
                                 const int32_t* layer_head_pairs, int n_sel, const int32_t* rows, int B, int L, int T, int d, int n_layers) {
    if (!probs || !q || !layer_head_pairs || !rows) return fail(WM_E_ARG, "probs, q, layer_head_pairs and rows are required");
    if (kv ? (X || Wk) : (!X || !Wk)) return fail(WM_E_ARG, "keys: either kv, or X and Wk");
    if (kv && kv_dtype != WM_F32 && kv_dtype != WM_BF16 && kv_dtype != WM_F16) return fail(WM_E_ARG, "kv_dtype %d", kv_dtype);
    if (B <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0 || d <= 0 || d % 64 || n_layers <= 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, 1 <= n_sel <= %d, 1 <= L <= %d, T >= 1, d a multiple of 64, n_layers >= 1)", ALIGN_MAX_HEADS,
                    ALIGN_MAX_ROWS);
    for (int b = 0; b < B; ++b)
        if (rows[b] < 0 || rows[b] > L) return fail(WM_E_ARG, "utterance %d: rows in [0, L]", b);
    for (int k = 0; k < n_sel; ++k)
        if (layer_head_pairs[2 * k] < 0 || layer_head_pairs[2 * k] >= n_layers || layer_head_pairs[2 * k + 1] < 0 || layer_head_pairs[2 * k + 1] >= d / 64)
            return fail(WM_E_ARG, "pair %d: layer in [0, %d), head in [0, %d)", k, n_layers, d / 64);
    TmpDev t;
    DevBuf &cap = t.add(), &keys = t.add(), &wk = t.add(), &kh = t.add(), &pr = t.add(), &dr = t.add();
    WMCHK(upload(cap, q, (size_t)B * L * n_sel * 64, WM_F32));
    WMCHK(upload(pr, probs, (size_t)B * n_sel * L * T, WM_F32));
    WMCHK(upload_bytes(dr, rows, (size_t)B * 4));
    AlignParams p{};
    p.cap = cap.as<float>();
    p.B = B;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.d = d;
    p.rows = dr.as<int>();
    if (kv) {
        WMCHK(upload(keys, kv, (size_t)n_layers * 2 * B * T * d, kv_dtype));
        p.kv = keys.p;
        p.kv_dtype = kv_dtype;
        p.kv_layer_stride = (long)((size_t)B * T * d);
    } else {
        WMCHK(upload(keys, X, (size_t)B * T * d, WM_BF16));
        WMCHK(upload(wk, Wk, (size_t)n_layers * 2 * d * d, WM_BF16));
        WMCHK(kh.alloc((size_t)B * n_sel * T * 64 * 4));
        p.X = keys.p;
        p.Wk = wk.p;
        p.kh = kh.as<float>();
    }
    for (int k = 0; k < n_sel; ++k) {
        p.layer[k] = layer_head_pairs[2 * k];
        p.head[k] = layer_head_pairs[2 * k + 1];
    }
    p.probs = pr.as<float>();
    LCHK(launch_align_probs(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(probs, pr.p, (size_t)B * n_sel * L * T * 4, hipMemcpyDeviceToHost));
    return 0;
}

// launch_align_norm alone: wm_op_token_times_rows' tables -> M [n_tab][L][T], uploaded first (cells outside a table's R x F corner keep
// what the caller put there).
extern "C" int wm_op_align_norm(float* M, const float* weights, int n_tab, int n_sel, int L, int T, const int32_t* R, const int32_t* F) {
    if (!M || !weights || !R || !F || n_tab <= 0 || n_sel <= 0 || n_sel > ALIGN_MAX_HEADS || L <= 0 || L > ALIGN_MAX_ROWS || T <= 0)
        return fail(WM_E_ARG, "bad argument (1 <= n_sel <= %d, 1 <= L <= %d, T >= 1)", ALIGN_MAX_HEADS, ALIGN_MAX_ROWS);
    for (int b = 0; b < n_tab; ++b)
        if (R[b] < 0 || R[b] > L || F[b] < 1 || F[b] > T) return fail(WM_E_ARG, "table %d: R in [0, L], F in [1, T]", b);
    TmpDev t;
    DevBuf &probs = t.add(), &mean = t.add(), &sd = t.add(), &dm = t.add(), &dr = t.add(), &df = t.add();
    WMCHK(upload(probs, weights, (size_t)n_tab * n_sel * L * T, WM_F32));
    WMCHK(upload(dm, M, (size_t)n_tab * L * T, WM_F32));
    WMCHK(mean.alloc((size_t)n_tab * n_sel * T * 4));
    WMCHK(sd.alloc((size_t)n_tab * n_sel * T * 4));
    for (auto pr : {std::make_pair(&dr, R), std::make_pair(&df, F)}) WMCHK(upload_bytes(*pr.first, pr.second, (size_t)n_tab * 4));
    AlignParams p{};
    p.B = n_tab;
    p.L = L;
    p.n_sel = n_sel;
    p.T = T;
    p.n_frames = df.as<int>();
    p.rows = dr.as<int>();
    p.probs = probs.as<float>();
    p.mean = mean.as<float>();
    p.stdv = sd.as<float>();
    p.M = dm.as<float>();
    LCHK(launch_align_norm(p, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(M, dm.p, (size_t)n_tab * L * T * 4, hipMemcpyDeviceToHost));
    return 0;
}

// wm_transcribe_wait with the result left ON THE DEVICE as the gather buffer of the multi-GPU path: dev_packed
// [rows_cap, 1 + stride] int32 in the caller's device memory (e.g. a torch tensor), row r = [length, ids zero-padded]; rows past the
// batch are zeroed.  stride >= n_prompt + 1 + max_loop of the pass.
extern "C" int wm_transcribe_wait_device(wm_model* m, int slot, int32_t* dev_packed, int rows_cap, int stride) {
    if (!m || !dev_packed || slot < 0 || slot >= wm_model::NSLOT || stride <= 0) return fail(WM_E_ARG, "bad argument");
    PassOut out;
    out.dev_packed = dev_packed;
    out.rows_cap = rows_cap;
    out.pack_stride = stride;
    return collect_slot(m, slot, PassKind::transcribe, out);
}
extern "C" int wm_transcribe_steps(wm_model* m, int slot) {
    if (!m || slot < 0 || slot >= wm_model::NSLOT) return -1;
    return m->last_steps[slot];
}

// ---- log-mel front end: 16 kHz PCM -> [n_mels, n_frames]  (export_weights.py:100-116 delegates this to
// HF WhisperProcessor = transformers feature_extraction_whisper._np_extract_fbank_features)
static const int FE_NFFT = 400, FE_HOP = 160, FE_NFREQ = 201;

static double hz_to_mel_slaney(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; }
static double mel_to_hz_slaney(double m) { return m >= 15.0 ? 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0)) : 200.0 * m / 3.0; }

// The front end's four tables for n_mels filters, built once on the host in float64 and rounded once: the periodic Hann window [400],
// the real-DFT basis [512][416] (cos at row k, -sin at row 256 + k, k < 201; every other entry 0), the slaney filter bank
// [201][n_mels] and, per filter, the interval [lo, hi) of bins outside which it is 0 (band [n_mels][2]; an empty filter gives 0, 0).
static const double FE_PI = 3.14159265358979323846;
static void frontend_window(std::vector<float>& window) {
    window.assign(FE_NFFT, 0.f);
    for (int n = 0; n < FE_NFFT; ++n) window[n] = (float)(0.5 - 0.5 * std::cos(2.0 * FE_PI * n / FE_NFFT));  // periodic Hann
}
static void frontend_tables(int n_mels, std::vector<float>& window, std::vector<float>& dft, std::vector<float>& fb, std::vector<int>& band) {
    const double PI = FE_PI;
    frontend_window(window);
    dft.assign((size_t)512 * 416, 0.f);
    fb.assign((size_t)FE_NFREQ * n_mels, 0.f);
    for (int k = 0; k < FE_NFREQ; ++k)
        for (int n = 0; n < FE_NFFT; ++n) {
            const double ang = 2.0 * PI * (double)((k * n) % FE_NFFT) / FE_NFFT;
            dft[(size_t)k * 416 + n] = (float)std::cos(ang);
            dft[(size_t)(256 + k) * 416 + n] = (float)(-std::sin(ang));
        }
    // slaney-scale, slaney-normalised triangular filters (transformers.audio_utils.mel_filter_bank)
    std::vector<double> ff(n_mels + 2);
    const double m0 = hz_to_mel_slaney(0.0), m1 = hz_to_mel_slaney(8000.0);
    for (int i = 0; i < n_mels + 2; ++i) ff[i] = mel_to_hz_slaney(m0 + (m1 - m0) * i / (n_mels + 1));
    band.assign(2 * (size_t)n_mels, 0);
    for (int mm = 0; mm < n_mels; ++mm) {
        int lo = FE_NFREQ, hi = 0;
        const double enorm = 2.0 / (ff[mm + 2] - ff[mm]);
        for (int k = 0; k < FE_NFREQ; ++k) {
            const double f = 8000.0 * k / (FE_NFREQ - 1);
            const double down = (f - ff[mm]) / (ff[mm + 1] - ff[mm]), up = (ff[mm + 2] - f) / (ff[mm + 2] - ff[mm + 1]);
            const double v = std::max(0.0, std::min(down, up)) * enorm;
            fb[(size_t)k * n_mels + mm] = (float)v;
            if (v > 0.0) {
                lo = std::min(lo, k);
                hi = std::max(hi, k + 1);
            }
        }
        band[2 * mm] = lo < hi ? lo : 0;
        band[2 * mm + 1] = lo < hi ? hi : 0;
    }
}

static int frontend_init(wm_model* m) {
    if (m->fe.ready) return 0;
    const wm_dims& c = m->cfg.dims;
    const int n_mels = c.n_mels, n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames, maxB = m->cfg.max_batch;
    std::vector<float> window, dft, fb;
    std::vector<int> band;
    frontend_tables(n_mels, window, dft, fb, band);
    WMCHK(upload(m->fe.window, window.data(), window.size(), WM_F32));
    WMCHK(upload(m->fe.dft, dft.data(), dft.size(), WM_F32));
    WMCHK(upload(m->fe.fb, fb.data(), fb.size(), WM_F32));
    WMCHK(m->fe.band.alloc(band.size() * 4));
    HIPCHK(hipMemcpy(m->fe.band.p, band.data(), band.size() * 4, hipMemcpyHostToDevice));
    const size_t ch = std::min(maxB, m->fe.chunk);
    const size_t rows = (ch * n_frames + 255) / 256 * 256 + 256;
    WMCHK(m->fe.pcm.alloc((size_t)maxB * N * 4, true));
    WMCHK(m->fe.lens.alloc((size_t)maxB * 4, true));
    WMCHK(m->fe.frames.alloc(rows * 416 * 4, true));
    WMCHK(m->fe.spec.alloc(rows * 512 * 4, true));
    WMCHK(m->fe.logtmp.alloc((size_t)maxB * n_mels * n_frames * 4));
    WMCHK(m->fe.mel.alloc((size_t)maxB * n_mels * n_frames * 4));
    m->fe.ready = true;
    return 0;
}

static int frontend_compute(wm_model* m, int B, float* mel_out);
// pcm: host [B][stride] fp32 at 16 kHz; n_samples[b] valid samples (<= stride).  Result stays in m->fe.mel (device).
static int frontend_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride) {
    if (!pcm || !n_samples || B <= 0 || stride <= 0) return fail(WM_E_ARG, "bad argument");
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    hipStream_t st = m->stream;
    // pad / trim to the 30 s window: ONE strided upload of the common prefix, then a kernel zeroes each utterance's tail
    for (int b = 0; b < B; ++b)
        if (n_samples[b] < 0 || n_samples[b] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    const size_t w = std::min(stride, N);
    if (w < (size_t)N) HIPCHK(hipMemsetAsync(m->fe.pcm.p, 0, (size_t)B * N * 4, st));
    HIPCHK(hipMemcpy2DAsync(m->fe.pcm.p, (size_t)N * 4, pcm, (size_t)stride * 4, w * 4, B, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(m->fe.lens.p, n_samples, (size_t)B * 4, hipMemcpyHostToDevice, st));
    launch_zero_tails(m->fe.pcm.as<float>(), m->fe.lens.as<int>(), B, N, st);
    return frontend_compute(m, B, m->fe.mel.as<float>());
}
// m->fe.pcm [B][N] (padded / trimmed to the window, on the device) -> mel_out [B][n_mels][n_frames] (device), on the model's stream
static int frontend_compute(wm_model* m, int B, float* mel_out) {
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    hipStream_t st = m->stream;
    for (int c0 = 0; c0 < B; c0 += m->fe.chunk) {
        const int bc = std::min(m->fe.chunk, B - c0);
        launch_frames(m->fe.pcm.as<float>() + (size_t)c0 * N, m->fe.frames.as<float>(), m->fe.window.as<float>(), bc, N, n_frames, FE_HOP, st);
        GemmParams p{};
        p.A = m->fe.frames.p;
        p.W = m->fe.dft.p;
        p.C = m->fe.spec.p;
        p.M = bc * n_frames;
        p.N = 512;
        p.K = 416;
        p.lda = 416;
        p.ldw = 416;
        p.ldc = 512;
        LCHK((launch_gemm_nt<float, float>(p, 1, st)));
        launch_mel_log(m->fe.spec.as<float>(), m->fe.fb.as<float>(), m->fe.band.as<int>(), m->fe.logtmp.as<float>() + (size_t)c0 * c.n_mels * n_frames,
                       bc, n_frames, c.n_mels, st);
    }
    launch_mel_norm(m->fe.logtmp.as<float>(), mel_out, B, c.n_mels * n_frames, st);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int wm_log_mel(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));
    const wm_dims& c = m->cfg.dims;
    if (mel_out) HIPCHK(hipMemcpyAsync(mel_out, m->fe.mel.p, (size_t)B * c.n_mels * 2 * c.n_audio_ctx * 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    return 0;
}

// ---- the front end's stages one at a time (known-answer tests; include/whisper_mi.h) -- each through the launcher the runtime uses
static const int FE_MAX_MELS = 128, FE_MAX_GRID_Y = 65535;
extern "C" int wm_op_fe_tables(int n_mels, float* window, float* dft, float* fb, int32_t* band) {
    if (!window || !dft || !fb || !band || n_mels < 1 || n_mels > FE_MAX_MELS) return fail(WM_E_ARG, "bad argument (1 <= n_mels <= %d)", FE_MAX_MELS);
    std::vector<float> w, d, f;
    std::vector<int> bd;
    frontend_tables(n_mels, w, d, f, bd);
    memcpy(window, w.data(), w.size() * 4);
    memcpy(dft, d.data(), d.size() * 4);
    memcpy(fb, f.data(), f.size() * 4);
    memcpy(band, bd.data(), bd.size() * 4);
    return 0;
}
extern "C" int wm_op_fe_frames(float* out, const float* pcm, const int32_t* n_samples, int B, int N, int n, int t0) {
    if (!out || !pcm || B <= 0 || B > FE_MAX_GRID_Y || N <= 200 || n <= 0 || t0 < 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, N > 200, n >= 1, t0 >= 0)");
    if ((int64_t)t0 + n > N / FE_HOP)
        return fail(WM_E_ARG, "frames [%d, %lld) leave the %d frames of %d samples", t0, (long long)t0 + n, N / FE_HOP, N);
    if (n_samples)
        for (int b = 0; b < B; ++b)
            if (n_samples[b] < 0 || n_samples[b] > N) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    std::vector<float> window;
    frontend_window(window);
    TmpDev tmp;
    DevBuf &dp = tmp.add(), &dl = tmp.add(), &dw = tmp.add(), &dout = tmp.add();
    const size_t n_out = ((size_t)B * n + 1) * 416;  // one guard row behind the last frame
    WMCHK(upload(dp, pcm, (size_t)B * N, WM_F32));
    WMCHK(upload(dw, window.data(), window.size(), WM_F32));
    WMCHK(upload(dout, out, n_out, WM_F32));  // in and out: what the kernel does not store keeps the caller's value
    if (n_samples) {
        WMCHK(upload_bytes(dl, n_samples, (size_t)B * 4));
        launch_zero_tails(dp.as<float>(), dl.as<int>(), B, N, nullptr);
    }
    launch_frames(dp.as<float>(), dout.as<float>(), dw.as<float>(), B, N, n, FE_HOP, nullptr, t0);
    HIPCHK(hipGetLastError());
    return download_f32(out, dout, n_out, WM_F32);
}
extern "C" int wm_op_fe_mel_log(float* logmel, const float* spec, int B, int n, int n_mels, int out_frames, int t_out) {
    if (!logmel || !spec || B <= 0 || B > FE_MAX_GRID_Y || n <= 0 || n_mels < 1 || n_mels > FE_MAX_MELS || t_out < 0)
        return fail(WM_E_ARG, "bad argument (B >= 1, n >= 1, 1 <= n_mels <= %d, t_out >= 0)", FE_MAX_MELS);
    if (out_frames <= 0 || (int64_t)t_out + n > out_frames)
        return fail(WM_E_ARG, "frames [%d, %lld) leave the row of %d", t_out, (long long)t_out + n, out_frames);
    std::vector<float> window, dft, fb;
    std::vector<int> band;
    frontend_tables(n_mels, window, dft, fb, band);
    TmpDev tmp;
    DevBuf &ds = tmp.add(), &df = tmp.add(), &db = tmp.add(), &dout = tmp.add();
    const size_t n_out = (size_t)B * n_mels * out_frames;
    WMCHK(upload(ds, spec, (size_t)B * n * 512, WM_F32));
    WMCHK(upload(df, fb.data(), fb.size(), WM_F32));
    WMCHK(upload_bytes(db, band.data(), band.size() * 4));
    WMCHK(upload(dout, logmel, n_out, WM_F32));  // in and out
    launch_mel_log(ds.as<float>(), df.as<float>(), db.as<int>(), dout.as<float>(), B, n, n_mels, nullptr, out_frames, t_out);
    HIPCHK(hipGetLastError());
    return download_f32(logmel, dout, n_out, WM_F32);
}
extern "C" int wm_op_fe_mel_norm(float* out, const float* logmel, int B, int64_t n, int long_mode) {
    if (!out || !logmel || B <= 0 || B > FE_MAX_GRID_Y || n <= 0 || (long_mode != 0 && long_mode != 1)) return fail(WM_E_ARG, "bad argument");
    if (n > INT32_MAX) return fail(WM_E_ARG, "n = %lld exceeds 2^31 - 1", (long long)n);
    TmpDev tmp;
    DevBuf &dx = tmp.add(), &dy = tmp.add(), &dpart = tmp.add();
    WMCHK(upload(dx, logmel, (size_t)B * n, WM_F32));
    if (long_mode) {
        WMCHK(dpart.alloc((size_t)B * 256 * 4));
        launch_mel_norm_long(dx.as<float>(), dpart.as<float>(), B, (size_t)n, nullptr);  // in place
    } else {
        WMCHK(dy.alloc((size_t)B * n * 4));
        launch_mel_norm(dx.as<float>(), dy.as<float>(), B, (int)n, nullptr);
    }
    HIPCHK(hipGetLastError());
    return download_f32(out, long_mode ? dx : dy, (size_t)B * n, WM_F32);
}
extern "C" int wm_op_window_gather(float* out, const float* mel, const int32_t* items, int rows, int B, int n_mels, int F, int W) {
    if (!out || !mel || !items || rows <= 0 || rows > FE_MAX_GRID_Y || B <= 0 || n_mels < 1 || n_mels > FE_MAX_MELS || F <= 0 || W <= 0)
        return fail(WM_E_ARG, "bad argument");
    for (int r = 0; r < rows; ++r) {
        const int32_t* t = items + 3 * (size_t)r;
        if (t[0] < 0 || t[0] >= B || t[1] < 0 || t[2] < 0 || t[2] > W || (int64_t)t[1] + t[2] > F)
            return fail(WM_E_ARG, "item %d = (%d, %d, %d) leaves mel [%d][%d][%d] or the window of %d frames", r, t[0], t[1], t[2], B, n_mels, F, W);
    }
    TmpDev tmp;
    DevBuf &dm = tmp.add(), &di = tmp.add(), &dout = tmp.add();
    const size_t n_out = (size_t)rows * n_mels * W;
    WMCHK(upload(dm, mel, (size_t)B * n_mels * F, WM_F32));
    WMCHK(upload_bytes(di, items, (size_t)rows * 3 * 4));
    WMCHK(upload(dout, out, n_out, WM_F32));  // in and out
    launch_window_gather(dm.as<float>(), di.as<int>(), dout.as<float>(), rows, n_mels, F, W, nullptr);
    HIPCHK(hipGetLastError());
    return download_f32(out, dout, n_out, WM_F32);
}

extern "C" int wm_transcribe_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                 int32_t* tokens_out, int32_t* n_tokens) {
    if (!m || !tokens_out || !n_tokens) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream as the encoder: ordered, no host sync
    return run_now(m, PassAsk{m->fe.mel.as<float>(), 1, B, o}, PassOut{tokens_out, n_tokens});
}

// n_frames[b] = min(2·n_audio_ctx, ceil(n_samples[b] / 160)): the attention mask of WhisperFeatureExtractor
extern "C" int wm_transcribe_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                    int32_t* tokens_out, int32_t* n_tokens, float* token_times) {
    if (!m || !tokens_out || !n_tokens || !token_times || !n_samples || B <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_opts(m, o, B));
    std::vector<int32_t> nf(B);
    for (int b = 0; b < B; ++b) nf[b] = (int32_t)std::min<long>(2L * m->cfg.dims.n_audio_ctx, ((long)n_samples[b] + FE_HOP - 1) / FE_HOP);
    std::vector<int32_t> cols;
    WMCHK(align_cols(m, nf.data(), B, cols));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));
    PassAsk ask{m->fe.mel.as<float>(), 1, B, o};
    ask.cols = &cols;
    return run_now(m, ask, PassOut{tokens_out, n_tokens, token_times});
}

// ---- any sample rate and int16 in: resampling to 16 kHz on the GPU --------------------------------------------------
// torchaudio.functional.resample(x, sr_in, 16000) with its defaults (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99): the
// taps are computed in float64 and rounded once; sr_in = 16000 is the identity (one tap of 1, as torchaudio returns its input).
static const int RS_RATE = 16000, RS_MAX_RATIO = 1024;
static int resample_ratio(int sr_in, int* orig, int* nw, int* width) {
    if (sr_in <= 0) return fail(WM_E_ARG, "sr_in = %d must be positive", sr_in);
    int a = sr_in, b = RS_RATE;
    while (b) {
        const int t = a % b;
        a = b, b = t;
    }
    const int64_t o = sr_in / a, n = RS_RATE / a;
    if (o > RS_MAX_RATIO || n > RS_MAX_RATIO)
        return fail(WM_E_ARG, "sr_in = %d: the reduced ratio %lld / %lld has a term above %d", sr_in, (long long)o, (long long)n, RS_MAX_RATIO);
    *orig = (int)o, *nw = (int)n;
    const double base = (double)std::min(o, n) * 0.99;
    *width = sr_in == RS_RATE ? 0 : (int)std::ceil(6.0 * (double)o / base);
    return 0;
}
// h [nw][2 * width + orig]
static void resample_taps_host(int orig, int nw, int width, std::vector<float>& h) {
    const int K = 2 * width + orig;
    h.assign((size_t)nw * K, 0.f);
    if (width == 0) {
        h[0] = 1.f;
        return;
    }
    const double PI = 3.14159265358979323846, base = (double)std::min(orig, nw) * 0.99, scale = base / (double)orig;
    for (int p = 0; p < nw; ++p)
        for (int k = 0; k < K; ++k) {
            double t = (-(double)p / (double)nw + (double)(k - width) / (double)orig) * base;
            t = std::min(6.0, std::max(-6.0, t));
            const double pt = PI * t, s = t == 0.0 ? 1.0 : std::sin(pt) / pt, c = std::cos(pt / 12.0);
            h[(size_t)p * K + k] = (float)(s * (c * c) * scale);
        }
}
static int resample_len(int64_t n_in, int orig, int nw, int64_t* n_out) {
    if (n_in < 0) return fail(WM_E_ARG, "n_in = %lld is negative", (long long)n_in);
    if (n_in > INT64_MAX / RS_MAX_RATIO - RS_MAX_RATIO) return fail(WM_E_SIZE, "n_in = %lld: the output length leaves 64 bits", (long long)n_in);
    *n_out = (n_in * nw + orig - 1) / orig;
    return 0;
}
extern "C" int wm_resample_len(int64_t n_in, int sr_in, int64_t* n_out) {
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int orig, nw, width;
    WMCHK(resample_ratio(sr_in, &orig, &nw, &width));
    return resample_len(n_in, orig, nw, n_out);
}
extern "C" int wm_op_resample_taps(int sr_in, float* taps, int64_t cap, int* orig, int* nw, int* width) {
    if (!orig || !nw || !width || cap < 0 || (cap > 0 && !taps)) return fail(WM_E_ARG, "bad argument");
    WMCHK(resample_ratio(sr_in, orig, nw, width));
    if (!taps) return 0;
    const int64_t need = (int64_t)*nw * (2 * *width + *orig);
    if (cap < need) return fail(WM_E_SIZE, "cap = %lld is smaller than the table of %lld taps", (long long)cap, (long long)need);
    std::vector<float> h;
    resample_taps_host(*orig, *nw, *width, h);
    memcpy(taps, h.data(), h.size() * 4);
    return 0;
}
// the table of one sr_in on the device, in the layout resample_kernel reads (wm_kernels.h ResampleParams)
static int resampler_build(wm_model::Frontend::Resampler& r, int sr_in) {
    WMCHK(resample_ratio(sr_in, &r.orig, &r.nw, &r.width));
    std::vector<float> h;
    resample_taps_host(r.orig, r.nw, r.width, h);
    const int K = 2 * r.width + r.orig;
    std::vector<int32_t> span(2 * (size_t)r.nw, 0);
    int most = 1;
    for (int p = 0; p < r.nw; ++p) {
        int lo = K, hi = 0;
        for (int k = 0; k < K; ++k)
            if (h[(size_t)p * K + k] != 0.f) lo = std::min(lo, k), hi = k + 1;
        if (lo < hi) span[2 * p] = lo, span[2 * p + 1] = hi - lo;
        most = std::max(most, span[2 * p + 1]);
    }
    std::vector<float> compact((size_t)most * r.nw, 0.f);
    for (int p = 0; p < r.nw; ++p)
        for (int q = 0; q < span[2 * p + 1]; ++q) compact[(size_t)q * r.nw + p] = h[(size_t)p * K + span[2 * p] + q];
    WMCHK(r.taps.alloc(compact.size() * 4));
    WMCHK(r.span.alloc(span.size() * 4));
    HIPCHK(hipMemcpy(r.taps.p, compact.data(), compact.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(r.span.p, span.data(), span.size() * 4, hipMemcpyHostToDevice));
    r.frames = resample_frames(r.orig, r.nw, r.width);
    r.sr = sr_in;
    return 0;
}
// what both entries refuse before anything is launched; n_out [B] and the longest row's output length
static int resample_check(const void* in, int in_dtype, const int32_t* n_in, int B, int64_t stride_in, int sr_in, const void* out, int64_t stride_out,
                          int32_t* n_out, int64_t* longest) {
    if (!in || !out || !n_in || !n_out || B <= 0 || stride_in <= 0 || stride_out <= 0) return fail(WM_E_ARG, "bad argument");
    int orig, nw, width;
    WMCHK(resample_ratio(sr_in, &orig, &nw, &width));
    if (in_dtype != WM_F32 && in_dtype != WM_I16) return fail(WM_E_ARG, "in_dtype = %d is neither WM_F32 nor WM_I16", in_dtype);
    if (B > 65535) return fail(WM_E_ARG, "B = %d rows exceed 65535", B);
    *longest = 0;
    for (int b = 0; b < B; ++b) {
        if (n_in[b] < 0 || n_in[b] > stride_in) return fail(WM_E_ARG, "n_in[%d] = %d outside [0, stride_in = %lld]", b, n_in[b], (long long)stride_in);
        int64_t n = 0;
        WMCHK(resample_len(n_in[b], orig, nw, &n));
        if (n > INT32_MAX) return fail(WM_E_SIZE, "row %d resamples to %lld samples, more than 2^31 - 1", b, (long long)n);
        *longest = std::max(*longest, n);
    }
    if (*longest > stride_out) return fail(WM_E_SIZE, "stride_out = %lld is smaller than the longest row's %lld samples", (long long)stride_out, (long long)*longest);
    for (int b = 0; b < B; ++b) n_out[b] = (int32_t)(((int64_t)n_in[b] * nw + orig - 1) / orig);
    return 0;
}
static int resample_launch(const wm_model::Frontend::Resampler& r, const void* d_in, int in_dtype, const int* d_nin, int B, int64_t stride_in, float* d_out,
                           int64_t stride_out, int* d_nout, int64_t longest, hipStream_t st) {
    ResampleParams p{};
    p.x = d_in, p.y = d_out, p.n_in = d_nin, p.n_out = d_nout;
    p.stride_in = (size_t)stride_in, p.stride_out = (size_t)stride_out;
    p.taps = r.taps.as<float>(), p.span = r.span.as<int>();
    p.orig = r.orig, p.nw = r.nw, p.width = r.width, p.frames = r.frames;
    LCHK(launch_resample(p, in_dtype == WM_I16, B, longest, st));
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int wm_op_resample(float* out, const void* in, int in_dtype, const int32_t* n_in, int B, int64_t stride_in, int sr_in, int64_t stride_out,
                              int32_t* n_out) {
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int64_t longest = 0;
    std::vector<int32_t> no(std::max(B, 1));
    WMCHK(resample_check(in, in_dtype, n_in, B, stride_in, sr_in, out, stride_out, no.data(), &longest));
    wm_model::Frontend::Resampler r;
    TmpDev tmp;
    DevBuf &din = tmp.add(), &dout = tmp.add(), &dni = tmp.add(), &dno = tmp.add();
    const size_t es = in_dtype == WM_I16 ? 2 : 4, nin = (size_t)B * stride_in, nout = (size_t)B * stride_out;
    int rc = resampler_build(r, sr_in);
    auto run = [&]() -> int {
        WMCHK(upload_bytes(din, in, nin * es));
        WMCHK(upload_bytes(dout, out, nout * 4));  // in and out: a cell the kernel does not store keeps the caller's value
        WMCHK(upload_bytes(dni, n_in, (size_t)B * 4));
        WMCHK(upload_bytes(dno, n_out, (size_t)B * 4));
        WMCHK(resample_launch(r, din.p, in_dtype, dni.as<int>(), B, stride_in, dout.as<float>(), stride_out, dno.as<int>(), longest, nullptr));
        HIPCHK(hipMemcpy(out, dout.p, nout * 4, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(n_out, dno.p, (size_t)B * 4, hipMemcpyDeviceToHost));  // what the kernel computed, not the host's copy
        return 0;
    };
    if (!rc) rc = run();
    r.taps.release();
    r.span.release();
    return rc;
}
static int resampler_get(wm_model* m, int sr_in, wm_model::Frontend::Resampler** out) {
    for (auto* r : m->fe.rs)
        if (r->sr == sr_in) {
            *out = r;
            return 0;
        }
    auto* r = new wm_model::Frontend::Resampler();
    const int rc = resampler_build(*r, sr_in);
    if (rc) {
        r->taps.release();
        r->span.release();
        delete r;
        return rc;
    }
    m->fe.rs.push_back(r);
    *out = r;
    return 0;
}
extern "C" int wm_resample_pcm(wm_model* m, const void* in, int in_dtype, int in_on_device, const int32_t* n_in, int B, int64_t stride_in, int sr_in,
                               float* out, int out_on_device, int64_t stride_out, int32_t* n_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    if (!n_out) return fail(WM_E_ARG, "bad argument");
    int64_t longest = 0;
    std::vector<int32_t> no(std::max(B, 1));
    WMCHK(resample_check(in, in_dtype, n_in, B, stride_in, sr_in, out, stride_out, no.data(), &longest));
    if (stride_out > INT32_MAX) return fail(WM_E_SIZE, "stride_out = %lld exceeds 2^31 - 1", (long long)stride_out);
    HIPCHK(hipSetDevice(m->device));
    wm_model::Frontend::Resampler* r = nullptr;
    WMCHK(resampler_get(m, sr_in, &r));
    hipStream_t st = m->stream;
    TmpDev tmp;
    DevBuf &din = tmp.add(), &dout = tmp.add(), &dni = tmp.add(), &dno = tmp.add();
    const size_t es = in_dtype == WM_I16 ? 2 : 4, nin = (size_t)B * stride_in, nout = (size_t)B * stride_out;
    auto run = [&]() -> int {
        const void* d_in = in;
        float* d_out = out;
        if (!in_on_device) {
            WMCHK(din.alloc(nin * es));
            HIPCHK(hipMemcpyAsync(din.p, in, nin * es, hipMemcpyHostToDevice, st));
            d_in = din.p;
        }
        if (!out_on_device) {
            WMCHK(dout.alloc(nout * 4));
            d_out = dout.as<float>();
        }
        WMCHK(dni.alloc((size_t)B * 4));
        WMCHK(dno.alloc((size_t)B * 4));
        HIPCHK(hipMemcpyAsync(dni.p, n_in, (size_t)B * 4, hipMemcpyHostToDevice, st));
        WMCHK(resample_launch(*r, d_in, in_dtype, dni.as<int>(), B, stride_in, d_out, stride_out, dno.as<int>(), longest, st));
        launch_zero_tails(d_out, dno.as<int>(), B, (int)stride_out, st);  // the model path hands on rows that are zero past their length
        HIPCHK(hipGetLastError());
        if (!out_on_device) HIPCHK(hipMemcpyAsync(out, dout.p, nout * 4, hipMemcpyDeviceToHost, st));
        return 0;
    };
    const int rc = run();
    const std::string err = g_err;
    const hipError_t e = hipStreamSynchronize(st);  // the scratch is released on return, and no[] is the caller's from here
    if (rc) {
        g_err = err;
        return rc;
    }
    if (e != hipSuccess) return fail(WM_E_HIP, "hipStreamSynchronize: %s", hipGetErrorString(e));
    std::copy(no.begin(), no.begin() + B, n_out);
    return 0;
}

// ---- chunked long-form transcription -----------------------------------------------------------------------------
// HF's ASR pipeline with chunk_length_s / stride_length_s: overlapping chunks cut by pipelines/automatic_speech_recognition.py::chunk_iter,
// every chunk decoded on its own in batches, the id lists stitched by tokenization_whisper._find_longest_common_sequence.
static const int CHUNK_COLS = 6;  // (recording, start, len, stride_left, stride_right, is_last)
extern "C" int wm_chunk_table(const int32_t* n_samples, int R, int chunk_len, int stride_left, int stride_right, int window, int32_t* table, int cap,
                              int32_t* n_chunks) {
    if (!n_samples || R <= 0 || !n_chunks || cap < 0 || (cap > 0 && !table)) return fail(WM_E_ARG, "bad argument");
    if (chunk_len <= 0 || stride_left < 0 || stride_right < 0) return fail(WM_E_ARG, "chunk_len must be positive and the strides non-negative");
    const int64_t step = (int64_t)chunk_len - stride_left - stride_right;
    if (step <= 0)  // HF: "Chunk length must be superior to stride length" for <; the equal case dies in chunk_iter's range(0, n, 0)
        return fail(WM_E_ARG, "chunk_len %d must exceed stride_left %d + stride_right %d", chunk_len, stride_left, stride_right);
    if (window > 0 && chunk_len > window) return fail(WM_E_ARG, "chunk_len %d exceeds the model's window of %d samples", chunk_len, window);
    int64_t n = 0;
    for (int r = 0; r < R; ++r) {
        const int64_t T = n_samples[r];
        if (T < 0) return fail(WM_E_ARG, "n_samples[%d] = %d is negative", r, n_samples[r]);
        for (int64_t start = 0; start < T; start += step) {
            const int64_t end = start + chunk_len, len = std::min(T, end) - start;
            const int sl = start == 0 ? 0 : stride_left;
            const bool last = end >= T;
            if (len > sl) {
                if (n < cap) {
                    int32_t* t = table + n * CHUNK_COLS;
                    t[0] = r, t[1] = (int32_t)start, t[2] = (int32_t)len, t[3] = sl, t[4] = last ? 0 : stride_right, t[5] = last;
                }
                ++n;
            }
            if (last) break;
        }
    }
    if (n > INT32_MAX) return fail(WM_E_SIZE, "more than 2^31 chunks");
    *n_chunks = (int32_t)n;
    if (table && n > cap) return fail(WM_E_SIZE, "the table holds %d chunks, %lld are needed", cap, (long long)n);
    return 0;
}

extern "C" int wm_op_chunk_gather(float* out, const float* pcm, int R, int64_t T_max, const int32_t* items, int n, int N) {
    if (!out || !pcm || !items || R <= 0 || T_max <= 0 || n <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    for (int k = 0; k < n; ++k) {
        const int32_t* t = items + 3 * (size_t)k;
        if (t[0] < 0 || t[0] >= R || t[1] < 0 || t[2] < 0 || t[2] > N || (int64_t)t[1] + t[2] > T_max)
            return fail(WM_E_ARG, "item %d = (%d, %d, %d) leaves pcm [%d][%lld] or the row of %d samples", k, t[0], t[1], t[2], R, (long long)T_max, N);
    }
    TmpDev tmp;
    DevBuf &dp = tmp.add(), &di = tmp.add(), &dout = tmp.add();
    WMCHK(upload_bytes(dp, pcm, (size_t)R * T_max * 4));
    WMCHK(upload_bytes(di, items, (size_t)n * 3 * 4));
    WMCHK(upload_bytes(dout, out, (size_t)n * N * 4));  // in and out: a store the kernel misses keeps the caller's value
    launch_chunk_gather(dp.as<float>(), di.as<int>(), 3, 0, dout.as<float>(), n, (size_t)T_max, N, nullptr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, dout.p, (size_t)n * N * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ids [n_rows][stride] + lens [n_rows] -> the packed rows the kernel reads, [n_rows][1 + stride]
extern "C" int wm_op_chunk_merge(int32_t* merged, int32_t* merged_len, const int32_t* ids, const int32_t* lens, const int32_t* rec_off, int n_rows,
                                 int n_rec, int stride, int cap, int first_special) {
    if (!merged || !merged_len || !ids || !lens || !rec_off || n_rows <= 0 || n_rec <= 0 || stride <= 0 || cap <= 0) return fail(WM_E_ARG, "bad argument");
    if (rec_off[0] < 0 || rec_off[n_rec] > n_rows) return fail(WM_E_ARG, "rec_off leaves the %d rows", n_rows);
    for (int r = 0; r < n_rec; ++r)
        if (rec_off[r + 1] < rec_off[r]) return fail(WM_E_ARG, "rec_off must not decrease");
    std::vector<int32_t> packed((size_t)n_rows * (1 + stride), 0);
    for (int k = 0; k < n_rows; ++k) {
        if (lens[k] < 0 || lens[k] > stride) return fail(WM_E_ARG, "lens[%d] = %d outside [0, %d]", k, lens[k], stride);
        packed[(size_t)k * (1 + stride)] = lens[k];
        std::copy(ids + (size_t)k * stride, ids + (size_t)k * stride + lens[k], packed.begin() + (size_t)k * (1 + stride) + 1);
    }
    for (int r = 0; r < n_rec; ++r) {  // cap must hold the recording's ids even when nothing overlaps
        int64_t sum = 0;
        for (int k = rec_off[r]; k < rec_off[r + 1]; ++k) sum += lens[k];
        if (sum > cap) return fail(WM_E_ARG, "recording %d has %lld ids, cap is %d", r, (long long)sum, cap);
    }
    TmpDev tmp;
    DevBuf &dr = tmp.add(), &doff = tmp.add(), &dm = tmp.add(), &dl = tmp.add();
    WMCHK(upload_bytes(dr, packed.data(), packed.size() * 4));
    WMCHK(upload_bytes(doff, rec_off, (size_t)(n_rec + 1) * 4));
    WMCHK(upload_bytes(dm, merged, (size_t)n_rec * cap * 4));  // in and out, as wm_op_chunk_gather
    WMCHK(dl.alloc((size_t)n_rec * 4));
    LCHK(launch_chunk_merge(dr.as<int>(), doff.as<int>(), n_rec, stride, first_special, dm.as<int>(), dl.as<int>(), cap, nullptr));
    HIPCHK(hipMemcpy(merged, dm.p, (size_t)n_rec * cap * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(merged_len, dl.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    return 0;
}

// Chunks of all recordings fill passes of up to max_batch rows, in table order; passes alternate over the caller's slots 0..1 (0..3 under
// coalesce = 2, where two submits make one pass), so two passes are in flight, each with a log-mel buffer of its own.  A pass's ids go
// from its decode state into the packed table on the device (wm_transcribe_wait_device's rows); the stitch reads that table.
// The timestamp outputs of wm_transcribe_chunked_ts.  mode 0: none of this — wm_transcribe_chunked, which launches what it
// always launched.  mode 1 (segments): chunk_segments_kernel stitches instead of chunk_merge_kernel.  mode 2 (word): every pass also
// carries the alignment-head capture with per-row n_frames = len // 160, and its times are packed next to its ids.
struct ChunkTs {
    int mode = 0;
    double time_precision = 0.0;
    int32_t* n_seg = nullptr;
    double* seg_times = nullptr;
    int32_t* seg_range = nullptr;
    int seg_cap = 0;
    double* pairs = nullptr;
    float* chunk_times = nullptr;
};
static int chunked_impl(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                        int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang, int first_special,
                        int32_t* merged, int32_t* merged_len, int cap, int32_t* chunk_ids, int32_t* chunk_n, int32_t* n_passes, const ChunkTs& ts) {
    if (!m || !pcm || !n_samples || R <= 0 || stride <= 0 || !merged || !merged_len || cap <= 0 || (!chunk_ids != !chunk_n) || first_special <= 0)
        return fail(WM_E_ARG, "bad argument");
    const wm_dims& c = m->cfg.dims;
    const int n_frames = 2 * c.n_audio_ctx, N = FE_HOP * n_frames;
    WMCHK(check_opts(m, o, 1));
    if (m->top_k > 0)  // (the stitched result has no place for them yet)
        return fail(WM_E_ARG, "top-k alternatives (wm_set_top_k) are not available in chunked transcription: set top_k to 0");
    const bool word = ts.mode == 2;
    if (ts.mode) {  // everything is refused before anything is launched
        if (ts.mode != 1 && ts.mode != 2) return fail(WM_E_ARG, "mode must be 1 (segments) or 2 (word)");
        if (!ts.n_seg || !ts.seg_times || !ts.seg_range || ts.seg_cap <= 0 || (word && !ts.pairs) || (ts.chunk_times && (!word || !chunk_ids)))
            return fail(WM_E_ARG, "bad argument");
        if (o->timestamp_begin <= 0) return fail(WM_E_ARG, "chunked timestamps need the timestamp rule (opts->timestamp_begin)");
        if (o->timestamp_begin < first_special) return fail(WM_E_ARG, "timestamp_begin %d lies below first_special %d", o->timestamp_begin, first_special);
        if (word && m->align_pairs.empty()) return fail(WM_E_ARG, "word timestamps need alignment heads (wm_set_alignment_heads)");
        if (word && lang_ids) return fail(WM_E_ARG, "word timestamps do not combine with language detection (a language pass carries no token timestamps)");
        if (ts.time_precision < 0.0 || ts.time_precision != ts.time_precision) return fail(WM_E_ARG, "time_precision must be positive (0: the model's)");
    }
    for (int r = 0; r < R; ++r)
        if (n_samples[r] < 0 || n_samples[r] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", r, n_samples[r]);
    int32_t n = 0;
    WMCHK(wm_chunk_table(n_samples, R, chunk_len, stride_left, stride_right, N, nullptr, 0, &n));
    std::vector<int32_t> tab((size_t)std::max(n, 1) * CHUNK_COLS), off(R + 1, 0);
    WMCHK(wm_chunk_table(n_samples, R, chunk_len, stride_left, stride_right, N, tab.data(), n, &n));
    for (int k = 0; k < n; ++k) ++off[tab[(size_t)k * CHUNK_COLS] + 1];
    int most = 0;
    for (int r = 0; r < R; ++r) {
        most = std::max(most, off[r + 1]);
        off[r + 1] += off[r];
    }
    const int total = o->n_prompt + 1 + o->max_loop;
    if ((int64_t)most * total > cap) return fail(WM_E_SIZE, "cap %d is smaller than %d chunks x %d ids of the longest recording", cap, most, total);
    if (ts.mode && total > CHUNK_MERGE_MAX_IDS) return fail(WM_E_ARG, "more than %d ids per chunk", CHUNK_MERGE_MAX_IDS);
    if (word)
        for (int k = 0; k < n; ++k)
            if (tab[(size_t)k * CHUNK_COLS + 2] < 2 * FE_HOP)
                return fail(WM_E_ARG, "chunk %d has %d samples: word timestamps need two mel frames of audio per chunk", k, tab[(size_t)k * CHUNK_COLS + 2]);
    if (ts.mode) std::fill(ts.n_seg, ts.n_seg + R, 0);
    const int PB = std::min(m->cfg.max_batch, std::max(n, 1));
    if (lang_ids) {  // what a _lang pass would refuse, before anything is launched
        WMCHK(lang_list_check(c.vocab, lang_ids, n_lang));
        if (o->n_prompt < 2) return fail(WM_E_ARG, "language detection needs at least two initial ids");
        if (dec_lanes_for(PB) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    }
    if (n_passes) *n_passes = 0;
    std::fill(merged_len, merged_len + R, 0);
    if (n == 0) return 0;
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    WMCHK(flush_held(m));
    const int NS = m->cfg.coalesce == 2 ? 4 : 2;
    for (int s = 0; s < NS; ++s)
        if (m->slot_ref[s].pending) return fail(WM_E_STATE, "slot %d still holds a pass that was not waited for (chunked transcription uses slots 0..%d)", s, NS - 1);
    hipStream_t st = m->stream;
    TmpDev tmp;
    DevBuf &d_pcm = tmp.add(), &d_tab = tmp.add(), &d_off = tmp.add(), &d_packed = tmp.add(), &d_merged = tmp.add(), &d_len = tmp.add();
    DevBuf &d_times = tmp.add(), &d_nseg = tmp.add(), &d_segt = tmp.add(), &d_segr = tmp.add(), &d_pairs = tmp.add();
    if (ts.mode) {
        WMCHK(d_nseg.alloc((size_t)R * 4));
        WMCHK(d_segt.alloc((size_t)R * ts.seg_cap * 2 * 8));
        WMCHK(d_segr.alloc((size_t)R * ts.seg_cap * 2 * 4));
    }
    if (word) {
        WMCHK(d_times.alloc((size_t)n * total * 4));
        WMCHK(d_pairs.alloc((size_t)R * cap * 2 * 8));
    }
    const float* dpcm = pcm;
    if (!pcm_on_device) {
        WMCHK(d_pcm.alloc((size_t)R * stride * 4));
        HIPCHK(hipMemcpyAsync(d_pcm.p, pcm, (size_t)R * stride * 4, hipMemcpyHostToDevice, st));
        dpcm = d_pcm.as<float>();
    }
    WMCHK(d_tab.alloc(tab.size() * 4));
    WMCHK(d_off.alloc(off.size() * 4));
    WMCHK(d_packed.alloc((size_t)n * (1 + total) * 4));
    WMCHK(d_merged.alloc((size_t)R * cap * 4));
    WMCHK(d_len.alloc((size_t)R * 4));
    HIPCHK(hipMemcpyAsync(d_tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));  // the chunk table and (below) its recording offsets: all that crosses the bus
    HIPCHK(hipMemcpyAsync(d_off.p, off.data(), off.size() * 4, hipMemcpyHostToDevice, st));
    DevBuf* d_mel[4];
    for (int s = 0; s < NS; ++s) {
        d_mel[s] = &tmp.add();
        WMCHK(d_mel[s]->alloc((size_t)PB * c.n_mels * n_frames * 4));
    }
    struct Pend {
        int row0 = 0, rows = 0;
        bool live = false;
    } pend[4];
    auto collect = [&](int s) {
        Pend& p = pend[s];
        p.live = false;
        PassOut out;
        out.dev_packed = d_packed.as<int32_t>() + (size_t)p.row0 * (1 + total);
        out.rows_cap = p.rows;
        out.pack_stride = total;
        if (word) out.dev_times = d_times.as<float>() + (size_t)p.row0 * total;  // this pass's times, next to its ids
        return collect_slot(m, s, PassKind::transcribe, out);
    };
    int rc = 0, np = 0;
    std::string err;
    for (int row0 = 0; row0 < n && !rc; row0 += PB, ++np) {
        const int s = np % NS, rows = std::min(PB, n - row0);
        if (pend[s].live) rc = collect(s);
        if (!rc) {
            launch_chunk_gather(dpcm, d_tab.as<int>(), CHUNK_COLS, row0, m->fe.pcm.as<float>(), rows, (size_t)stride, N, st);
            rc = frontend_compute(m, rows, d_mel[s]->as<float>());
        }
        if (!rc && word) {  // the ragged form of §28: row b keeps (len // 160) // 2 encoder positions
            std::vector<int32_t> nf(rows), cols;
            for (int b = 0; b < rows; ++b) nf[b] = tab[(size_t)(row0 + b) * CHUNK_COLS + 2] / FE_HOP;
            rc = align_cols(m, nf.data(), rows, cols);
            if (!rc) {
                PassAsk ask{d_mel[s]->as<float>(), 1, rows, o};
                ask.cols = &cols;
                rc = submit_slot(m, s, ask);
            }
        } else if (!rc)
            rc = lang_ids ? lang_entry(m, s, d_mel[s]->as<float>(), 1, rows, o, nullptr, nullptr, 0, false, -1, o->n_prompt, lang_ids, n_lang, PassOut())
                          : submit_slot(m, s, PassAsk{d_mel[s]->as<float>(), 1, rows, o});
        if (!rc) {
            pend[s].row0 = row0, pend[s].rows = rows, pend[s].live = true;
        } else {
            err = g_err;
        }
    }
    for (int k = 0; k < NS; ++k) {  // the oldest pass first; after a failure the rest is still collected, so no slot stays pending
        const int s = (np + k) % NS;
        if (!pend[s].live) continue;
        const int rc2 = collect(s);
        if (rc2 && !rc) rc = rc2, err = g_err;
    }
    if (rc) {
        (void)hipStreamSynchronize(st);  // the scratch is released on return
        g_err = err;
        return rc;
    }
    if (n_passes) *n_passes = np;
    if (ts.mode) {
        ChunkSegArgs a{};
        a.rows = d_packed.as<int>();
        a.rec_off = d_off.as<int>();
        a.tab = d_tab.as<int>();
        a.times = word ? d_times.as<float>() : nullptr;
        a.tab_cols = CHUNK_COLS, a.tab_c0 = 2, a.stride = total, a.first_special = first_special, a.timestamp_begin = o->timestamp_begin;
        a.segment_size = c.n_audio_ctx;
        a.time_precision = ts.time_precision > 0.0 ? ts.time_precision : (double)N / 16000.0 / (double)c.n_audio_ctx;
        a.merged = d_merged.as<int>(), a.merged_len = d_len.as<int>(), a.n_seg = d_nseg.as<int>();
        a.seg_times = (double*)d_segt.p, a.seg_range = d_segr.as<int>(), a.pairs = word ? (double*)d_pairs.p : nullptr;
        a.cap = cap, a.seg_cap = ts.seg_cap;
        LCHK(launch_chunk_segments(a, R, st));
        HIPCHK(hipMemcpyAsync(ts.n_seg, d_nseg.p, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    } else {
        LCHK(launch_chunk_merge(d_packed.as<int>(), d_off.as<int>(), R, total, first_special, d_merged.as<int>(), d_len.as<int>(), cap, st));
    }
    HIPCHK(hipMemcpyAsync(merged_len, d_len.p, (size_t)R * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int r = 0; r < R && ts.mode; ++r)
        if (ts.n_seg[r] > ts.seg_cap) return fail(WM_E_SIZE, "recording %d has %d segments, seg_cap is %d", r, ts.n_seg[r], ts.seg_cap);
    for (int r = 0; r < R; ++r) {
        if (merged_len[r] > 0)
            HIPCHK(hipMemcpyAsync(merged + (size_t)r * cap, d_merged.as<int32_t>() + (size_t)r * cap, (size_t)merged_len[r] * 4, hipMemcpyDeviceToHost, st));
        if (word && merged_len[r] > 0)
            HIPCHK(hipMemcpyAsync(ts.pairs + (size_t)r * cap * 2, (const double*)d_pairs.p + (size_t)r * cap * 2, (size_t)merged_len[r] * 16, hipMemcpyDeviceToHost, st));
        if (ts.mode && ts.n_seg[r] > 0) {
            const size_t at = (size_t)r * ts.seg_cap * 2;
            HIPCHK(hipMemcpyAsync(ts.seg_times + at, (const double*)d_segt.p + at, (size_t)ts.n_seg[r] * 16, hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(ts.seg_range + at, d_segr.as<int32_t>() + at, (size_t)ts.n_seg[r] * 8, hipMemcpyDeviceToHost, st));
        }
    }
    if (ts.chunk_times)
        HIPCHK(hipMemcpyAsync(ts.chunk_times, d_times.p, (size_t)n * total * 4, hipMemcpyDeviceToHost, st));
    if (chunk_ids) {  // on request: every chunk's own ids, as wm_transcribe_pcm of that chunk's samples returns them
        HIPCHK(hipMemcpy2DAsync(chunk_n, 4, d_packed.p, (size_t)(1 + total) * 4, 4, n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpy2DAsync(chunk_ids, (size_t)total * 4, d_packed.as<int32_t>() + 1, (size_t)(1 + total) * 4, (size_t)total * 4, n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int wm_transcribe_chunked(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                                     int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang, int first_special,
                                     int32_t* merged, int32_t* merged_len, int cap, int32_t* chunk_ids, int32_t* chunk_n, int32_t* n_passes) {
    return chunked_impl(m, pcm, pcm_on_device, n_samples, R, stride, chunk_len, stride_left, stride_right, o, lang_ids, n_lang, first_special, merged,
                        merged_len, cap, chunk_ids, chunk_n, n_passes, ChunkTs());
}
extern "C" int wm_transcribe_chunked_ts(wm_model* m, const float* pcm, int pcm_on_device, const int32_t* n_samples, int R, int stride, int chunk_len,
                                        int stride_left, int stride_right, const wm_decode_opts* o, const int32_t* lang_ids, int n_lang,
                                        int first_special, int mode, double time_precision, int32_t* merged, int32_t* merged_len, int cap,
                                        int32_t* n_seg, double* seg_times, int32_t* seg_range, int seg_cap, double* pairs, int32_t* chunk_ids,
                                        int32_t* chunk_n, float* chunk_times, int32_t* n_passes) {
    ChunkTs ts;
    ts.mode = mode;
    ts.time_precision = time_precision;
    ts.n_seg = n_seg, ts.seg_times = seg_times, ts.seg_range = seg_range, ts.seg_cap = seg_cap, ts.pairs = pairs, ts.chunk_times = chunk_times;
    if (mode != 1 && mode != 2) return fail(WM_E_ARG, "mode must be 1 (segments) or 2 (word)");
    return chunked_impl(m, pcm, pcm_on_device, n_samples, R, stride, chunk_len, stride_left, stride_right, o, lang_ids, n_lang, first_special, merged,
                        merged_len, cap, chunk_ids, chunk_n, n_passes, ts);
}

// chunk_segments_kernel alone: ids [n_rows][stride] with lens [n_rows], strides [n_rows][3] = (len, stride_left, stride_right) in samples,
// times [n_rows][stride] (word mode) or NULL (segments mode).  The outputs are uploaded first, so a cell the kernel does not store
// keeps the caller's value.
extern "C" int wm_op_chunk_segments(const int32_t* ids, const int32_t* lens, const int32_t* strides, const float* times, const int32_t* rec_off,
                                    int n_rows, int n_rec, int stride, int first_special, int timestamp_begin, double time_precision,
                                    int segment_size, int32_t* merged, int32_t* merged_len, int cap, int32_t* n_seg, double* seg_times,
                                    int32_t* seg_range, int seg_cap, double* pairs) {
    if (!ids || !lens || !strides || !rec_off || !merged || !merged_len || !n_seg || !seg_times || !seg_range || n_rows <= 0 || n_rec <= 0 ||
        stride <= 0 || cap <= 0 || seg_cap <= 0 || (times && !pairs))
        return fail(WM_E_ARG, "bad argument");
    if (rec_off[0] < 0 || rec_off[n_rec] > n_rows) return fail(WM_E_ARG, "rec_off leaves the %d rows", n_rows);
    for (int r = 0; r < n_rec; ++r)
        if (rec_off[r + 1] < rec_off[r]) return fail(WM_E_ARG, "rec_off must not decrease");
    std::vector<int32_t> packed((size_t)n_rows * (1 + stride), 0);
    for (int k = 0; k < n_rows; ++k) {
        if (lens[k] < 0 || lens[k] > stride) return fail(WM_E_ARG, "lens[%d] = %d outside [0, %d]", k, lens[k], stride);
        if (strides[3 * k] < 0 || strides[3 * k + 1] < 0 || strides[3 * k + 2] < 0) return fail(WM_E_ARG, "strides[%d] is negative", k);
        packed[(size_t)k * (1 + stride)] = lens[k];
        std::copy(ids + (size_t)k * stride, ids + (size_t)k * stride + lens[k], packed.begin() + (size_t)k * (1 + stride) + 1);
    }
    for (int r = 0; r < n_rec; ++r) {  // cap must hold the recording's ids even when nothing overlaps
        int64_t sum = 0;
        for (int k = rec_off[r]; k < rec_off[r + 1]; ++k) sum += lens[k];
        if (sum > cap) return fail(WM_E_SIZE, "recording %d has %lld ids, cap is %d", r, (long long)sum, cap);
    }
    TmpDev tmp;
    DevBuf &dr = tmp.add(), &doff = tmp.add(), &dtab = tmp.add(), &dtt = tmp.add(), &dm = tmp.add(), &dl = tmp.add(), &dn = tmp.add(), &dst = tmp.add(),
           &dsr = tmp.add(), &dp = tmp.add();
    const size_t nm = (size_t)n_rec * cap, ns = (size_t)n_rec * seg_cap * 2;
    WMCHK(upload_bytes(dr, packed.data(), packed.size() * 4));
    WMCHK(upload_bytes(doff, rec_off, (size_t)(n_rec + 1) * 4));
    WMCHK(upload_bytes(dtab, strides, (size_t)n_rows * 3 * 4));
    WMCHK(upload_bytes(dm, merged, nm * 4));
    WMCHK(dl.alloc((size_t)n_rec * 4));
    WMCHK(dn.alloc((size_t)n_rec * 4));
    WMCHK(upload_bytes(dst, seg_times, ns * 8));
    WMCHK(upload_bytes(dsr, seg_range, ns * 4));
    if (times) {
        WMCHK(upload_bytes(dtt, times, (size_t)n_rows * stride * 4));
        WMCHK(upload_bytes(dp, pairs, nm * 2 * 8));
    }
    ChunkSegArgs a{};
    a.rows = dr.as<int>(), a.rec_off = doff.as<int>(), a.tab = dtab.as<int>(), a.times = times ? dtt.as<float>() : nullptr;
    a.tab_cols = 3, a.tab_c0 = 0, a.stride = stride, a.first_special = first_special, a.timestamp_begin = timestamp_begin;
    a.segment_size = segment_size, a.time_precision = time_precision;
    a.merged = dm.as<int>(), a.merged_len = dl.as<int>(), a.n_seg = dn.as<int>(), a.seg_times = (double*)dst.p, a.seg_range = dsr.as<int>();
    a.pairs = times ? (double*)dp.p : nullptr;
    a.cap = cap, a.seg_cap = seg_cap;
    LCHK(launch_chunk_segments(a, n_rec, nullptr));
    HIPCHK(hipMemcpy(merged, dm.p, nm * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(merged_len, dl.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(n_seg, dn.p, (size_t)n_rec * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(seg_times, dst.p, ns * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(seg_range, dsr.p, ns * 4, hipMemcpyDeviceToHost));
    if (times) HIPCHK(hipMemcpy(pairs, dp.p, nm * 2 * 8, hipMemcpyDeviceToHost));
    for (int r = 0; r < n_rec; ++r)
        if (n_seg[r] > seg_cap) return fail(WM_E_SIZE, "recording %d has %d segments, seg_cap is %d", r, n_seg[r], seg_cap);
    return 0;
}

// ---- transcript scoring --------------------------------------------------------------------------------------------
// Row b holds ids y[0 .. len_b); its decoder input is y[0 .. len_b - 1), run through the per-row prefill's position-major chunks
// (left-padded so that the rows end together, key windows as in §16) with no logits launch; after every chunk the real rows of the
// last layer's residual stream are copied out, utterance-major; then one LayerNorm launch, one vocabulary sweep and the merge.
// Everything is refused before anything is launched.
static int score_check(wm_model* m, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len) {
    if (!m || !ids || !ids_len || B <= 0 || ids_stride < 2) return fail(WM_E_ARG, "bad argument");
    if (pos_mode != WM_POS_REF && pos_mode != WM_POS_HF) return fail(WM_E_ARG, "bad pos_mode");
    const wm_dims& c = m->cfg.dims;
    if (B > m->cfg.max_batch) return fail(WM_E_ARG, "batch %d exceeds max_batch %d", B, m->cfg.max_batch);
    if (dec_lanes_for(B) != 1) return fail(WM_E_ARG, "scoring needs a single-lane decode state");
    const int cap = std::min(ids_stride, c.n_text_ctx);
    for (int b = 0; b < B; ++b) {
        const int L = ids_len[b], cl = context_len ? context_len[b] : 1;
        if (L < 2 || L > cap) return fail(WM_E_ARG, "ids_len[%d] = %d outside [2, min(ids_stride, n_text_ctx) = %d]", b, L, cap);
        if (cl < 1 || cl > L - 1) return fail(WM_E_ARG, "context_len[%d] = %d outside [1, ids_len - 1 = %d]", b, cl, L - 1);
        for (int i = 0; i < L; ++i) {
            const int32_t id = ids[(size_t)b * ids_stride + i];
            if (id < 0 || id >= c.vocab) return fail(WM_E_ARG, "id %d of row %d out of range", id, b);
        }
    }
    return 0;
}
static int score_pass(wm_model* m, wm_state* s, const ScoreAsk& a) {
    const wm_dims& c = m->cfg.dims;
    const int B = s->B, T = dec_dtype(m->cfg);
    const size_t d = c.d_model;
    wm_state::Score& sc = s->sc;
    int Lmax = 0, M = 0;
    for (int b = 0; b < B; ++b) {
        Lmax = std::max(Lmax, a.len[b] - 1);
        M += a.len[b] - 1;
    }
    sc.M = M;
    sc.Lmax = Lmax;
    sc.stride = a.stride;
    sc.h_tok.assign((size_t)Lmax * B, 0);
    sc.h_pos.assign((size_t)Lmax * B, 0);
    sc.h_dst.assign((size_t)Lmax * B, -1);
    sc.h_key_lo.assign(B, 0);
    sc.h_target.assign(M, -1);
    sc.h_slot.assign(M, 0);
    sc.h_len.assign(a.len, a.len + B);
    sc.h_ctx.assign(B, 1);
    // an align pass: the cross-q rows of inputs t in [context_len, len - 1) are captured, R_b = len_b - context_len_b - 1
    const bool align = a.cols != nullptr, want_lp = !align || a.lp;
    wm_state::Align& al = s->al;
    int Lal = 0;
    if (align) {
        al.h_rows.assign(B, 0);
        al.h_row0.assign(B, 1);
        for (int b = 0; b < B; ++b) {
            al.h_row0[b] = a.ctx ? a.ctx[b] : 1;
            al.h_rows[b] = a.len[b] - al.h_row0[b] - 1;
            Lal = std::max(Lal, al.h_rows[b]);
        }
        al.h_map.assign((size_t)Lmax * B, -1);
    }
    for (int b = 0, base = 0; b < B; ++b) {
        const int n_in = a.len[b] - 1, pad = Lmax - n_in, cl = a.ctx ? a.ctx[b] : 1;
        const int32_t* y = a.ids + (size_t)b * a.stride;
        sc.h_ctx[b] = cl;
        sc.h_key_lo[b] = pad;
        for (int t = 0; t < Lmax; ++t) {
            const size_t o = (size_t)t * B + b;
            if (t < pad) {  // a dead slot in front of a shorter row: the row's first id at position 0, never attended to (§16)
                sc.h_tok[o] = y[0];
                continue;
            }
            const int i = t - pad;
            sc.h_tok[o] = y[i];
            // WM_POS_REF: the reference's loop feeds position current_len - 1 (whisper.mojo:217), as set_rows_step_kernel applies it
            sc.h_pos[o] = a.pos_mode == WM_POS_REF && i >= cl ? i - 1 : i;
            sc.h_dst[o] = base + i;
            if (align && i >= cl) al.h_map[o] = b * Lal + (i - cl);
            sc.h_target[base + i] = y[i + 1];
            sc.h_slot[base + i] = b * a.stride + i + 1;
        }
        base += n_in;
    }
    int spp = 0;
    const size_t parts = score_parts(c.vocab, T, &spp), ctx = c.n_text_ctx;
    WMCHK(grow(s->rw.key_lo, (size_t)B * 4));
    WMCHK(grow(s->tok_rows, (size_t)B * ctx * 4));
    WMCHK(grow(s->pos_rows, (size_t)B * ctx * 4));
    if (want_lp) {
        WMCHK(grow(sc.rows, (size_t)M * d * 4));
        WMCHK(grow(sc.a, score_operand_bytes(M, c.d_model, T)));
        for (DevBuf* p : {&sc.pmax, &sc.psum, &sc.pidx}) WMCHK(grow(*p, (size_t)M * parts * 4));
        for (DevBuf* p : {&sc.ztgt, &sc.target, &sc.slot}) WMCHK(grow(*p, (size_t)M * 4));
        WMCHK(grow(sc.dst, (size_t)B * ctx * 4));
        for (DevBuf* p : {&sc.len, &sc.ctx, &sc.sum, &sc.avg}) WMCHK(grow(*p, (size_t)B * 4));
        for (DevBuf* p : {&sc.lp, &sc.top}) WMCHK(grow(*p, (size_t)B * a.stride * 4));
    }
    al.on = al.ragged = align;
    al.win = false;
    if (align) {  // the buffers of a timestamp pass, sized by the longest row of THIS pass
        al.pairs = m->align_pairs;
        al.L = Lal;
        al.n_prompt = 0;
        al.stride = a.stride;
        al.cols = *a.cols;
        ++al.gen;
        invalidate_step_graphs(s);  // the captured step graph may hold a capture into a buffer that is re-sized here
        WMCHK(align_buffers(m, s, std::max(Lal, 1), a.stride));
        for (DevBuf* p : {&al.rows, &al.row0}) WMCHK(grow(*p, (size_t)B * 4));
        WMCHK(grow(al.map, (size_t)B * ctx * 4));
    }
    s->rw.on = true;  // the prefill's self-attention sweeps each row's own key window
    s->rw.Lmax = Lmax;
    sc.on = true;
    const wm_state::Lane& ln = s->lanes[0];
    const DecView v{ln.b0, ln.nb, ln.st, ln.ctl};
    HIPCHK(hipEventRecord(s->enc_done, s->enc_stream ? s->enc_stream : m->stream));
    HIPCHK(hipStreamWaitEvent(v.st, s->enc_done, 0));
    auto up = [&](DevBuf& dst, const std::vector<int32_t>& h) { return hipMemcpyAsync(dst.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, v.st); };
    HIPCHK(up(s->tok_rows, sc.h_tok));
    HIPCHK(up(s->pos_rows, sc.h_pos));
    HIPCHK(up(s->rw.key_lo, sc.h_key_lo));
    if (want_lp) {
        HIPCHK(up(sc.dst, sc.h_dst));
        HIPCHK(up(sc.target, sc.h_target));
        HIPCHK(up(sc.slot, sc.h_slot));
        HIPCHK(up(sc.len, sc.h_len));
        HIPCHK(up(sc.ctx, sc.h_ctx));
        HIPCHK(hipMemsetAsync(sc.lp.p, 0, (size_t)B * a.stride * 4, v.st));     // logprob[b][0] and the tails: 0
        HIPCHK(hipMemsetAsync(sc.top.p, 0xff, (size_t)B * a.stride * 4, v.st));  // top_id[b][0] and the tails: -1
    }
    if (align) {  // (the host vectors outlive the copies: the state is not reused before this pass is waited for)
        HIPCHK(up(al.map, al.h_map));
        HIPCHK(up(al.rows, al.h_rows));
        HIPCHK(up(al.row0, al.h_row0));
        HIPCHK(up(al.ncols, al.cols));
    }
    HIPCHK(hipEventRecord(sc.ev[1], v.st));
    trace_mark(v.st, "state %p score prefill start", (void*)s);
    for (int t0 = 0; t0 < Lmax; t0 += wm_state::PREFILL_MAX) {
        const int P = std::min<int>(wm_state::PREFILL_MAX, Lmax - t0);
        launch_set_step(v.ctl, t0, 1, nullptr, 0, nullptr, 0, v.nb, v.st);
        DecPass chunk;
        chunk.P = P;
        chunk.t0 = t0;
        chunk.capture = align && Lal > 0;
        WMCHK(decode_core(m, s, v, chunk));
        if (want_lp) launch_score_collect(s->dx.as<float>(), sc.rows.as<float>(), sc.dst.as<int>() + (size_t)t0 * B, P * B, c.d_model, v.st);
    }
    HIPCHK(hipEventRecord(sc.ev[2], v.st));
    trace_mark(v.st, "state %p score prefill end", (void*)s);
    if (!want_lp) {  // times only: no LayerNorm, sweep, merge or sums
        for (int k = 3; k <= 5; ++k) HIPCHK(hipEventRecord(sc.ev[k], v.st));
    } else {
    const VocabHead h = vocab_head(m);
    ScoreParams q{};
    q.x = sc.rows.as<float>();
    q.ln_g = h.ln_g;
    q.ln_b = h.ln_b;
    q.emb = h.emb;
    q.a = sc.a.p;
    q.target = sc.target.as<int>();
    q.slot = sc.slot.as<int>();
    q.M = M;
    q.N = h.vocab;
    q.K = h.d_model;
    q.pmax = sc.pmax.as<float>();
    q.psum = sc.psum.as<float>();
    q.pidx = sc.pidx.as<int>();
    q.ztgt = sc.ztgt.as<float>();
    q.logprob = sc.lp.as<float>();
    q.top_id = sc.top.as<int>();
    int lrc = 0;
    DISPATCH_DT(T, TT, lrc = launch_score<TT>(q, v.st, sc.ev + 3));
    LCHK(lrc);
    launch_score_sums(sc.lp.as<float>(), a.stride, sc.len.as<int>(), sc.ctx.as<int>(), sc.sum.as<float>(), sc.avg.as<float>(), B, v.st);
    HIPCHK(hipEventRecord(sc.ev[5], v.st));
    }
    if (align) {  // the align chain on the lane's stream, before the pass's completion event
        WMCHK(enqueue_align(m, s));
        HIPCHK(hipEventRecord(sc.ev[6], v.st));
    }
    trace_mark(v.st, "state %p score end", (void*)s);
    HIPCHK(hipEventRecord(ln.done, ln.st));
    HIPCHK(hipGetLastError());
    s->enq_rc = 0;
    s->enq_done.store(true);
    return 0;
}
static int score_collect(wm_model* m, wm_state* s, const PassOut& out) {
    if (!s || !s->pending || !s->sc.on) return fail(WM_E_STATE, "no score pass was submitted on this slot");
    HIPCHK(hipSetDevice(m->device));
    const bool align = s->al.on;  // an align pass: out.token_times [B][stride] too, the log-probs only if it computed them
    const hipError_t e = hipEventSynchronize(s->lanes[0].done);
    s->pending = false;  // afterwards the state holds no usable pass, exactly as after wm_transcribe
    s->has_enc = false;
    s->sc.on = false;
    s->rw.on = false;
    s->al.on = false;
    HIPCHK(e);
    s->sc.timed = true;
    s->sc.timed_al = align;
    const size_t n = (size_t)s->B * s->sc.stride * 4;
    if (out.token_times) HIPCHK(hipMemcpy(out.token_times, s->al.times.p, n, hipMemcpyDeviceToHost));
    if (!out.token_logprobs) return 0;
    HIPCHK(hipMemcpy(out.token_logprobs, s->sc.lp.p, n, hipMemcpyDeviceToHost));
    if (out.top_ids) HIPCHK(hipMemcpy(out.top_ids, s->sc.top.p, n, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.sum_logprob, s->sc.sum.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out.avg_logprob, s->sc.avg.p, (size_t)s->B * 4, hipMemcpyDeviceToHost));
    return 0;
}
// the request and the outputs of a checked score / align call (a: the caller's ScoreAsk, alive for the call)
static PassAsk score_ask(const float* mel, int mel_on_device, int B, const ScoreAsk& a) {
    PassAsk ask{mel, mel_on_device, B};
    ask.score = &a;
    return ask;
}
static PassOut score_out(float* token_times, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    PassOut out;
    out.token_times = token_times;
    out.token_logprobs = token_logprobs;
    out.top_ids = top_ids;
    out.sum_logprob = sum_logprob;
    out.avg_logprob = avg_logprob;
    return out;
}
extern "C" int wm_score(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                        int ids_stride, const int32_t* context_len, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    if (!m || !mel || !token_logprobs || !sum_logprob || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return run_now(m, score_ask(mel, mel_on_device, B, a), score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}
extern "C" int wm_score_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids,
                               const int32_t* ids_len, int ids_stride, const int32_t* context_len) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return submit_slot(m, slot, score_ask(mel, mel_on_device, B, a));
}
extern "C" int wm_score_wait(wm_model* m, int slot, float* token_logprobs, int32_t* top_ids, float* sum_logprob, float* avg_logprob) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    return collect_slot(m, slot, PassKind::score, score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}
extern "C" int wm_score_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                            const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_logprobs, int32_t* top_ids,
                            float* sum_logprob, float* avg_logprob) {
    if (!m || !token_logprobs || !sum_logprob || !avg_logprob) return fail(WM_E_ARG, "bad argument");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream order as the encoder: no host sync
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode};
    return run_now(m, score_ask(m->fe.mel.as<float>(), 1, B, a), score_out(nullptr, token_logprobs, top_ids, sum_logprob, avg_logprob));
}
extern "C" int wm_score_phases(wm_model* m, int slot, float* ms) {
    if (!m || !ms || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    wm_state* s = *slot_state(m, slot);
    if (!s || !state_is_live(s) || s->pending || !s->sc.timed) return fail(WM_E_STATE, "no completed score pass on this slot's state");
    HIPCHK(hipSetDevice(m->device));
    for (int k = 0; k < 5; ++k) HIPCHK(hipEventElapsedTime(ms + k, s->sc.ev[k], s->sc.ev[k + 1]));
    return 0;
}

// ---- forced alignment ------------------------------------------------------------------------------------------------
// Token timestamps of a GIVEN transcript: the score pass with the alignment layers' cross-q rows captured by row map, then the align
// chain with per-row row counts and offsets.  token_logprobs / sum_logprob / avg_logprob are nullable as a group: without them the
// vocabulary side is not launched.  Everything is refused before anything is launched.
static int align_check(wm_model* m, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len, int ids_stride, const int32_t* context_len,
                       const int32_t* n_frames, const float* token_logprobs, const float* sum_logprob, const float* avg_logprob,
                       std::vector<int32_t>& cols) {
    if ((token_logprobs != nullptr) != (sum_logprob != nullptr) || (token_logprobs != nullptr) != (avg_logprob != nullptr))
        return fail(WM_E_ARG, "token_logprobs, sum_logprob and avg_logprob go together");
    WMCHK(score_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len));
    return align_cols(m, n_frames, B, cols);
}
extern "C" int wm_align(wm_model* m, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids, const int32_t* ids_len,
                        int ids_stride, const int32_t* context_len, const int32_t* n_frames, float* token_times, float* token_logprobs,
                        float* sum_logprob, float* avg_logprob) {
    if (!m || !mel || !token_times) return fail(WM_E_ARG, "bad argument");
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, n_frames, token_logprobs, sum_logprob, avg_logprob, cols));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, token_logprobs != nullptr};
    return run_now(m, score_ask(mel, mel_on_device, B, a), score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
extern "C" int wm_align_submit(wm_model* m, int slot, const float* mel, int mel_on_device, int B, int pos_mode, const int32_t* ids,
                               const int32_t* ids_len, int ids_stride, const int32_t* context_len, const int32_t* n_frames, int want_logprobs) {
    if (!m || !mel || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument (slot must be 0..7)");
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, n_frames, nullptr, nullptr, nullptr, cols));
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, want_logprobs != 0};
    return submit_slot(m, slot, score_ask(mel, mel_on_device, B, a));
}
extern "C" int wm_align_wait(wm_model* m, int slot, float* token_times, float* token_logprobs, float* sum_logprob, float* avg_logprob) {
    if (!m || !token_times || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    if ((token_logprobs != nullptr) != (sum_logprob != nullptr) || (token_logprobs != nullptr) != (avg_logprob != nullptr))
        return fail(WM_E_ARG, "token_logprobs, sum_logprob and avg_logprob go together");
    return collect_slot(m, slot, PassKind::align, score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
// n_frames from the sample counts, as wm_transcribe_pcm_tt
extern "C" int wm_align_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int pos_mode, const int32_t* ids,
                            const int32_t* ids_len, int ids_stride, const int32_t* context_len, float* token_times, float* token_logprobs,
                            float* sum_logprob, float* avg_logprob) {
    if (!m || !token_times || !n_samples || B <= 0) return fail(WM_E_ARG, "bad argument");
    std::vector<int32_t> nf(B);
    for (int b = 0; b < B; ++b) nf[b] = (int32_t)std::min<long>(2L * m->cfg.dims.n_audio_ctx, ((long)n_samples[b] + FE_HOP - 1) / FE_HOP);
    std::vector<int32_t> cols;
    WMCHK(align_check(m, B, pos_mode, ids, ids_len, ids_stride, context_len, nf.data(), token_logprobs, sum_logprob, avg_logprob, cols));
    WMCHK(frontend_run(m, pcm, n_samples, B, stride));  // same stream order as the encoder: no host sync
    const ScoreAsk a{ids, ids_len, context_len, ids_stride, pos_mode, &cols, token_logprobs != nullptr};
    return run_now(m, score_ask(m->fe.mel.as<float>(), 1, B, a), score_out(token_times, token_logprobs, nullptr, sum_logprob, avg_logprob));
}
// ms[6]: wm_score_phases' five (LayerNorm, sweep and merge are 0 for a pass without log-probs) and the align chain
extern "C" int wm_align_phases(wm_model* m, int slot, float* ms) {
    if (!m || !ms || slot < 0 || slot >= wm_model::NSLOT) return fail(WM_E_ARG, "bad argument");
    wm_state* s = *slot_state(m, slot);
    if (!s || !state_is_live(s) || s->pending || !s->sc.timed_al) return fail(WM_E_STATE, "no completed align pass on this slot's state");
    HIPCHK(hipSetDevice(m->device));
    for (int k = 0; k < 6; ++k) HIPCHK(hipEventElapsedTime(ms + k, s->sc.ev[k], s->sc.ev[k + 1]));
    return 0;
}
// The score pass's vocabulary side alone (LayerNorm, sweep, merge) on host operands: known-answer tests.
extern "C" int wm_op_score_logits(float* logprob, int32_t* top_id, const float* x, const float* ln_g, const float* ln_b, const float* emb,
                                  const int32_t* target, int M, int N, int K, int dtype) {
    if (!logprob || !top_id || !x || !ln_g || !ln_b || !emb || !target || M <= 0 || N <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(vocab_k_check(K));
    if (dtype < 0 || dtype > 2) return fail(WM_E_ARG, "bad dtype");
    for (int r = 0; r < M; ++r)
        if (target[r] >= N) return fail(WM_E_ARG, "target[%d] = %d is not a vocabulary id", r, target[r]);
    TmpDev t;
    const size_t parts = score_parts(N, dtype);
    const float* dx;
    VocabHead vh;
    WMCHK(upload_vocab_head(t, x, ln_g, ln_b, emb, M, N, K, dtype, &dx, &vh));
    DevBuf &a = t.add(), &pm = t.add(), &ps = t.add(), &pi = t.add(), &zt = t.add(), &tg = t.add(), &lp = t.add(), &top = t.add();
    WMCHK(a.alloc(score_operand_bytes(M, K, dtype)));
    for (DevBuf* p : {&pm, &ps, &pi}) WMCHK(p->alloc((size_t)M * parts * 4, true));
    for (DevBuf* p : {&zt, &lp, &top}) WMCHK(p->alloc((size_t)M * 4, true));
    WMCHK(upload_bytes(tg, target, (size_t)M * 4));
    ScoreParams q{};
    q.x = dx;
    q.ln_g = vh.ln_g;
    q.ln_b = vh.ln_b;
    q.emb = vh.emb;
    q.a = a.p;
    q.target = tg.as<int>();
    q.M = M;
    q.N = N;
    q.K = K;
    q.pmax = pm.as<float>();
    q.psum = ps.as<float>();
    q.pidx = pi.as<int>();
    q.ztgt = zt.as<float>();
    q.logprob = lp.as<float>();
    q.top_id = top.as<int>();
    int lrc = 0;
    DISPATCH_DT(dtype, TT, lrc = launch_score<TT>(q, nullptr));
    LCHK(lrc);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(logprob, lp.p, (size_t)M * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(top_id, top.p, (size_t)M * 4, hipMemcpyDeviceToHost));
    return 0;
}

// ---- sequential long-form transcription (thresholds and no-speech window skipping: §18) -----------------------------
struct wm_long_result {
    std::vector<std::vector<int32_t>> tokens;  // per utterance: the concatenation of its segments' ids
    std::vector<std::vector<wm_segment>> segs;
    int windows = 0, stalled = 0, passes = 0, rows = 0;
    int longest_prompt = 0, row_passes = 0;  // longest decoder prompt a window of a real utterance carried; passes that went per row
    // thresholds (quality = either use_* flag of wm_long_opts was set): per utterance the window log in decode order,
    // skipped windows included, and each segment's window values
    struct Window {
        int64_t seek;
        float avg_logprob, no_speech_prob;
        int32_t skipped;
    };
    bool quality = false;
    int skipped = 0;
    std::vector<std::vector<Window>> wins;
    std::vector<std::vector<float>> seg_avg, seg_nsp;
    // token timestamps (tt = the run computed them): per utterance one time per id of `tokens`
    bool tt = false;
    std::vector<std::vector<double>> times;
};

// The times of one window's kept ids: win[i] is generated id i's time with the window's offset (what align_window_kernel wrote);
// each segment takes its own slice, so the trailing eot and the ids behind the last kept segment leave no entry.
static void long_slice_times(const double* win, const std::vector<wm_segment>& segs, std::vector<double>& out) {
    for (const wm_segment& sg : segs) out.insert(out.end(), win + sg.first, win + sg.first + sg.count);
}
// align_window_kernel's arithmetic on the host, for wm_op_long_token_times: window-relative fp32 times -> float64 with time_offset
static void long_window_times(const float* rel, int n, int64_t seek, std::vector<double>& win) {
#pragma clang fp contract(off)
    const double off = (double)seek * 0.02 / 2;
    win.resize(n);
    for (int i = 0; i < n; ++i) win[i] = (double)rel[i] + off;
}

// HF WhisperGenerationMixin._retrieve_segment (time_precision 0.02, time_precision_features 0.01, input_stride 2) on one window's
// generated ids without the trailing eot.  Returns the seek advance in frames exactly as HF computes it (possibly 0).
static int long_segments(const int32_t* ids, int n, int tb, int64_t seek, int snf, std::vector<wm_segment>& out) {
#pragma clang fp contract(off)
    out.clear();
    const double off = (double)seek * 0.02 / 2;  // time_offset: float64(seek) * time_precision / input_stride
    auto ts = [&](int i) { return ids[i] >= tb; };
    const bool single_end = n >= 2 && !ts(n - 2) && ts(n - 1);  // timestamp_tokens[-2:] == [False, True]
    std::vector<int> slices;
    for (int i = 1; i < n; ++i)
        if (ts(i - 1) && ts(i)) slices.push_back(i);  // consecutive timestamps end a segment
    if (!slices.empty()) {
        if (single_end) slices.push_back(n);
        else slices.back() += 1;  // the last pair stays in the last segment
        int last = 0;
        for (size_t k = 0; k < slices.size(); ++k) {
            const int cur = slices[k];
            const bool is_last = k + 1 == slices.size();
            const int end_i = (!is_last || single_end) ? cur - 1 : cur - 2;
            out.push_back(wm_segment{last, cur - last, off + (double)(ids[last] - tb) * 0.02, off + (double)(ids[end_i] - tb) * 0.02});
            last = cur;
        }
        return single_end ? snf : (ids[last - 2] - tb) * 2;
    }
    // no pair: the whole window is one segment, ending at the last timestamp (other than <|0.00|>) or at the window's end — the
    // latter as HF computes it, int(seek_num_frames * 0.01 / 0.02) in float32 (a long tensor times a Python float)
    int last_ts = -1;
    for (int i = 0; i < n; ++i)
        if (ts(i)) last_ts = ids[i];
    const double end_pos = (last_ts >= 0 && last_ts != tb) ? (double)(last_ts - tb) : (double)(int)((float)snf * 0.01f / 0.02f);
    out.push_back(wm_segment{0, n, off, off + end_pos * 0.02});
    return snf;
}

extern "C" int wm_op_long_segments(const int32_t* ids, int n, int timestamp_begin, int64_t seek, int seek_num_frames, wm_segment* segs,
                                   int32_t* n_segs, int32_t* advance) {
    if (n < 0 || (n > 0 && !ids) || !segs || !n_segs || !advance || timestamp_begin <= 0 || seek < 0 || seek_num_frames < 0)
        return fail(WM_E_ARG, "bad argument");
    std::vector<wm_segment> out;
    *advance = long_segments(ids, n, timestamp_begin, seek, seek_num_frames, out);
    *n_segs = (int32_t)out.size();
    std::copy(out.begin(), out.end(), segs);
    return 0;
}

// The long-form scratch that grows with the audio goes back to the device once a call is done (the two decode states stay, like the
// slots').  hipFree waits for the device, and every pass of the call has been waited for.
static void long_release(wm_model* m) {
    wm_model::LongForm& L = m->lf;
    DevBuf* bs[] = {&L.pcm, &L.lens, &L.frames, &L.spec, &L.part, &L.mel, &L.in_mel, &L.win[0], &L.win[1], &L.items[0], &L.items[1]};
    for (DevBuf* b : bs) b->release();
}

// Log-mel of long audio into m->lf.mel [B][n_mels][stride / 160] (device): the 30 s path's kernels over chunks of frames of all
// utterances at once, so frames / spec stay one chunk however long the audio; then the two-stage max and the clamp / rescale.
static const int LONG_FE_ROWS = 16 * 3000;  // frames per DFT GEMM (the 30 s path's largest chunk)
static int frontend_long_run(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, int32_t* n_frames_out) {
    if (!pcm || !n_samples || B <= 0 || stride <= 200) return fail(WM_E_ARG, "bad argument (B >= 1, stride > 200 samples)");
    for (int b = 0; b < B; ++b)
        if (n_samples[b] < 0 || n_samples[b] > stride) return fail(WM_E_ARG, "n_samples[%d]=%d out of range", b, n_samples[b]);
    HIPCHK(hipSetDevice(m->device));
    WMCHK(frontend_init(m));
    const int n_mels = m->cfg.dims.n_mels, F = stride / FE_HOP;
    hipStream_t st = m->stream;
    wm_model::LongForm& L = m->lf;
    const int nt = std::max(32, std::min((F + 31) / 32 * 32, LONG_FE_ROWS / B / 32 * 32));  // frames per chunk and utterance
    const size_t rows = ((size_t)B * nt + 255) / 256 * 256 + 256;
    if (!L.frames.p || L.frames.bytes < rows * 416 * 4) WMCHK(L.frames.alloc(rows * 416 * 4, true));
    if (!L.spec.p || L.spec.bytes < rows * 512 * 4) WMCHK(L.spec.alloc(rows * 512 * 4, true));
    WMCHK(grow(L.pcm, (size_t)B * stride * 4));
    WMCHK(grow(L.lens, (size_t)B * 4));
    WMCHK(grow(L.part, (size_t)B * 256 * 4));
    WMCHK(grow(L.mel, (size_t)B * n_mels * F * 4));
    HIPCHK(hipMemcpyAsync(L.pcm.p, pcm, (size_t)B * stride * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(L.lens.p, n_samples, (size_t)B * 4, hipMemcpyHostToDevice, st));
    launch_zero_tails(L.pcm.as<float>(), L.lens.as<int>(), B, stride, st);  // HF pads with zeros to the longest recording
    for (int t0 = 0; t0 < F; t0 += nt) {
        const int n = std::min(nt, F - t0);
        launch_frames(L.pcm.as<float>(), L.frames.as<float>(), m->fe.window.as<float>(), B, stride, n, FE_HOP, st, t0);
        GemmParams p{};
        p.A = L.frames.p;
        p.W = m->fe.dft.p;
        p.C = L.spec.p;
        p.M = B * n;
        p.N = 512;
        p.K = 416;
        p.lda = 416;
        p.ldw = 416;
        p.ldc = 512;
        LCHK((launch_gemm_nt<float, float>(p, 1, st)));
        launch_mel_log(L.spec.as<float>(), m->fe.fb.as<float>(), m->fe.band.as<int>(), L.mel.as<float>(), B, n, n_mels, st, F, t0);
    }
    launch_mel_norm_long(L.mel.as<float>(), L.part.as<float>(), B, (size_t)n_mels * F, st);
    HIPCHK(hipGetLastError());
    if (n_frames_out)
        for (int b = 0; b < B; ++b) n_frames_out[b] = std::min((n_samples[b] + FE_HOP - 1) / FE_HOP, F);
    return 0;
}

extern "C" int wm_log_mel_long(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, float* mel_out, int32_t* n_frames_out) {
    if (!m) return fail(WM_E_ARG, "null model");
    const int rc = frontend_long_run(m, pcm, n_samples, B, stride, n_frames_out);
    if (rc) {
        (void)hipStreamSynchronize(m->stream);
        long_release(m);
        return rc;
    }
    hipError_t e = hipSuccess;
    if (mel_out)
        e = hipMemcpyAsync(mel_out, m->lf.mel.p, (size_t)B * m->cfg.dims.n_mels * (stride / FE_HOP) * 4, hipMemcpyDeviceToHost, m->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
    long_release(m);
    if (e != hipSuccess) return fail(WM_E_HIP, "wm_log_mel_long: %s", hipGetErrorString(e));
    return 0;
}

// HF WhisperGenerationMixin._prepare_decoder_input_ids for ONE utterance (wm_op_long_prompt).  seq / segs: the utterance's segments
// so far; the first-segment pseudo-segment (prompt_ids minus a leading <|startofprev|>) is entered in front of them here.
static bool long_opts_plain(const wm_long_opts* lo) { return !lo || (!lo->condition_on_prev_tokens && (!lo->prompt_ids || lo->n_prompt_ids <= 0)); }
static void long_prompt(const int32_t* seq, const wm_segment* segs, int n_segs, const int32_t* init, int n_init, const wm_long_opts* lo, int tb,
                        int n_text_ctx, std::vector<int32_t>& out) {
    out.clear();
    const bool have_prompt = lo && lo->prompt_ids && lo->n_prompt_ids > 0;
    const bool cond = lo && lo->condition_on_prev_tokens;
    const bool all_segments = lo && lo->prompt_condition_type == 1;
    const int pseudo0 = have_prompt && lo->prompt_ids[0] == lo->prev_sot_token ? 1 : 0;
    const bool pseudo = have_prompt && !all_segments;
    if (cond && (n_segs > 0 || pseudo)) {
        const int cut = n_text_ctx / 2 - 1;
        std::vector<int32_t> prev;
        auto add = [&](const int32_t* t, int n) {  // skip_ending_double_timestamps
            if (n > 2 && t[n - 2] >= tb) --n;
            prev.insert(prev.end(), t, t + n);
        };
        if (pseudo) add(lo->prompt_ids + pseudo0, lo->n_prompt_ids - pseudo0);
        for (int i = 0; i < n_segs; ++i) add(seq + segs[i].first, segs[i].count);
        if ((int)prev.size() > cut) prev.erase(prev.begin(), prev.end() - cut);
        if (have_prompt && all_segments)
            out.assign(lo->prompt_ids, lo->prompt_ids + lo->n_prompt_ids);
        else
            out.push_back(lo->prev_sot_token);
        out.insert(out.end(), prev.begin(), prev.end());
    } else if (have_prompt) {
        out.assign(lo->prompt_ids, lo->prompt_ids + lo->n_prompt_ids);
    }
    out.insert(out.end(), init, init + n_init);
}
static int long_opts_check(const wm_long_opts* lo, const int32_t* init, int n_init, int max_loop, int vocab, int n_text_ctx, int pass_rows) {
    if (lo && lo->use_no_speech_threshold) {  // HF dereferences logprob_threshold whenever no_speech_threshold is set
        if (!lo->use_logprob_threshold) return fail(WM_E_ARG, "no_speech_threshold needs logprob_threshold");
        if (lo->no_speech_token < 0 || lo->no_speech_token >= vocab) return fail(WM_E_ARG, "no_speech_token %d is not a vocabulary id", lo->no_speech_token);
    }
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold) && lo->no_speech_token != -1 &&
        (lo->no_speech_token < 0 || lo->no_speech_token >= vocab))  // (-1 with logprob_threshold alone: no probe, no_speech_prob is NaN)
        return fail(WM_E_ARG, "no_speech_token %d is neither -1 nor a vocabulary id", lo->no_speech_token);
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold) && dec_lanes_for(pass_rows) != 1)
        return fail(WM_E_ARG, "log-probabilities need a single-lane decode state");
    if (long_opts_plain(lo)) {
        if (lo && lo->prompt_condition_type == 1) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
        return 0;
    }
    (void)init;
    if (dec_lanes_for(pass_rows) != 1) return fail(WM_E_ARG, "per-row prompts need a single-lane decode state");
    const int cut = n_text_ctx / 2 - 1;
    const int np = lo->prompt_ids ? std::max(lo->n_prompt_ids, 0) : 0;
    if (lo->n_prompt_ids < 0 || (lo->n_prompt_ids > 0 && !lo->prompt_ids)) return fail(WM_E_ARG, "bad prompt_ids");
    if (lo->prompt_condition_type != 0 && lo->prompt_condition_type != 1) return fail(WM_E_ARG, "prompt_condition_type must be 0 (first-segment) or 1 (all-segments)");
    if (lo->prompt_condition_type == 1 && !lo->condition_on_prev_tokens) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
    if (lo->prev_sot_token < 0 || lo->prev_sot_token >= vocab) return fail(WM_E_ARG, "prev_sot_token %d is not a vocabulary id", lo->prev_sot_token);
    for (int i = 0; i < np; ++i)
        if (lo->prompt_ids[i] < 0 || lo->prompt_ids[i] >= vocab) return fail(WM_E_ARG, "prompt id out of range");
    if (np > cut + 1) return fail(WM_E_ARG, "n_prompt_ids %d exceeds %d (half the decoder context)", np, cut + 1);
    const int worst = lo->condition_on_prev_tokens ? ((lo->prompt_condition_type == 1 && np > 0 ? np : 1) + cut + n_init) : np + n_init;
    if (worst + 1 + max_loop > n_text_ctx)
        return fail(WM_E_ARG, "longest decoder prompt %d + 1 + max_loop %d exceeds the decoder context %d", worst, max_loop, n_text_ctx);
    return 0;
}
extern "C" int wm_op_long_prompt(const int32_t* seq, const wm_segment* segs, int n_segs, const int32_t* init, int n_init, const wm_long_opts* lo,
                                 int timestamp_begin, int n_text_ctx, int32_t* out, int32_t* n_out) {
    if (n_segs < 0 || (n_segs > 0 && (!seq || !segs)) || !init || n_init <= 0 || !out || !n_out || n_text_ctx < 4 || timestamp_begin <= 0)
        return fail(WM_E_ARG, "bad argument");
    if (lo) {
        if (lo->n_prompt_ids < 0 || (lo->n_prompt_ids > 0 && !lo->prompt_ids)) return fail(WM_E_ARG, "bad prompt_ids");
        if (lo->prompt_condition_type != 0 && lo->prompt_condition_type != 1) return fail(WM_E_ARG, "prompt_condition_type must be 0 (first-segment) or 1 (all-segments)");
        if (lo->prompt_condition_type == 1 && !lo->condition_on_prev_tokens) return fail(WM_E_ARG, "prompt_condition_type all-segments needs condition_on_prev_tokens");
        if (!long_opts_plain(lo) && lo->prev_sot_token < 0) return fail(WM_E_ARG, "prev_sot_token is required with conditioning or prompt_ids");
        if (lo->prompt_ids && lo->n_prompt_ids > n_text_ctx / 2) return fail(WM_E_ARG, "n_prompt_ids %d exceeds %d (half the decoder context)", lo->n_prompt_ids, n_text_ctx / 2);
    }
    for (int i = 0; i < n_segs; ++i)
        if (segs[i].first < 0 || segs[i].count < 0) return fail(WM_E_ARG, "bad segment %d", i);
    std::vector<int32_t> v;
    long_prompt(seq, segs, n_segs, init, n_init, lo, timestamp_begin, n_text_ctx, v);
    if ((int)v.size() > n_text_ctx) return fail(WM_E_ARG, "the prompt (%d ids) exceeds the decoder context %d", (int)v.size(), n_text_ctx);
    std::copy(v.begin(), v.end(), out);
    *n_out = (int32_t)v.size();
    return 0;
}

static int long_check(wm_model* m, const wm_decode_opts* o, int B) {
    WMCHK(check_opts(m, o, B));
    if (o->timestamp_begin <= 0) return fail(WM_E_ARG, "long-form transcription needs the timestamp rules (timestamp_begin > 0)");
    if (o->ignore_eot) return fail(WM_E_ARG, "long-form transcription stops each window at eot (ignore_eot must be 0)");
    if (o->n_prompt + 1 + o->max_loop > m->cfg.dims.n_text_ctx)
        return fail(WM_E_ARG, "n_prompt + 1 + max_loop = %d exceeds the decoder context %d", o->n_prompt + 1 + o->max_loop, m->cfg.dims.n_text_ctx);
    if (m->held.active) return fail(WM_E_STATE, "a coalesced submit is held: wait for it before long-form transcription");
    return 0;
}

// The window scheduler.  Without condition_on_prev_tokens an utterance carries nothing but seek from one window to the next, so a
// pass may take ANY pending (utterance, seek) items: passes of R = min(ceil(B / 2), max_batch) rows (short passes repeat their first
// item, so neither state is re-created within a call and the repeat finishes with its original), two in flight on m->lf.st[0..1]
// — one pass's gather + encoder and the host's segment bookkeeping overlap the other's decode.  An utterance rides one pass at a
// time: with B <= 2R the two states keep the utterances they started with, and when one state runs dry the other's tail runs
// one pass at a time.  mel: device [B][n_mels][T].
// lo (conditioning / prompt_ids): a row's decoder prompt is built from its utterance's own segments when the row is
// assigned to a pass; a pass whose rows all carry opts->prompt goes out exactly as before, any other as a per-row pass.
// lang_ids != null: HF detects once per recording, on its first window — before the loop every recording's window at
// seek 0 is gathered in groups of R rows and run through wm_detect_language's device path on state 0, the ids are read back once per
// group, and from then on recording b's initial ids are opts->prompt with slot 1 replaced by its language: every pass is a per-row pass.
static int long_run(wm_model* m, const float* mel, int T, const int32_t* nf, int B, const wm_decode_opts* o, wm_long_result* res,
                    const wm_long_opts* lo, const int32_t* lang_ids = nullptr, int n_lang = 0, int32_t* lang_out = nullptr, bool tt = false) {
    const wm_dims& c = m->cfg.dims;
    if (m->top_k > 0)  // (no entry of the long-form result carries them yet)
        return fail(WM_E_ARG, "top-k alternatives (wm_set_top_k) are not available in long-form transcription: set top_k to 0");
    const bool plain = long_opts_plain(lo) && !lang_ids;
    // thresholds: every pass is a log-prob pass; with a no_speech_token it also carries the probe at the first of the
    // o->n_prompt initial ids.  A window is skipped iff avg_logprob < logprob_threshold and no_speech_prob > no_speech_threshold.
    const bool quality = lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold);
    const NsAsk ns = quality && lo->no_speech_token >= 0 ? NsAsk{lo->no_speech_token, o->n_prompt} : NsAsk();  // (range checked up front)
    res->quality = quality;
    // half the batch per state (when it fits), so that two passes are in flight whenever two utterances are pending
    const int W = 2 * c.n_audio_ctx, R = std::min((B + 1) / 2, m->cfg.max_batch), total = plain ? o->n_prompt + 1 + o->max_loop : c.n_text_ctx;
    std::vector<int32_t> row_prompts[2], row_len[2];  // per state: the pass's prompts [R][n_text_ctx] and their lengths
    int pass_total[2] = {total, total};
    std::vector<int32_t> pr;
    wm_model::LongForm& L = m->lf;
    std::vector<int64_t> seek(B, 0);
    std::vector<char> busy(B, 0);
    std::vector<int> snf(B, 0);
    int n_items[2] = {0, 0}, order[2] = {0, 0}, ticket = 0;
    for (int k = 0; k < 2; ++k) {
        WMCHK(grow(L.win[k], (size_t)R * c.n_mels * W * 4));
        WMCHK(grow(L.items[k], (size_t)R * 3 * 4));
    }
    std::vector<int32_t> toks((size_t)R * total), cnt(R);
    std::vector<float> lps(quality ? (size_t)R * total : 0), avg(R, 0.f), nsp(R, NAN);
    std::vector<wm_segment> segs;
    PassOut out{toks.data(), cnt.data()};
    out.token_logprobs = quality ? lps.data() : nullptr;
    out.avg_logprob = quality ? avg.data() : nullptr;
    out.no_speech_prob = ns.token >= 0 ? nsp.data() : nullptr;
    // token timestamps: every window pass carries the alignment capture and the chain; per state the columns kept per
    // row (window frames / 2) and the window table the finishing kernel reads, per pass the times [R][max_loop + 1] it hands back
    const int L1 = o->max_loop + 1;
    std::vector<double> wt(tt ? (size_t)R * L1 : 0);
    std::vector<int32_t> win_cols[2];
    WinAsk win_ask[2];
    out.win_times = tt ? wt.data() : nullptr;
    res->tt = tt;
    auto collect = [&](int k) { return wait_on(m, L.st[k], 0, -1, out); };
    auto window_ask = [&](int k, const wm_decode_opts* opts) {  // a pass over state k's gathered windows
        PassAsk ask{L.win[k].as<float>(), 1, R, opts};
        ask.lp = quality;
        ask.ns = ns;
        ask.rp = m->repeat;  // every window's pass sees its own decoder ids only, carried previous text included (HF's per-window generate)
        if (tt) {
            win_cols[k].resize(R);
            for (int r = 0; r < R; ++r) win_cols[k][r] = std::max(1, L.h_items[k][3 * r + 2] / 2);
            win_ask[k] = WinAsk{L.items[k].as<int>(), n_items[k]};
            ask.cols = &win_cols[k];
            ask.win = &win_ask[k];
        }
        return ask;
    };
    auto drain = [&]() {  // an error mid-run: let the other pass finish before returning
        for (int k = 0; k < 2; ++k)
            if (n_items[k] && L.st[k] && L.st[k]->pending) (void)collect(k);
    };
    std::vector<int32_t> inits;  // language detection: [B][n_prompt] each recording's own initial ids
    if (lang_ids) {
        std::vector<int32_t>& h = L.h_items[0];
        for (int b0 = 0; b0 < B; b0 += R) {
            const int nb = std::min(R, B - b0);
            h.clear();
            for (int r = 0; r < R; ++r) {  // (spare rows repeat the group's first recording)
                const int b = b0 + (r < nb ? r : 0);
                h.insert(h.end(), {b, 0, (int32_t)std::min<int64_t>(nf[b], W)});
            }
            HIPCHK(hipMemcpyAsync(L.items[0].p, h.data(), (size_t)R * 3 * 4, hipMemcpyHostToDevice, m->stream));
            launch_window_gather(mel, L.items[0].as<int>(), L.win[0].as<float>(), R, c.n_mels, T, W, m->stream);
            HIPCHK(hipGetLastError());
            WMCHK(submit_on(m, &L.st[0], lang_only_ask(L.win[0].as<float>(), 1, R, lang_ids, n_lang, o->prompt[0])));
            HIPCHK(hipStreamSynchronize(L.st[0]->lanes[0].st));
            HIPCHK(hipMemcpy(lang_out + b0, L.st[0]->lg.out.p, (size_t)nb * 4, hipMemcpyDeviceToHost));
        }
        inits.resize((size_t)B * o->n_prompt);
        for (int b = 0; b < B; ++b) {
            std::copy(o->prompt, o->prompt + o->n_prompt, inits.begin() + (size_t)b * o->n_prompt);
            inits[(size_t)b * o->n_prompt + 1] = lang_out[b];
        }
    }
    int cursor = 0;
    for (;;) {
        for (int k = 0; k < 2; ++k) {  // fill idle states with ready utterances
            if (n_items[k]) continue;
            std::vector<int32_t>& h = L.h_items[k];
            h.clear();
            for (int i = 0; i < B && (int)h.size() < 3 * R; ++i) {
                const int b = (cursor + i) % B;
                if (busy[b] || seek[b] >= nf[b]) continue;
                snf[b] = (int)std::min<int64_t>(nf[b] - seek[b], W);
                h.insert(h.end(), {b, (int32_t)seek[b], snf[b]});
                busy[b] = 1;
            }
            if (h.empty()) continue;
            n_items[k] = (int)h.size() / 3;
            cursor = (h[3 * (n_items[k] - 1)] + 1) % B;
            for (int r = n_items[k]; r < R; ++r) h.insert(h.end(), {h[0], h[1], h[2]});
            int rc = hipMemcpyAsync(L.items[k].p, h.data(), (size_t)R * 3 * 4, hipMemcpyHostToDevice, m->stream) == hipSuccess ? 0
                     : fail(WM_E_HIP, "items upload failed");
            if (!rc) {
                launch_window_gather(mel, L.items[k].as<int>(), L.win[k].as<float>(), R, c.n_mels, T, W, m->stream);
                rc = hipGetLastError() == hipSuccess ? 0 : fail(WM_E_HIP, "window gather launch failed");
            }
            bool per_row = false;
            if (!plain) {
                row_prompts[k].assign((size_t)R * c.n_text_ctx, 0);
                row_len[k].assign(R, 0);
                for (int r = 0; r < R; ++r) {  // (spare rows repeat row 0 with its prompt)
                    const int b = h[3 * r];
                    const int32_t* init = lang_ids ? inits.data() + (size_t)b * o->n_prompt : o->prompt;  // the row's own initial ids
                    long_prompt(res->tokens[b].data(), res->segs[b].data(), (int)res->segs[b].size(), init, o->n_prompt, lo, o->timestamp_begin,
                                c.n_text_ctx, pr);
                    std::copy(pr.begin(), pr.end(), row_prompts[k].begin() + (size_t)r * c.n_text_ctx);
                    row_len[k][r] = (int32_t)pr.size();
                    per_row = per_row || lang_ids || (int)pr.size() != o->n_prompt || !std::equal(pr.begin(), pr.end(), init);
                }
            }
            row_len[k].resize(R, o->n_prompt);
            if (!per_row) {
                res->longest_prompt = std::max(res->longest_prompt, o->n_prompt);
                std::fill(row_len[k].begin(), row_len[k].end(), o->n_prompt);
                pass_total[k] = o->n_prompt + 1 + o->max_loop;
                if (!rc) rc = submit_on(m, &L.st[k], window_ask(k, o));
            } else if (!rc) {
                wm_decode_opts o2;
                RowPrompts rows;
                rc = rows_check(m, o, R, row_prompts[k].data(), row_len[k].data(), c.n_text_ctx, o2, rows);
                pass_total[k] = o2.n_prompt + 1 + o2.max_loop;
                if (!rc) {
                    res->longest_prompt = std::max(res->longest_prompt, o2.n_prompt);
                    ++res->row_passes;
                }
                if (!rc) {
                    PassAsk ask = window_ask(k, &o2);
                    ask.rows = &rows;
                    rc = submit_on(m, &L.st[k], ask);
                }
            }
            if (rc) {
                n_items[k] = 0;
                drain();
                return rc;
            }
            order[k] = ++ticket;
            ++res->passes;
            res->rows += R;
        }
        int k = -1;  // the older pass in flight
        for (int j = 0; j < 2; ++j)
            if (n_items[j] && (k < 0 || order[j] < order[k])) k = j;
        if (k < 0) break;
        const int rc = collect(k);
        const int n = n_items[k];
        n_items[k] = 0;
        if (rc) {
            drain();
            return rc;
        }
        for (int r = 0; r < n; ++r) {
            const int b = L.h_items[k][3 * r];
            const int32_t* row = toks.data() + (size_t)r * pass_total[k];
            const int n_prompt = row_len[k][r];
            int g1 = cnt[r];
            if (g1 > n_prompt && row[g1 - 1] == o->eot) --g1;  // HF drops the trailing eos
            const int g0 = std::min(n_prompt, g1);
            if (quality) {
                const bool skip = lo->use_no_speech_threshold && avg[r] < lo->logprob_threshold && nsp[r] > lo->no_speech_threshold;
                res->wins[b].push_back(wm_long_result::Window{seek[b], avg[r], nsp[r], skip ? 1 : 0});
                if (skip) {  // HF: no segments, no ids, seek += seek_num_frames (not _retrieve_segment's advance)
                    seek[b] += snf[b];
                    busy[b] = 0;
                    ++res->windows;
                    ++res->skipped;
                    continue;
                }
            }
            int adv = long_segments(row + g0, g1 - g0, o->timestamp_begin, seek[b], snf[b], segs);
            if (adv == 0) {  // the deviation: HF would decode this window again, forever
                adv = snf[b];
                ++res->stalled;
            }
            std::vector<int32_t>& seq = res->tokens[b];
            for (wm_segment sg : segs) {
                const int32_t first = (int32_t)seq.size();
                seq.insert(seq.end(), row + g0 + sg.first, row + g0 + sg.first + sg.count);
                sg.first = first;
                res->segs[b].push_back(sg);
                if (quality) {
                    res->seg_avg[b].push_back(avg[r]);
                    res->seg_nsp[b].push_back(nsp[r]);
                }
            }
            if (tt) long_slice_times(wt.data() + (size_t)r * L1, segs, res->times[b]);
            seek[b] += adv;
            busy[b] = 0;
            ++res->windows;
        }
    }
    return 0;
}

static int transcribe_long_impl(wm_model* m, const float* mel_dev, int T, const int32_t* nf, int B, const wm_decode_opts* o, wm_long_result** out,
                                const wm_long_opts* lo, const int32_t* lang_ids = nullptr, int n_lang = 0, int32_t* lang_out = nullptr,
                                bool tt = false) {
    wm_long_result* r = new wm_long_result();
    r->times.resize(B);
    r->tokens.resize(B);
    r->segs.resize(B);
    r->wins.resize(B);
    r->seg_avg.resize(B);
    r->seg_nsp.resize(B);
    const int rc = long_run(m, mel_dev, T, nf, B, o, r, lo, lang_ids, n_lang, lang_out, tt);
    (void)hipStreamSynchronize(m->stream);
    long_release(m);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return 0;
}

// the extra refusals of a long-form run with language detection; everything is refused before anything is launched
static int long_lang_check(wm_model* m, const wm_decode_opts* o, int B, const int32_t* lang_ids, int n_lang, const int32_t* lang_out) {
    if (!lang_out) return fail(WM_E_ARG, "bad argument");
    WMCHK(lang_list_check(m->cfg.dims.vocab, lang_ids, n_lang));
    if (o->n_prompt < 2) return fail(WM_E_ARG, "language detection needs at least two initial ids (<|startoftranscript|> and the language slot)");
    if (dec_lanes_for(std::min((B + 1) / 2, m->cfg.max_batch)) != 1) return fail(WM_E_ARG, "language detection needs a single-lane decode state");
    if (m->cfg.dims.n_text_ctx < o->n_prompt + 1 + o->max_loop) return fail(WM_E_ARG, "the decoder context is too short");
    return 0;
}
// the extra refusals of a long-form run with token timestamps, before anything is launched
static int long_tt_check(wm_model* m, const wm_long_opts* lo) {
    if (lo && (lo->use_logprob_threshold || lo->use_no_speech_threshold))
        return fail(WM_E_ARG, "token timestamps do not combine with logprob_threshold / no_speech_threshold");
    if (m->align_pairs.empty()) return fail(WM_E_STATE, "token timestamps need alignment heads (wm_set_alignment_heads)");
    return 0;
}
static int long_mel_impl(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* o,
                         const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, bool want_lang, wm_long_result** out,
                         bool tt = false) {
    if (!m || !mel || !out || T <= 0) return fail(WM_E_ARG, "bad argument");
    *out = nullptr;
    WMCHK(long_check(m, o, B));
    if (tt) WMCHK(long_tt_check(m, lo));
    WMCHK(long_opts_check(lo, o->prompt, o->n_prompt, o->max_loop, m->cfg.dims.vocab, m->cfg.dims.n_text_ctx, std::min((B + 1) / 2, m->cfg.max_batch)));
    if (want_lang) WMCHK(long_lang_check(m, o, B, lang_ids, n_lang, lang_out));
    std::vector<int32_t> nf(B, T);
    if (n_frames)
        for (int b = 0; b < B; ++b) {
            if (n_frames[b] < 0 || n_frames[b] > T) return fail(WM_E_ARG, "n_frames[%d] = %d outside [0, %d]", b, n_frames[b], T);
            nf[b] = n_frames[b];
        }
    HIPCHK(hipSetDevice(m->device));
    const float* dev = mel;
    if (!mel_on_device) {
        const size_t bytes = (size_t)B * m->cfg.dims.n_mels * T * 4;
        WMCHK(grow(m->lf.in_mel, bytes));
        HIPCHK(hipMemcpyAsync(m->lf.in_mel.p, mel, bytes, hipMemcpyHostToDevice, m->stream));
        dev = m->lf.in_mel.as<float>();
    }
    return transcribe_long_impl(m, dev, T, nf.data(), B, o, out, lo, want_lang ? lang_ids : nullptr, n_lang, lang_out, tt);
}
extern "C" int wm_transcribe_long_ex(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                     const wm_decode_opts* o, const wm_long_opts* lo, wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, nullptr, 0, nullptr, false, out);
}
extern "C" int wm_transcribe_long_lang(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                       const wm_decode_opts* o, const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out,
                                       wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, lang_ids, n_lang, lang_out, true, out);
}
// lang_ids null: no language detection (lang_out is not written), else as wm_transcribe_long_lang
extern "C" int wm_transcribe_long_tt(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames,
                                     const wm_decode_opts* o, const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out,
                                     int token_timestamps, wm_long_result** out) {
    return long_mel_impl(m, mel, mel_on_device, B, T, n_frames, o, lo, lang_ids, n_lang, lang_out, lang_ids != nullptr, out, token_timestamps != 0);
}
extern "C" int wm_long_result_token_times(const wm_long_result* r, int b, double* times) {
    if (!r || b < 0 || b >= (int)r->tokens.size()) return fail(WM_E_ARG, "bad argument");
    if (!r->tt) return fail(WM_E_STATE, "this run had no token timestamps (wm_transcribe_long_tt)");
    if (!times && !r->times[b].empty()) return fail(WM_E_ARG, "bad argument");
    std::copy(r->times[b].begin(), r->times[b].end(), times);
    return 0;
}
// Host only: what a timestamp window pass and the scheduler make of one window.  rel: the window-relative fp32 time of
// each of its n generated ids (trailing eot dropped), segs: wm_op_long_segments' segments of those ids -> one float64 per kept id.
extern "C" int wm_op_long_token_times(const float* rel, int n, int64_t seek, const wm_segment* segs, int n_segs, double* times, int32_t* n_times) {
    if (n < 0 || (n > 0 && !rel) || seek < 0 || n_segs < 0 || (n_segs > 0 && !segs) || !n_times) return fail(WM_E_ARG, "bad argument");
    size_t total = 0;
    for (int i = 0; i < n_segs; ++i) {
        if (segs[i].first < 0 || segs[i].count < 0 || segs[i].first + segs[i].count > n) return fail(WM_E_ARG, "segment %d outside the window's %d ids", i, n);
        total += segs[i].count;
    }
    if (total > 0 && !times) return fail(WM_E_ARG, "bad argument");
    std::vector<double> win, kept;
    long_window_times(rel, n, seek, win);
    long_slice_times(win.data(), std::vector<wm_segment>(segs, segs + n_segs), kept);
    std::copy(kept.begin(), kept.end(), times);
    *n_times = (int32_t)kept.size();
    return 0;
}

extern "C" int wm_transcribe_long(wm_model* m, const float* mel, int mel_on_device, int B, int T, const int32_t* n_frames, const wm_decode_opts* o,
                                  wm_long_result** out) {
    return wm_transcribe_long_ex(m, mel, mel_on_device, B, T, n_frames, o, nullptr, out);
}

extern "C" int wm_transcribe_long_pcm(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                      wm_long_result** out) {
    return wm_transcribe_long_pcm_ex(m, pcm, n_samples, B, stride, o, nullptr, out);
}
static int long_pcm_impl(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o, const wm_long_opts* lo,
                         const int32_t* lang_ids, int n_lang, int32_t* lang_out, bool want_lang, wm_long_result** out, bool tt = false) {
    if (!m || !out) return fail(WM_E_ARG, "bad argument");
    *out = nullptr;
    WMCHK(long_check(m, o, B));
    if (tt) WMCHK(long_tt_check(m, lo));
    WMCHK(long_opts_check(lo, o->prompt, o->n_prompt, o->max_loop, m->cfg.dims.vocab, m->cfg.dims.n_text_ctx, std::min((B + 1) / 2, m->cfg.max_batch)));
    if (want_lang) WMCHK(long_lang_check(m, o, B, lang_ids, n_lang, lang_out));
    std::vector<int32_t> nf(std::max(B, 0));
    const int rc = frontend_long_run(m, pcm, n_samples, B, stride, nf.data());  // same stream as the gathers: ordered, no host sync
    if (rc) {
        (void)hipStreamSynchronize(m->stream);
        long_release(m);
        return rc;
    }
    return transcribe_long_impl(m, m->lf.mel.as<float>(), stride / FE_HOP, nf.data(), B, o, out, lo, want_lang ? lang_ids : nullptr, n_lang, lang_out, tt);
}
extern "C" int wm_transcribe_long_pcm_ex(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                         const wm_long_opts* lo, wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, nullptr, 0, nullptr, false, out);
}
extern "C" int wm_transcribe_long_pcm_lang(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                           const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, lang_ids, n_lang, lang_out, true, out);
}
extern "C" int wm_transcribe_long_pcm_tt(wm_model* m, const float* pcm, const int32_t* n_samples, int B, int stride, const wm_decode_opts* o,
                                         const wm_long_opts* lo, const int32_t* lang_ids, int n_lang, int32_t* lang_out, int token_timestamps,
                                         wm_long_result** out) {
    return long_pcm_impl(m, pcm, n_samples, B, stride, o, lo, lang_ids, n_lang, lang_out, lang_ids != nullptr, out, token_timestamps != 0);
}

extern "C" int wm_long_result_sizes(const wm_long_result* r, int b, int32_t* n_tokens, int32_t* n_segments) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || !n_tokens || !n_segments) return fail(WM_E_ARG, "bad argument");
    *n_tokens = (int32_t)r->tokens[b].size();
    *n_segments = (int32_t)r->segs[b].size();
    return 0;
}
extern "C" int wm_long_result_get(const wm_long_result* r, int b, int32_t* tokens, wm_segment* segs) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || (!tokens && !r->tokens[b].empty()) || (!segs && !r->segs[b].empty()))
        return fail(WM_E_ARG, "bad argument");
    std::copy(r->tokens[b].begin(), r->tokens[b].end(), tokens);
    std::copy(r->segs[b].begin(), r->segs[b].end(), segs);
    return 0;
}
extern "C" int wm_long_result_stats(const wm_long_result* r, int32_t* windows, int32_t* stalled, int32_t* passes, int32_t* rows) {
    if (!r || !windows || !stalled || !passes || !rows) return fail(WM_E_ARG, "bad argument");
    *windows = r->windows;
    *stalled = r->stalled;
    *passes = r->passes;
    *rows = r->rows;
    return 0;
}
extern "C" int wm_long_result_prompt_stats(const wm_long_result* r, int32_t* longest_prompt, int32_t* row_passes) {
    if (!r || !longest_prompt || !row_passes) return fail(WM_E_ARG, "bad argument");
    *longest_prompt = r->longest_prompt;
    *row_passes = r->row_passes;
    return 0;
}
extern "C" int wm_long_result_quality(const wm_long_result* r, int b, float* seg_avg_logprob, float* seg_no_speech_prob) {
    if (!r || b < 0 || b >= (int)r->tokens.size()) return fail(WM_E_ARG, "bad argument");
    if (!r->quality) return fail(WM_E_STATE, "this run had no thresholds (wm_long_opts.use_logprob_threshold / use_no_speech_threshold)");
    if ((!seg_avg_logprob || !seg_no_speech_prob) && !r->segs[b].empty()) return fail(WM_E_ARG, "bad argument");
    std::copy(r->seg_avg[b].begin(), r->seg_avg[b].end(), seg_avg_logprob);
    std::copy(r->seg_nsp[b].begin(), r->seg_nsp[b].end(), seg_no_speech_prob);
    return 0;
}
extern "C" int wm_long_result_windows(const wm_long_result* r, int b, int32_t* n_windows, int64_t* seek, float* avg_logprob, float* no_speech_prob,
                                      int32_t* skipped) {
    if (!r || b < 0 || b >= (int)r->tokens.size() || !n_windows) return fail(WM_E_ARG, "bad argument");
    if (!r->quality) return fail(WM_E_STATE, "this run had no thresholds (wm_long_opts.use_logprob_threshold / use_no_speech_threshold)");
    const std::vector<wm_long_result::Window>& w = r->wins[b];
    *n_windows = (int32_t)w.size();
    for (size_t i = 0; i < w.size(); ++i) {
        if (seek) seek[i] = w[i].seek;
        if (avg_logprob) avg_logprob[i] = w[i].avg_logprob;
        if (no_speech_prob) no_speech_prob[i] = w[i].no_speech_prob;
        if (skipped) skipped[i] = w[i].skipped;
    }
    return 0;
}
extern "C" int wm_long_result_skip_stats(const wm_long_result* r, int32_t* skipped_windows) {
    if (!r || !skipped_windows) return fail(WM_E_ARG, "bad argument");
    *skipped_windows = r->skipped;
    return 0;
}
extern "C" void wm_long_result_free(wm_long_result* r) { delete r; }

// ---- measurement helpers ------------------------------------------------------------------------------------------------
// A freshly encoded state has an empty self-attention cache; the decode step is priced AND timed mid-sequence, at this many
// cached rows (SURVEY §8d quotes its byte figures at t = 50; the rows of a fresh cache are zero, which the timing does not care about)
static const int BENCH_STEP_LEN = 50;
extern "C" int wm_bench_bytes(wm_model* m, wm_state* s, int which, double* bytes) {
    if (!m || !s || !bytes) return fail(WM_E_ARG, "null argument");
    if (!state_is_live(s) || s->m != m) return fail(WM_E_ARG, "stale or foreign state handle");
    const wm_dims& c = m->cfg.dims;
    const double d = c.d_model, H = c.n_heads, B = s->B;
    const double ks = dt_size(m->cfg.kv_dtype), ws = dt_size(dec_dtype(m->cfg));
    // m->xattn: the cross-attention of one layer (absorb + sweep + merge, as wm_bench_kernel times it) reads X (bf16) once per
    // utterance, Wk and Wv (bf16) once, q' (three bf16 images) per row (written and read), and writes / re-reads H·d partials per key chunk
    const double x_layer = B * (double)c.n_audio_ctx * d * 2 + 2 * d * d * 2 + B * d * 4 + B * 3 * H * d * 2 * 2 +
                           B * s->nsplit * (H * d + 2 * H) * 4 * 2 + B * d * ws;
    if (which == WM_KERNEL_CROSS_ATTN) {
        // one layer: K and V rows of every utterance once + q in + partials out
        *bytes = m->xattn ? x_layer : B * 2.0 * c.n_audio_ctx * d * ks + B * d * 4 + B * s->nsplit * (d + 2 * H) * 4;
    } else if (which == WM_KERNEL_DECODE_STEP || which == WM_KERNEL_DECODE_STEP_SHARED) {
        // every weight once per step, KV once per utterance, KV write; logits are NOT materialised
        // (fused argmax: only B x ceil(V/128) (value, index) partials are written and re-read)
        const double f = c.ffn, L = c.n_layers, V = c.vocab;
        const double p_blk = 8 * d * d + 2 * f * d + (4 + 4 + 1 + 1 + 6) * d + f;  // 2 attn (4 mats each) + mlp + biases + 3 LN
        const double t = s->host_len > 0 ? s->host_len : BENCH_STEP_LEN;
        *bytes = ws * (L * (8 * d * d + 2 * f * d) + V * d) + 4 * (L * (p_blk - 8 * d * d - 2 * f * d) + 2 * d) +
                 B * L * 2 * d * ks * (c.n_audio_ctx + t) + B * L * 2 * d * ks + B * s->npart * 8.0 * 2 + B * 4;
        if (m->xattn)  // X and the bf16 Wk / Wv in place of the cross K/V cache (and the decoder-dtype Wk / Wv counted above)
            *bytes += L * (x_layer - B * 2.0 * c.n_audio_ctx * d * ks - 2 * d * d * ws);
    } else if (which == WM_KERNEL_ENCODER) {
        *bytes = 0;  // MFMA-bound: see wm_bench_flops in DESIGN.md
    } else {
        return fail(WM_E_ARG, "unknown kernel id %d", which);
    }
    return 0;
}

extern "C" int wm_bench_kernel(wm_model* m, wm_state* s, int which, int reps, float* avg_us) {
    if (!m || !s || !avg_us || reps <= 0) return fail(WM_E_ARG, "bad argument");
    WMCHK(check_state(m, s, -1));
    if (!s->has_cross) return fail(WM_E_STATE, "state has no cross K/V (call wm_encode first)");
    HIPCHK(hipSetDevice(m->device));
    hipStream_t st = m->stream;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    const int L = m->cfg.dims.n_layers;
#ifdef WM_DEV
    // phase stamps in groups of 8 (100 MHz clock): per phase the sum / max of the us after the first group's entry; returns the groups seen
    auto phase_stats = [](const std::vector<long long>& h, int nphase, double* av, double* mx) {
        long long t0 = -1;
        for (size_t g = 0; g < h.size() / 8; ++g) if (h[g * 8] > 0 && (t0 < 0 || h[g * 8] < t0)) t0 = h[g * 8];
        int n = 0;
        for (size_t g = 0; g < h.size() / 8; ++g) {
            if (h[g * 8] <= 0) continue;
            ++n;
            for (int k = 0; k < nphase; ++k) {
                const double us = (double)(h[g * 8 + k] - t0) / 100.0;
                av[k] += us;
                mx[k] = std::max(mx[k], us);
            }
        }
        return n;
    };
#endif
    if (which == WM_KERNEL_CROSS_ATTN) {
        // m->xattn: absorb + X sweep + merge / V-apply, everything that replaces attn_decode + attn_combine (wm_bench_bytes prices
        // the same three launches).  Every layer reads the SAME X (73.7 MB at B = 64), so after the first launch the stream is
        // served from the 256 MB Infinity Cache — as it is inside a decode step, where the four layers re-read it.
        const DecView v = whole_batch(m, s);
        const int TD = dec_dtype(m->cfg);
        auto one = [&](int l) -> int {
            WMCHK(launch_cross_attn(m, s, l, v, 1));
            return m->xattn ? cross_attn_merge(m, s, l, v, 1, s->dattn.p, TD) : 0;
        };
        for (int i = 0; i < L; ++i) WMCHK(one(i));  // warm-up
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) WMCHK(one(i % L));  // fp32 K/V: cycles the layers, 4 x 295 MB > 256 MB L3
        HIPCHK(hipEventRecord(e1, st));
    } else if (which == WM_KERNEL_DECODE_STEP || which == WM_KERNEL_DECODE_STEP_SHARED) {
        s->shares_chip = which == WM_KERNEL_DECODE_STEP_SHARED;  // the K/V stream as pipelined passes launch it
        // on the state's own decode stream, as the transcribe loop runs it: several states can be timed concurrently
        // from several host threads (bench.py: four chains in flight)
        const int len0 = s->host_len > 0 ? s->host_len : BENCH_STEP_LEN;  // the cache length wm_bench_bytes prices
        HIPCHK(hipStreamSynchronize(m->stream));  // wm_encode ran there
        const bool own = s->lanes.size() == 1;      // (WM_DEC_LANES > 1: whole batch on the model stream as before)
        if (own) st = s->lanes[0].st;
        const DecView v{0, s->B, st, own ? s->lanes[0].ctl : s->ctl.as<StepCtl>()};
        launch_set_step(v.ctl, len0, 1, nullptr, 0, nullptr, 0, s->B, st);
        DecPass step;  // the bare step: embeds its input, logits partials with no mask
        step.logits = Logits::partials;
        WMCHK(decode_core(m, s, v, step));
        // timed as the transcribe loop runs it: a captured graph of the step, replayed (cache length held constant)
        hipGraph_t g = nullptr;
        hipGraphExec_t ge = nullptr;
        HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        const int crc = decode_core(m, s, v, step);
        const hipError_t cap = hipStreamEndCapture(st, &g);
        if (crc) {
            if (g) (void)hipGraphDestroy(g);
            return crc;
        }
        HIPCHK(cap);
        HIPCHK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        (void)hipGraphDestroy(g);
        HIPCHK(hipGraphLaunch(ge, st));
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) HIPCHK(hipGraphLaunch(ge, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        (void)hipGraphExecDestroy(ge);
        s->shares_chip = false;
#ifdef WM_DEV
    } else if (which == 41 || which == 42) {  // developer: phase stamps of one LN1 + QKV (41) / O-proj (42) launch
        const wm_dims& c = m->cfg.dims;
        const int T = dec_dtype(m->cfg);
        DecLayer& w0 = m->dec[0];
        DevBuf dbg;
        WMCHK(dbg.alloc((size_t)4096 * 16 * 8 * 8, true));
        const DecView v = whole_batch(m, s);  // layer 0's launch as a single-position pass over the whole batch wires it
        DecLinearParams p = which == 41 ? qkv_block(m, s, v, 0, 1) : proj_residual_block(m, s, v, 1, s->dattn.as<float>(), c.d_model, w0.so_w, w0.so_b);
        launch_set_step(s->ctl.as<StepCtl>(), 10, 1, nullptr, 0, nullptr, 0, s->B, st);
        for (int i = 0; i < 3; ++i) { WMCHK(dec_linear_dispatch(T, p, st)); if (!wm_env("WM_STAMP_NO_STREAM")) WMCHK(launch_cross_attn(m, s, i, whole_batch(m, s), 1)); }
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        WMCHK(dec_linear_dispatch(T, p, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)4096 * 16 * 8);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double mx[6] = {0}, av[6] = {0};
        const int n = phase_stats(h, 6, av, mx);
        fprintf(stderr, "[wm] dec_linear %s phases (us after the first wave's entry; mean / max over %d waves): entry %.2f/%.2f  loads issued %.2f/%.2f  operands ready %.2f/%.2f  MFMA + partial stored %.2f/%.2f  after barrier %.2f/%.2f  end %.2f/%.2f\n",
                which == 41 ? "LN1+QKV" : "O-proj", n, av[0] / n, mx[0], av[1] / n, mx[1], av[2] / n, mx[2], av[3] / n, mx[3], av[4] / n, mx[4], av[5] / n, mx[5]);
        dbg.release();
    } else if (which == 43) {  // developer: phase stamps of the encoder's QKV row-panel GEMM (layer 0) on the rows of the last encode
        const wm_dims& c = m->cfg.dims;
        const int T = m->cfg.compute_dtype;
        const int M = std::min(s->B, s->Bc) * c.n_audio_ctx;
        EncLayer& w0 = m->enc[0];
        GemmParams p{};
        p.A = s->xn.p; p.W = w0.qkv_w.p; p.C = s->qkv.p; p.M = M; p.N = 3 * c.d_model; p.K = c.d_model;
        p.lda = c.d_model; p.ldw = c.d_model; p.ldc = 3 * c.d_model; p.bias = w0.qkv_b.as<float>();
        if (!gemm_nt_fuses_layernorm(T == WM_F32 ? 4 : 2, p, 1)) return fail(WM_E_ARG, "this configuration does not run the row-panel kernel");
        for (int i = 0; i < 3; ++i) WMCHK(gemm_dispatch(T, T, p, 1, st));
        DevBuf dbg;
        WMCHK(dbg.alloc((size_t)512 * 96 * 8, true));
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        WMCHK(gemm_dispatch(T, T, p, 1, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)512 * 96);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double wait = 0, issue = 0, comp = 0, epi = 0, gap = 0, unit = 0;
        int ns = 0, nu = 0, ng = 0;
        for (int g = 0; g < 512; ++g)
            for (int uu = 1; uu < 3; ++uu) {  // second and third unit of each workgroup (the first carries the panel load)
                const long long* d = &h[(size_t)g * 96 + uu * 32];
                if (d[0] <= 0 || d[25] <= 0) continue;
                for (int t = 0; t < 6; ++t) {
                    wait += (double)(d[t * 4 + 1] - d[t * 4 + 0]);
                    issue += (double)(d[t * 4 + 2] - d[t * 4 + 1]);
                    comp += (double)(d[t * 4 + 3] - d[t * 4 + 2]);
                    if (t > 0) { gap += (double)(d[t * 4] - d[t * 4 - 1]); ++ng; }
                    ++ns;
                }
                epi += (double)(d[25] - d[24]);
                unit += (double)(d[25] - d[0]);
                ++nu;
            }
        if (ns)
            fprintf(stderr, "[wm] row-panel QKV, wave 0, per 64-k stage (ns): wait + barrier %.0f  DMA issue %.0f  fragment reads + 32 MFMAs issued %.0f  to next top %.0f | "
                            "per unit: epilogue %.0f, whole unit %.0f (%d stages, %d units)\n",
                    wait / ns * 10, issue / ns * 10, comp / ns * 10, ng ? gap / ng * 10 : 0.0, epi / nu * 10, unit / nu * 10, ns, nu);
        dbg.release();
    } else if (which == 40) {  // developer: phase stamps of one logits launch (after a few warm ones), printed to stderr
        const int T = dec_dtype(m->cfg);
        DevBuf dbg;
        const int nwg = s->npart;
        WMCHK(dbg.alloc((size_t)nwg * 8 * 8 * 8, true));
        const VocabHead vh = vocab_head(m);
        DecLinearParams p = linear_block(s->dx.as<float>(), vh.ln_g, vh.ln_b, vh.emb, nullptr, vh.vocab, vh.d_model, s->B, nullptr, m->Vpad);
        p.amax_val = s->amax_val.as<float>(); p.amax_idx = s->amax_idx.as<int>(); p.amax_stride = s->npart;
        for (int i = 0; i < 3; ++i) { DISPATCH_DT(T, TT, (void)launch_dec_logits<TT>(p, st)); WMCHK(launch_cross_attn(m, s, i, whole_batch(m, s), 1)); }
        p.dbg = dbg.as<long long>();
        HIPCHK(hipEventRecord(e0, st));
        DISPATCH_DT(T, TT, (void)launch_dec_logits<TT>(p, st));
        HIPCHK(hipEventRecord(e1, st));
        HIPCHK(hipEventSynchronize(e1));
        std::vector<long long> h((size_t)nwg * 64);
        HIPCHK(hipMemcpy(h.data(), dbg.p, h.size() * 8, hipMemcpyDeviceToHost));
        double mx[8] = {0, 0, 0, 0, 0, 0, 0, 0}, av[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int n = phase_stats(h, 7, av, mx);
        fprintf(stderr, "[wm] logits phases (us after the first wave's entry; mean / max over %d waves): entry %.2f/%.2f  loads issued + staged %.2f/%.2f  after barrier %.2f/%.2f  MFMA done %.2f/%.2f  end %.2f/%.2f\n",
                n, av[0] / n, mx[0], av[1] / n, mx[1], av[2] / n, mx[2], av[3] / n, mx[3], av[4] / n, mx[4]);
        fprintf(stderr, "[wm]   gamma/beta + activations arrived (own wave) %.2f/%.2f  all waves of the workgroup %.2f/%.2f\n", av[5] / n, mx[5], av[6] / n, mx[6]);
        dbg.release();
#endif
    } else if (which == WM_KERNEL_ENCODER) {
        if (!s->last_mel) return fail(WM_E_STATE, "no mel was encoded into this state");
        WMCHK(run_encoder(m, s, s->last_mel, s->B, st, nullptr, 0, false));  // as the transcribe paths run it
        HIPCHK(hipEventRecord(e0, st));
        for (int i = 0; i < reps; ++i) WMCHK(run_encoder(m, s, s->last_mel, s->B, st, nullptr, 0, false));
        HIPCHK(hipEventRecord(e1, st));
    } else {
        return fail(WM_E_ARG, "unknown kernel id %d", which);
    }
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *avg_us = ms * 1000.0f / (float)reps;
    return 0;
}
