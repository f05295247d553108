// whisper_mi.hpp — C++ host mirror of the reference's Mojo interface, header-only, over the C-ABI of whisper_mi.h.
//
// The reference (antonvice/whisper.Mojo) is compiled Mojo; its toolchain is not in this image, so the compiled-language
// host layer is written in C++ with the reference's names, argument meaning and error behaviour:
//   WhisperConfig            whisper.mojo:9-37     (tiny() defaults)
//   Tensor                   whisper_tensor.mojo:14-60   (rows x cols fp32, row-major, owning)
//   WeightLoader(filename)   loader.mojo:5-31      (raises when the file cannot be opened)
//   Whisper / load / transcribe   whisper.mojo:169-223   (prompt 50258 50259 50359 50363, eot 50257, 195-step bound)
//   Tokenizer(path) / decode tokenizer.mojo:4-28   (bug-compatible rendering)
// Everything computes through libwhispermi.so; there is no CPU path here.  Errors become std::runtime_error carrying
// wm_last_error().  examples/main.cpp is main.mojo:11-45 written against this header.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "whisper_mi.h"

namespace whisper_mi {

inline void check(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("whisper_mi: ") + wm_last_error());
}
// the structs this header fills are WM_ABI_VERSION's: a library of another version would read tails this host never wrote
inline void check_abi() {
    if (wm_abi_version() != WM_ABI_VERSION)
        throw std::runtime_error("whisper_mi: libwhispermi.so speaks ABI version " + std::to_string(wm_abi_version()) + ", this header " +
                                 std::to_string(WM_ABI_VERSION));
}

// whisper.mojo:9-37
struct WhisperConfig {
    int d_model = 384, n_heads = 6, n_layers = 4, ffn = 1536, n_mels = 80, n_audio_ctx = 1500, n_text_ctx = 448,
        vocab_size = 51865;
    static WhisperConfig tiny() { return WhisperConfig{}; }
    static WhisperConfig base() { return WhisperConfig{512, 8, 6, 2048, 80, 1500, 448, 51865}; }
    static WhisperConfig small() { return WhisperConfig{768, 12, 12, 3072, 80, 1500, 448, 51865}; }
    static WhisperConfig medium() { return WhisperConfig{1024, 16, 24, 4096, 80, 1500, 448, 51865}; }
    static WhisperConfig micro() { return WhisperConfig{128, 2, 2, 512, 16, 100, 64, 1000}; }  // test-size model
    wm_dims dims() const { return wm_dims{d_model, n_heads, n_layers, ffn, n_mels, n_audio_ctx, n_text_ctx, vocab_size}; }
    int n_frames() const { return 2 * n_audio_ctx; }
    size_t weight_count() const {
        const wm_dims d = dims();
        return wm_weight_count(&d);
    }
};

// whisper_tensor.mojo:14-60 — just the owning rows x cols buffer the call surface passes around
struct Tensor {
    int rows = 0, cols = 0;
    std::vector<float> data;
    Tensor() = default;
    Tensor(int r, int c) : rows(r), cols(c), data((size_t)r * c, 0.f) {}
    float* ptr() { return data.data(); }
    const float* ptr() const { return data.data(); }
    size_t size() const { return data.size(); }
};

// loader.mojo:5-31: the constructor raises if the file cannot be opened; the library validates the size against the
// config at load (the reference silently reads past the end, loader.mojo:21-27)
class WeightLoader {
public:
    explicit WeightLoader(const std::string& filename) : filename_(filename) {
        std::ifstream f(filename, std::ios::binary);
        if (!f) throw std::runtime_error("WeightLoader: cannot open " + filename);
    }
    const std::string& filename() const { return filename_; }

private:
    std::string filename_;
};

// whisper.mojo:169-223
class Whisper {
public:
    static constexpr int32_t PROMPT[4] = {50258, 50259, 50359, 50363};  // whisper.mojo:187-191
    static constexpr int32_t EOT = 50257;                                // whisper.mojo:206
    static constexpr int MAX_LOOP = 195;                                 // whisper.mojo:205

    explicit Whisper(const WhisperConfig& cfg = WhisperConfig::tiny(), int compute_dtype = WM_F32, int kv_dtype = -1,
                     int max_batch = 1, int device = 0, int coalesce = 0)
        : cfg_(cfg), device_(device) {
        wcfg_.dims = cfg.dims();
        wcfg_.gelu_mode = WM_GELU_TANH;  // whisper_tensor.mojo:288-308
        wcfg_.compute_dtype = compute_dtype;
        wcfg_.kv_dtype = kv_dtype < 0 ? compute_dtype : kv_dtype;
        wcfg_.max_batch = max_batch;
        wcfg_.coalesce = coalesce;  // 2: consecutive transcribe_submit calls share one 2·B-row decode state (wm_config.coalesce)
    }
    Whisper(const Whisper&) = delete;
    Whisper& operator=(const Whisper&) = delete;
    ~Whisper() {
        if (model_) wm_model_free(model_);
    }

    // whisper.load(loader)  (whisper.mojo:180-182, main.mojo:16-17)
    void load(const WeightLoader& loader) {
        check_abi();
        if (model_) wm_model_free(model_), model_ = nullptr, top_k_ = 0;
        check(wm_model_load(loader.filename().c_str(), &wcfg_, device_, &model_));
    }
    // weights already in memory (flat fp32, the file's order)
    void load(const float* weights, size_t n_floats) {
        check_abi();
        if (model_) wm_model_free(model_), model_ = nullptr, top_k_ = 0;
        check(wm_model_load_memory(weights, n_floats, &wcfg_, device_, &model_));
    }

    // whisper.transcribe(mel) -> List[Int]  (whisper.mojo:184-223): prompt + generated ids (+ eot when hit)
    std::vector<int> transcribe(const Tensor& mel, int max_loop = MAX_LOOP) const {
        if (mel.rows != cfg_.n_mels || mel.cols != cfg_.n_frames()) throw std::runtime_error("transcribe: mel must be n_mels x 2*n_audio_ctx");
        return transcribe_batch(mel.ptr(), 1, max_loop)[0];
    }
    // B utterances, host mels [B][n_mels][n_frames]
    std::vector<std::vector<int>> transcribe_batch(const float* mels, int B, int max_loop = MAX_LOOP, bool ignore_eot = false) const {
        need_model();
        wm_decode_opts o = opts(max_loop, ignore_eot);
        const int stride = o.n_prompt + 1 + max_loop;
        std::vector<int32_t> toks((size_t)B * stride), n(B);
        check(wm_transcribe(model_, mels, 0, B, &o, toks.data(), n.data()));
        return unpack(toks, n, B, stride);
    }
    // pipelined form: submit on slot 0..7, wait later (four in flight is the optimum; see whisper_mi.h)
    void transcribe_submit(const float* mels, int B, int slot, int max_loop = MAX_LOOP, bool ignore_eot = false) {
        need_model();
        wm_decode_opts o = opts(max_loop, ignore_eot);
        check(wm_transcribe_submit(model_, slot, mels, 0, B, &o));
        pend_[slot] = {B, o.n_prompt + 1 + max_loop};
    }
    std::vector<std::vector<int>> transcribe_wait(int slot) {
        need_model();
        const auto [B, stride] = pend_[slot];
        std::vector<int32_t> toks((size_t)B * stride), n(B);
        check(wm_transcribe_wait(model_, slot, toks.data(), n.data()));
        return unpack(toks, n, B, stride);
    }
    // token-level timestamps (HF return_token_timestamps): (layer, head) alignment heads; none = off
    void set_alignment_heads(const std::vector<std::pair<int, int>>& pairs) {
        need_model();
        std::vector<int32_t> flat;
        for (const auto& [l, h] : pairs) flat.insert(flat.end(), {l, h});
        check(wm_set_alignment_heads(model_, flat.data(), (int)pairs.size()));
    }
    // ids and, per id, the time it was spoken (seconds); n_frames: mel frames of real audio per utterance, empty = whole window
    std::vector<std::vector<int>> transcribe_batch_tt(const float* mels, int B, std::vector<std::vector<float>>& times, int max_loop = MAX_LOOP,
                                                      const std::vector<int32_t>& n_frames = {}) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        const int stride = o.n_prompt + 1 + max_loop;
        std::vector<int32_t> toks((size_t)B * stride), n(B);
        std::vector<float> t((size_t)B * stride);
        check(wm_transcribe_tt(model_, mels, 0, B, &o, n_frames.empty() ? nullptr : n_frames.data(), toks.data(), n.data(), t.data()));
        times.assign(B, {});
        for (int b = 0; b < B; ++b) times[b].assign(t.begin() + (size_t)b * stride, t.begin() + (size_t)b * stride + n[b]);
        return unpack(toks, n, B, stride);
    }
    // ids and, per id, its log-probability (0 at the prompt positions); avg_logprob per utterance.  prompts: one decoder
    // prompt per utterance (empty = the model's shared prompt)
    std::vector<std::vector<int>> transcribe_batch_lp(const float* mels, int B, std::vector<std::vector<float>>& token_logprobs,
                                                      std::vector<float>& avg_logprob, int max_loop = MAX_LOOP,
                                                      const std::vector<std::vector<int32_t>>& prompts = {}) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        int lmax = 0;
        for (const auto& r : prompts) lmax = std::max(lmax, (int)r.size());
        std::vector<int32_t> tab((size_t)B * std::max(lmax, 1)), len(B);
        for (size_t b = 0; b < prompts.size() && b < (size_t)B; ++b) {
            len[b] = (int32_t)prompts[b].size();
            std::copy(prompts[b].begin(), prompts[b].end(), tab.begin() + b * lmax);
        }
        const bool rows = !prompts.empty();
        const int stride = (rows ? lmax : o.n_prompt) + 1 + max_loop;
        std::vector<int32_t> toks((size_t)B * stride), n(B);
        std::vector<float> lp((size_t)B * stride);
        avg_logprob.assign(B, 0.f);
        check(wm_transcribe_lp(model_, mels, 0, B, &o, rows ? tab.data() : nullptr, rows ? len.data() : nullptr, lmax, toks.data(), n.data(),
                               lp.data(), avg_logprob.data()));
        token_logprobs.assign(B, {});
        for (int b = 0; b < B; ++b) token_logprobs[b].assign(lp.begin() + (size_t)b * stride, lp.begin() + (size_t)b * stride + n[b]);
        return unpack(toks, n, B, stride);
    }
    // transcribe_batch_lp plus openai-whisper's no_speech_prob per utterance: the probability of no_speech_token under the
    // raw logits at each row's <|startoftranscript|> position, prompt length - n_init (n_init <= 0: the shared prompt's length)
    std::vector<std::vector<int>> transcribe_batch_lp_ns(const float* mels, int B, int32_t no_speech_token, std::vector<std::vector<float>>& token_logprobs,
                                                         std::vector<float>& avg_logprob, std::vector<float>& no_speech_prob, int max_loop = MAX_LOOP,
                                                         const std::vector<std::vector<int32_t>>& prompts = {}, int n_init = 0) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        int lmax = 0;
        for (const auto& r : prompts) lmax = std::max(lmax, (int)r.size());
        std::vector<int32_t> tab((size_t)B * std::max(lmax, 1)), len(B);
        for (size_t b = 0; b < prompts.size() && b < (size_t)B; ++b) {
            len[b] = (int32_t)prompts[b].size();
            std::copy(prompts[b].begin(), prompts[b].end(), tab.begin() + b * lmax);
        }
        const bool rows = !prompts.empty();
        const int stride = (rows ? lmax : o.n_prompt) + 1 + max_loop;
        std::vector<int32_t> toks((size_t)B * stride), n(B);
        std::vector<float> lp((size_t)B * stride);
        avg_logprob.assign(B, 0.f);
        no_speech_prob.assign(B, 0.f);
        check(wm_transcribe_lp_ns(model_, mels, 0, B, &o, rows ? tab.data() : nullptr, rows ? len.data() : nullptr, lmax, no_speech_token,
                                  n_init > 0 ? n_init : o.n_prompt, toks.data(), n.data(), lp.data(), avg_logprob.data(), no_speech_prob.data()));
        token_logprobs.assign(B, {});
        for (int b = 0; b < B; ++b) token_logprobs[b].assign(lp.begin() + (size_t)b * stride, lp.begin() + (size_t)b * stride + n[b]);
        return unpack(toks, n, B, stride);
    }
    // How likely is this transcript for this audio (wm_score): ids[b] = the decoder prompt followed by the hypothesis (a
    // trailing eot included if it is to be scored); context_len: per row (empty = 1) how many leading ids are context — reported, not
    // summed.  Returns per row the log-probability of every id (0 at t = 0) over the raw logits; sum_logprob / avg_logprob [B] over
    // t >= context_len (avg = -HF loss with labels = -100 on the context); top_ids (optional): the arg-max id per position, lowest id
    // on ties, -1 at t = 0.  Positions as this mirror's passes (WM_POS_REF).
    struct ScoreResult {
        std::vector<std::vector<float>> token_logprobs;
        std::vector<float> sum_logprob, avg_logprob;
        std::vector<std::vector<int32_t>> top_ids;  // want_top_ids
    };
    ScoreResult score(const float* mels, int B, const std::vector<std::vector<int32_t>>& ids, const std::vector<int32_t>& context_len = {},
                      bool want_top_ids = false) const {
        need_model();
        if ((int)ids.size() != B || (!context_len.empty() && (int)context_len.size() != B)) throw std::runtime_error("score: one id row (and context_len) per clip");
        int stride = 2;
        for (const auto& r : ids) stride = std::max(stride, (int)r.size());
        std::vector<int32_t> tab((size_t)B * stride), len(B), top((size_t)B * stride);
        for (int b = 0; b < B; ++b) {
            len[b] = (int32_t)ids[b].size();
            std::copy(ids[b].begin(), ids[b].end(), tab.begin() + (size_t)b * stride);
        }
        std::vector<float> lp((size_t)B * stride);
        ScoreResult r;
        r.sum_logprob.assign(B, 0.f);
        r.avg_logprob.assign(B, 0.f);
        check(wm_score(model_, mels, 0, B, WM_POS_REF, tab.data(), len.data(), stride, context_len.empty() ? nullptr : context_len.data(), lp.data(),
                       want_top_ids ? top.data() : nullptr, r.sum_logprob.data(), r.avg_logprob.data()));
        r.token_logprobs.assign(B, {});
        if (want_top_ids) r.top_ids.assign(B, {});
        for (int b = 0; b < B; ++b) {
            r.token_logprobs[b].assign(lp.begin() + (size_t)b * stride, lp.begin() + (size_t)b * stride + len[b]);
            if (want_top_ids) r.top_ids[b].assign(top.begin() + (size_t)b * stride, top.begin() + (size_t)b * stride + len[b]);
        }
        return r;
    }
    // Several candidate transcripts per clip on one encoder run (wm_score_nbest): candidates[u] = clip u's id rows, each as
    // a row of score(); context_len: per candidate ROW, clip by clip (empty = 1).  Rows are flattened clip by clip; rows, order and
    // posterior of clip u are entries [row0[u], row0[u] + n_cand[u]) of the flat results.  order: candidate indices by sum_logprob
    // (normalize: avg_logprob) descending, equal keys lower index first; best[u] = the first of them; posterior: softmax of the keys
    // over the clip's candidates.
    struct NbestResult {
        ScoreResult rows;  // per candidate row, as score() on the clip's mel repeated
        std::vector<int32_t> n_cand, row0, order, best;
        std::vector<float> posterior;
    };
    // The flat table of an n-best call, built on the host alone (tests/cpp/nbest_check.cpp): rows clip by clip, zero-padded to the
    // longest; throws std::invalid_argument on a wrong clip count, an empty clip or a wrong number of context lengths.
    struct NbestTable {
        int R = 0, stride = 2;
        std::vector<int32_t> tab, len, n_cand, row0, utt_of;
    };
    static NbestTable nbest_table(int U, const std::vector<std::vector<std::vector<int32_t>>>& candidates, const std::vector<int32_t>& context_len) {
        if (U < 1 || (int)candidates.size() != U) throw std::invalid_argument("score_candidates: one candidate list per clip");
        NbestTable t;
        for (int u = 0; u < U; ++u) {
            const auto& c = candidates[u];
            if (c.empty()) throw std::invalid_argument("score_candidates: every clip needs at least one candidate");
            t.row0.push_back(t.R);
            t.n_cand.push_back((int32_t)c.size());
            t.R += (int)c.size();
            for (const auto& row : c) {
                t.stride = std::max(t.stride, (int)row.size());
                t.utt_of.push_back(u);
            }
        }
        if (!context_len.empty() && (int)context_len.size() != t.R) throw std::invalid_argument("score_candidates: one context_len per candidate row");
        t.tab.assign((size_t)t.R * t.stride, 0);
        for (const auto& c : candidates)
            for (const auto& row : c) {
                std::copy(row.begin(), row.end(), t.tab.begin() + t.len.size() * (size_t)t.stride);
                t.len.push_back((int32_t)row.size());
            }
        return t;
    }
    NbestResult score_candidates(const float* mels, int U, const std::vector<std::vector<std::vector<int32_t>>>& candidates,
                                 const std::vector<int32_t>& context_len = {}, bool normalize = false, bool want_top_ids = false) const {
        need_model();
        const NbestTable t = nbest_table(U, candidates, context_len);
        const int R = t.R, stride = t.stride;
        const std::vector<int32_t>&tab = t.tab, &len = t.len;
        std::vector<int32_t> top((size_t)R * stride);
        NbestResult r;
        r.n_cand = t.n_cand;
        r.row0 = t.row0;
        std::vector<float> lp((size_t)R * stride);
        r.rows.sum_logprob.assign(R, 0.f);
        r.rows.avg_logprob.assign(R, 0.f);
        r.order.assign(R, -1);
        r.best.assign(U, -1);
        r.posterior.assign(R, 0.f);
        check(wm_score_nbest(model_, mels, 0, U, r.n_cand.data(), normalize ? 1 : 0, WM_POS_REF, tab.data(), len.data(), stride,
                             context_len.empty() ? nullptr : context_len.data(), lp.data(), want_top_ids ? top.data() : nullptr,
                             r.rows.sum_logprob.data(), r.rows.avg_logprob.data(), r.order.data(), r.best.data(), r.posterior.data()));
        r.rows.token_logprobs.assign(R, {});
        if (want_top_ids) r.rows.top_ids.assign(R, {});
        for (int b = 0; b < R; ++b) {
            r.rows.token_logprobs[b].assign(lp.begin() + (size_t)b * stride, lp.begin() + (size_t)b * stride + len[b]);
            if (want_top_ids) r.rows.top_ids[b].assign(top.begin() + (size_t)b * stride, top.begin() + (size_t)b * stride + len[b]);
        }
        return r;
    }
    // When each id of a given transcript was spoken (wm_align): ids / context_len as score(); n_frames: per row the mel frames
    // of real audio (empty = the whole window).  Returns per row one time per id: 0 for the context, then HF's _extract_token_timestamps
    // over the teacher-forced cross-attentions.  scores (optional): what score() returns for the same inputs, from the same pass.
    std::vector<std::vector<float>> align(const float* mels, int B, const std::vector<std::vector<int32_t>>& ids,
                                          const std::vector<int32_t>& context_len = {}, const std::vector<int32_t>& n_frames = {},
                                          ScoreResult* scores = nullptr) const {
        need_model();
        if ((int)ids.size() != B || (!context_len.empty() && (int)context_len.size() != B) || (!n_frames.empty() && (int)n_frames.size() != B))
            throw std::runtime_error("align: one id row (and context_len, n_frames) per clip");
        int stride = 2;
        for (const auto& r : ids) stride = std::max(stride, (int)r.size());
        std::vector<int32_t> tab((size_t)B * stride), len(B);
        for (int b = 0; b < B; ++b) {
            len[b] = (int32_t)ids[b].size();
            std::copy(ids[b].begin(), ids[b].end(), tab.begin() + (size_t)b * stride);
        }
        std::vector<float> tm((size_t)B * stride), lp(scores ? (size_t)B * stride : 0);
        if (scores) {
            scores->sum_logprob.assign(B, 0.f);
            scores->avg_logprob.assign(B, 0.f);
        }
        check(wm_align(model_, mels, 0, B, WM_POS_REF, tab.data(), len.data(), stride, context_len.empty() ? nullptr : context_len.data(),
                       n_frames.empty() ? nullptr : n_frames.data(), tm.data(), scores ? lp.data() : nullptr,
                       scores ? scores->sum_logprob.data() : nullptr, scores ? scores->avg_logprob.data() : nullptr));
        std::vector<std::vector<float>> times(B);
        if (scores) scores->token_logprobs.assign(B, {});
        for (int b = 0; b < B; ++b) {
            times[b].assign(tm.begin() + (size_t)b * stride, tm.begin() + (size_t)b * stride + len[b]);
            if (scores) scores->token_logprobs[b].assign(lp.begin() + (size_t)b * stride, lp.begin() + (size_t)b * stride + len[b]);
        }
        return times;
    }
    // openai-whisper's detect_language: per utterance the id of lang_ids with the largest logit after a decoder pass over
    // [sot] alone; probs (optional): [B][lang_ids.size()] softmax over the list, in list order
    std::vector<int32_t> detect_language(const float* mels, int B, const std::vector<int32_t>& lang_ids, int32_t sot,
                                         std::vector<float>* probs = nullptr) const {
        need_model();
        std::vector<int32_t> out(B);
        if (probs) probs->assign((size_t)B * lang_ids.size(), 0.f);
        check(wm_detect_language(model_, mels, 0, B, sot, lang_ids.data(), (int)lang_ids.size(), out.data(), probs ? probs->data() : nullptr));
        return out;
    }
    // transcribe_batch with the language detected on the device inside the same pass (HF generate's language = None): the
    // second of every row's n_init initial ids is overwritten with the row's detected id (returned in res.lang and in the id lists).
    // prompts: one decoder prompt per utterance (empty = the model's shared prompt; n_init <= 0: its length).  want_logprobs and
    // no_speech_token >= 0 (needs want_logprobs) add §17's and §18's values.
    struct LangResult {
        std::vector<std::vector<int>> ids;
        std::vector<int32_t> lang;                       // [B]
        std::vector<float> lang_probs;                   // [B][n_lang], list order
        std::vector<std::vector<float>> token_logprobs;  // want_logprobs
        std::vector<float> avg_logprob, no_speech_prob;
    };
    LangResult transcribe_batch_lang(const float* mels, int B, const std::vector<int32_t>& lang_ids, int max_loop = MAX_LOOP,
                                     const std::vector<std::vector<int32_t>>& prompts = {}, int n_init = 0, bool want_logprobs = false,
                                     int32_t no_speech_token = -1) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        std::vector<int32_t> tab, len;
        const int lmax = prompt_table(prompts, B, tab, len);
        const bool rows = !prompts.empty();
        const int stride = (rows ? lmax : o.n_prompt) + 1 + max_loop;
        LangSlot q{B, stride, (int)lang_ids.size(), want_logprobs, no_speech_token >= 0};
        return lang_collect(q, [&](int32_t* t, int32_t* n, float* lp, float* avg, float* nsp, int32_t* lo, float* pr) {
            return wm_transcribe_lang(model_, mels, 0, B, &o, rows ? tab.data() : nullptr, rows ? len.data() : nullptr, lmax, no_speech_token,
                                      n_init > 0 ? n_init : o.n_prompt, lang_ids.data(), (int)lang_ids.size(), t, n, lp, avg, nsp, lo, pr);
        });
    }
    // pipelined form of transcribe_batch_lang: submit on slot 0..7, collect with transcribe_wait_lang
    void transcribe_submit_lang(const float* mels, int B, int slot, const std::vector<int32_t>& lang_ids, int max_loop = MAX_LOOP,
                                const std::vector<std::vector<int32_t>>& prompts = {}, int n_init = 0, bool want_logprobs = false,
                                int32_t no_speech_token = -1) {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        std::vector<int32_t> tab, len;
        const int lmax = prompt_table(prompts, B, tab, len);
        const bool rows = !prompts.empty();
        check(wm_transcribe_submit_lang(model_, slot, mels, 0, B, &o, rows ? tab.data() : nullptr, rows ? len.data() : nullptr, lmax, no_speech_token,
                                        n_init > 0 ? n_init : o.n_prompt, lang_ids.data(), (int)lang_ids.size(), want_logprobs ? 1 : 0));
        lang_pend_[slot] = LangSlot{B, (rows ? lmax : o.n_prompt) + 1 + max_loop, (int)lang_ids.size(), want_logprobs, no_speech_token >= 0};
    }
    LangResult transcribe_wait_lang(int slot) {
        need_model();
        return lang_collect(lang_pend_[slot], [&](int32_t* t, int32_t* n, float* lp, float* avg, float* nsp, int32_t* lo, float* pr) {
            return wm_transcribe_wait_lang(model_, slot, t, n, lp, avg, nsp, lo, pr);
        });
    }
    // sequential long-form transcription (HF generate's long-form path; needs set_timestamps): host mels
    // [B][n_mels][T], n_frames per utterance (empty = T) -> per utterance the sequence and its segments
    struct LongSegment {
        double start, end;
        std::vector<int> tokens;
        float avg_logprob = 0.f, no_speech_prob = 0.f;  // the segment's window values; filled with LongThresholds only
        std::vector<double> token_timestamps{};         // seconds, one per id of `tokens`; filled with token_timestamps only
    };
    struct LongWindow {  // one decoded window of an utterance, skipped ones included (LongThresholds only)
        int64_t seek;
        float avg_logprob, no_speech_prob;
        bool skipped;
    };
    struct LongResult {
        std::vector<int> sequence;
        std::vector<LongSegment> segments;
        std::vector<LongWindow> windows;
        std::vector<double> token_times;  // seconds, one per id of `sequence`; filled with token_timestamps only
    };
    // HF generate's logprob_threshold / no_speech_threshold at temperature 0: a window with avg_logprob < logprob_threshold
    // and no_speech_prob > no_speech_threshold is skipped.  no_speech_threshold needs logprob_threshold and the <|nospeech|> id.
    struct LongThresholds {
        bool use_logprob_threshold = false;
        float logprob_threshold = 0.f;
        bool use_no_speech_threshold = false;
        float no_speech_threshold = 0.f;
        int32_t no_speech_token = -1;
    };
    // condition_on_prev_tokens / prompt_ids (as WhisperProcessor.get_prompt_ids returns them) / all_segments: HF generate's options of
    // the same names; the defaults are wm_transcribe_long.  token_timestamps (needs set_alignment_heads, not
    // with thresholds): the time of every id, per utterance and per segment
    std::vector<LongResult> transcribe_long(const float* mels, int B, int T, const std::vector<int32_t>& n_frames = {}, int max_loop = MAX_LOOP,
                                            bool condition_on_prev_tokens = false, const std::vector<int32_t>& prompt_ids = {},
                                            bool all_segments = false, int32_t prev_sot_token = 50361, const LongThresholds* thresholds = nullptr,
                                            const std::vector<int32_t>& lang_ids = {}, std::vector<int32_t>* lang_out = nullptr,
                                            bool token_timestamps = false) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        wm_long_result* r = nullptr;
        LongThresholds th;
        if (thresholds) th = *thresholds;
        const wm_long_opts lo{condition_on_prev_tokens ? 1 : 0, prev_sot_token, prompt_ids.empty() ? nullptr : prompt_ids.data(),
                              (int)prompt_ids.size(), all_segments ? 1 : 0, th.use_logprob_threshold ? 1 : 0, th.logprob_threshold,
                              th.use_no_speech_threshold ? 1 : 0, th.no_speech_threshold, th.no_speech_token};
        const bool quality = th.use_logprob_threshold || th.use_no_speech_threshold;
        if (token_timestamps) {
            std::vector<int32_t> lang(B);
            check(wm_transcribe_long_tt(model_, mels, 0, B, T, n_frames.empty() ? nullptr : n_frames.data(), &o, &lo,
                                        lang_ids.empty() ? nullptr : lang_ids.data(), (int)lang_ids.size(), lang.data(), 1, &r));
            if (lang_out && !lang_ids.empty()) *lang_out = lang;
        } else if (!lang_ids.empty()) {  // HF generate's language = None: each recording's language, detected on its first window
            std::vector<int32_t> lang(B);
            check(wm_transcribe_long_lang(model_, mels, 0, B, T, n_frames.empty() ? nullptr : n_frames.data(), &o, &lo, lang_ids.data(),
                                          (int)lang_ids.size(), lang.data(), &r));
            if (lang_out) *lang_out = lang;
        } else {
            check(wm_transcribe_long_ex(model_, mels, 0, B, T, n_frames.empty() ? nullptr : n_frames.data(), &o, &lo, &r));
        }
        std::vector<LongResult> out(B);
        int rc = 0;
        for (int b = 0; b < B && !rc; ++b) {
            int32_t nt = 0, ns = 0;
            rc = wm_long_result_sizes(r, b, &nt, &ns);
            std::vector<int32_t> ids(nt);
            std::vector<wm_segment> segs(ns);
            if (!rc) rc = wm_long_result_get(r, b, ids.data(), segs.data());
            out[b].sequence.assign(ids.begin(), ids.end());
            for (const wm_segment& sg : segs)
                out[b].segments.push_back({sg.start, sg.end, std::vector<int>(ids.begin() + sg.first, ids.begin() + sg.first + sg.count)});
            if (token_timestamps && !rc) {
                out[b].token_times.resize(nt);
                rc = wm_long_result_token_times(r, b, out[b].token_times.data());
                for (int i = 0; i < ns && !rc; ++i)
                    out[b].segments[i].token_timestamps.assign(out[b].token_times.begin() + segs[i].first,
                                                               out[b].token_times.begin() + segs[i].first + segs[i].count);
            }
            if (quality && !rc) {
                std::vector<float> qa(ns), qn(ns);
                rc = wm_long_result_quality(r, b, qa.data(), qn.data());
                for (int i = 0; i < ns && !rc; ++i) {
                    out[b].segments[i].avg_logprob = qa[i];
                    out[b].segments[i].no_speech_prob = qn[i];
                }
                int32_t nw = 0;
                if (!rc) rc = wm_long_result_windows(r, b, &nw, nullptr, nullptr, nullptr, nullptr);
                std::vector<int64_t> ws(nw);
                std::vector<float> wa(nw), wn(nw);
                std::vector<int32_t> wk(nw);
                if (!rc) rc = wm_long_result_windows(r, b, &nw, ws.data(), wa.data(), wn.data(), wk.data());
                for (int i = 0; i < nw && !rc; ++i) out[b].windows.push_back({ws[i], wa[i], wn[i], wk[i] != 0});
            }
        }
        wm_long_result_free(r);
        check(rc);
        return out;
    }
    // PCM at any sample rate, float (WM_F32) or int16_t (WM_I16, scaled by 1 / 32768), [B][stride] on the host with n_samples per row
    // -> one float vector at 16 kHz per row, resampled on the GPU as torchaudio.functional.resample defines it: what every
    // PCM entry above takes.  frontend.resample of the Python package.
    std::vector<std::vector<float>> resample(const void* pcm, int in_dtype, const std::vector<int32_t>& n_samples, int64_t stride, int sampling_rate) const {
        const int B = (int)n_samples.size();
        int64_t longest = 1;
        for (int32_t n : n_samples) {
            int64_t v = 0;
            check(wm_resample_len(n, sampling_rate, &v));
            longest = v > longest ? v : longest;
        }
        std::vector<float> out((size_t)(B > 0 ? B : 1) * longest);
        std::vector<int32_t> n_out(B > 0 ? B : 1);
        check(wm_resample_pcm(model_, pcm, in_dtype, 0, n_samples.data(), B, stride, sampling_rate, out.data(), 0, longest, n_out.data()));
        std::vector<std::vector<float>> rows(B);
        for (int b = 0; b < B; ++b) rows[b].assign(out.begin() + (size_t)b * longest, out.begin() + (size_t)b * longest + n_out[b]);
        return rows;
    }
    // chunked long-form transcription (HF's ASR pipeline with chunk_length_s / stride_length_s): PCM [R][stride] at
    // 16 kHz on the host, or (pcm_on_device) on the model's GPU, n_samples per recording; chunk_len / stride_left / stride_right in samples (strides < 0: chunk_len / 6).  Every chunk is
    // decoded on its own in passes of max_batch rows; `sequence` is the recording's stitched ids, `chunks` (want_chunks) every chunk
    // with its own ids.  lang_ids: every chunk's language is detected in its pass.
    struct Chunk {
        int32_t start, len, stride_left, stride_right;  // samples
        std::vector<int> tokens;
    };
    struct ChunkedResult {
        std::vector<int> sequence;
        std::vector<Chunk> chunks;
    };
    std::vector<ChunkedResult> transcribe_chunked(const float* pcm, const std::vector<int32_t>& n_samples, int stride, int chunk_len = 480000,
                                                  int stride_left = -1, int stride_right = -1, bool want_chunks = false, int max_loop = MAX_LOOP,
                                                  const std::vector<int32_t>& lang_ids = {}, int32_t first_special = 50257,
                                                  bool pcm_on_device = false) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        const int R = (int)n_samples.size(), sl = stride_left < 0 ? chunk_len / 6 : stride_left, sr = stride_right < 0 ? chunk_len / 6 : stride_right;
        int32_t n = 0;
        check(wm_chunk_table(n_samples.data(), R, chunk_len, sl, sr, 0, nullptr, 0, &n));
        std::vector<int32_t> tab((size_t)(n > 0 ? n : 1) * 6);
        check(wm_chunk_table(n_samples.data(), R, chunk_len, sl, sr, 0, tab.data(), n, &n));
        std::vector<int> per(R, 0);
        for (int k = 0; k < n; ++k) ++per[tab[(size_t)k * 6]];
        const int total = o.n_prompt + 1 + max_loop;
        int cap = 1;
        for (int v : per) cap = v * total > cap ? v * total : cap;
        std::vector<int32_t> merged((size_t)R * cap), mlen(R), cids(want_chunks ? (size_t)(n > 0 ? n : 1) * total : 0), cn(want_chunks ? (n > 0 ? n : 1) : 0);
        check(wm_transcribe_chunked(model_, pcm, pcm_on_device ? 1 : 0, n_samples.data(), R, stride, chunk_len, sl, sr, &o, lang_ids.empty() ? nullptr : lang_ids.data(),
                                    (int)lang_ids.size(), first_special, merged.data(), mlen.data(), cap, want_chunks ? cids.data() : nullptr,
                                    want_chunks ? cn.data() : nullptr, nullptr));
        std::vector<ChunkedResult> out(R);
        for (int r = 0; r < R; ++r) out[r].sequence.assign(merged.begin() + (size_t)r * cap, merged.begin() + (size_t)r * cap + mlen[r]);
        for (int k = 0; want_chunks && k < n; ++k) {
            const int32_t* t = &tab[(size_t)k * 6];
            out[t[0]].chunks.push_back({t[1], t[2], t[3], t[4], std::vector<int>(cids.begin() + (size_t)k * total, cids.begin() + (size_t)k * total + cn[k])});
        }
        return out;
    }
    // ... with timestamps (set_timestamps first): HF's return_timestamps = true (word = false) or "word" (word = true, needs
    // alignment heads).  `segments`: start / end in seconds (end NaN: no ending timestamp), the ids and, in word mode, the (start, end)
    // of every id; `sequence` is the segments' ids concatenated.
    struct ChunkSegment {
        double start, end;
        std::vector<int> tokens;
        std::vector<std::pair<double, double>> token_timestamps;
    };
    struct ChunkedTsResult {
        std::vector<int> sequence;
        std::vector<ChunkSegment> segments;
    };
    std::vector<ChunkedTsResult> transcribe_chunked_ts(const float* pcm, const std::vector<int32_t>& n_samples, int stride, bool word,
                                                       int chunk_len = 480000, int stride_left = -1, int stride_right = -1, int max_loop = MAX_LOOP,
                                                       int32_t first_special = 50257, bool pcm_on_device = false, double time_precision = 0.0) const {
        need_model();
        wm_decode_opts o = opts(max_loop, false);
        const int R = (int)n_samples.size(), sl = stride_left < 0 ? chunk_len / 6 : stride_left, sr = stride_right < 0 ? chunk_len / 6 : stride_right;
        int32_t n = 0;
        check(wm_chunk_table(n_samples.data(), R, chunk_len, sl, sr, 0, nullptr, 0, &n));
        std::vector<int32_t> tab((size_t)(n > 0 ? n : 1) * 6);
        check(wm_chunk_table(n_samples.data(), R, chunk_len, sl, sr, 0, tab.data(), n, &n));
        std::vector<int> per(R, 0);
        for (int k = 0; k < n; ++k) ++per[tab[(size_t)k * 6]];
        const int total = o.n_prompt + 1 + max_loop;
        int cap = 1;
        for (int v : per) cap = v * total > cap ? v * total : cap;
        const int seg_cap = cap + 1;
        std::vector<int32_t> merged((size_t)R * cap), mlen(R), nseg(R), range((size_t)R * seg_cap * 2);
        std::vector<double> times((size_t)R * seg_cap * 2), pairs(word ? (size_t)R * cap * 2 : 0);
        check(wm_transcribe_chunked_ts(model_, pcm, pcm_on_device ? 1 : 0, n_samples.data(), R, stride, chunk_len, sl, sr, &o, nullptr, 0, first_special,
                                       word ? 2 : 1, time_precision, merged.data(), mlen.data(), cap, nseg.data(), times.data(), range.data(), seg_cap,
                                       word ? pairs.data() : nullptr, nullptr, nullptr, nullptr, nullptr));
        std::vector<ChunkedTsResult> out(R);
        for (int r = 0; r < R; ++r) {
            const int32_t* ids = merged.data() + (size_t)r * cap;
            out[r].sequence.assign(ids, ids + mlen[r]);
            for (int k = 0; k < nseg[r]; ++k) {
                const size_t at = ((size_t)r * seg_cap + k) * 2;
                ChunkSegment sg{times[at], times[at + 1], std::vector<int>(ids + range[at], ids + range[at + 1]), {}};
                for (int j = range[at]; word && j < range[at + 1]; ++j)
                    sg.token_timestamps.emplace_back(pairs[((size_t)r * cap + j) * 2], pairs[((size_t)r * cap + j) * 2 + 1]);
                out[r].segments.push_back(std::move(sg));
            }
        }
        return out;
    }
    // other prompts / stop ids (reduced test models have small vocabularies); defaults are the reference's
    void set_prompt(const std::vector<int32_t>& prompt, int32_t eot) {
        prompt_ = prompt;
        eot_ = eot;
    }
    // timestamp rules of HF generate (the reference has none): timestamp_begin <= 0 switches them off
    void set_timestamps(int timestamp_begin, int no_timestamps_token, int max_initial_timestamp_index) {
        ts_begin_ = timestamp_begin;
        no_ts_ = no_timestamps_token;
        max_init_ = max_initial_timestamp_index;
    }
    // HF generate's repetition_penalty / no_repeat_ngram_size for every transcribe / transcribe_long call from now on:
    // 1.0 and 0 switch them off (the default).  Throws std::invalid_argument for a penalty <= 0 or an n outside [0, 64].
    void set_repeat_options(float repetition_penalty, int no_repeat_ngram_size) {
        need_model();
        if (wm_set_repeat_options(model_, repetition_penalty, no_repeat_ngram_size) != WM_OK) throw std::invalid_argument(wm_last_error());
    }
    // Top-k alternatives for every log-prob call (transcribe_batch_lp and its kin) from now on: 0 = off (the default),
    // 1..8.  After such a call top_k() returns, per utterance and per GENERATED position, the k (id, log-prob) candidates in
    // descending score — rank 0 the emitted id with token_logprobs' value; (-1, -inf) where no finite candidate is left.
    // prompt_len: the prompt lengths the call ran with (one entry = the shared prompt's).  Throws std::invalid_argument for what
    // wm_set_top_k refuses; the long-form calls refuse to run while it is non-zero.
    void set_top_k(int k) {
        need_model();
        if (wm_set_top_k(model_, k) != WM_OK) throw std::invalid_argument(wm_last_error());
        top_k_ = k;
    }
    struct TopK {
        std::vector<int32_t> ids;  // [positions][k]
        std::vector<float> logprobs;
    };
    std::vector<TopK> top_k(const std::vector<std::vector<int>>& result, const std::vector<int>& prompt_len, int max_loop = MAX_LOOP) const {
        need_model();
        const int B = (int)result.size(), k = top_k_;
        int lmax = 0;
        for (int v : prompt_len) lmax = std::max(lmax, v);
        const size_t stride = (size_t)lmax + 1 + max_loop;
        std::vector<int32_t> ids((size_t)B * stride * std::max(k, 1));
        std::vector<float> lps(ids.size());
        check(wm_transcribe_top_k(model_, 0, ids.data(), lps.data()));
        std::vector<TopK> out(B);
        for (int b = 0; b < B; ++b) {
            const size_t p0 = (size_t)prompt_len[prompt_len.size() == 1 ? 0 : b], p1 = std::max(p0, result[b].size());
            out[b].ids.assign(ids.begin() + (b * stride + p0) * k, ids.begin() + (b * stride + p1) * k);
            out[b].logprobs.assign(lps.begin() + (b * stride + p0) * k, lps.begin() + (b * stride + p1) * k);
        }
        return out;
    }
    // HF generate's sequence_bias / bad_words_ids, as ids, for every transcribe / transcribe_long call from now on: each
    // bias entry is (ids, bias), each bad word a list of ids; two empty lists switch them off (the default).  Throws
    // std::invalid_argument for what wm_set_sequence_bias refuses.
    void set_sequence_bias(const std::vector<std::pair<std::vector<int32_t>, float>>& sequence_bias,
                           const std::vector<std::vector<int32_t>>& bad_words_ids) {
        need_model();
        std::vector<int32_t> ids, off{0}, bids, boff{0};
        std::vector<float> bias;
        for (const auto& s : sequence_bias) {
            ids.insert(ids.end(), s.first.begin(), s.first.end());
            off.push_back((int32_t)ids.size());
            bias.push_back(s.second);
        }
        for (const auto& s : bad_words_ids) {
            bids.insert(bids.end(), s.begin(), s.end());
            boff.push_back((int32_t)bids.size());
        }
        if (wm_set_sequence_bias(model_, ids.data(), off.data(), bias.data(), (int)sequence_bias.size(), bids.data(), boff.data(),
                                 (int)bad_words_ids.size()) != WM_OK)
            throw std::invalid_argument(wm_last_error());
    }
    // Phrase-list constraint for every transcribe call from now on: the generated ids of every row, without the ids >=
    // free_from (< 0: none), are confined to one of the phrases followed by eot.  An empty list switches it off (the default; the C
    // entry wants NULL for that, which is what this passes).  Throws std::invalid_argument for what wm_set_constraint refuses; the
    // long-form calls refuse to run while it is set.  After a call, constraint_match(B) returns per row the index of the phrase it
    // stood on when it emitted eot, or -1.
    void set_constraint(const std::vector<std::vector<int32_t>>& phrases, int free_from = -1) {
        need_model();
        std::vector<int32_t> ids, off{0};
        for (const auto& s : phrases) {
            ids.insert(ids.end(), s.begin(), s.end());
            off.push_back((int32_t)ids.size());
        }
        const bool none = phrases.empty();
        if (wm_set_constraint(model_, none ? nullptr : ids.data(), none ? nullptr : off.data(), (int)phrases.size(), free_from) != WM_OK)
            throw std::invalid_argument(wm_last_error());
    }
    std::vector<int32_t> constraint_match(int B, int slot = 0) const {
        need_model();
        std::vector<int32_t> out((size_t)B);
        check(wm_transcribe_constraint_match(model_, slot, out.data(), B));
        return out;
    }
    // The trie wm_set_constraint builds from the phrases, flattened as the library flattens it: node v's child edges are edge_id /
    // edge_next [edge_off[v], edge_off[v + 1]), ids ascending; terminal[v] is the index of the phrase that ends at v or -1.  Node 0 is
    // the root, nodes are numbered in the order the phrases, in the caller's order and id by id, first reach them, and the last node
    // is the dead node (no edges, no phrase).  Host code only — for callers that want to walk the trie themselves (which ids may
    // follow a prefix), and checked against the Python host's builder.  Throws std::invalid_argument for a duplicate phrase.
    struct ConstraintTrie {
        std::vector<int32_t> edge_off, edge_id, edge_next, terminal;
    };
    static ConstraintTrie constraint_trie(const std::vector<std::vector<int32_t>>& phrases) {
        std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(1);  // per node: (id, child), ascending by id
        ConstraintTrie t;
        t.terminal.assign(1, -1);
        for (size_t q = 0; q < phrases.size(); ++q) {
            int32_t v = 0;
            for (int32_t id : phrases[q]) {
                auto it = std::lower_bound(kids[v].begin(), kids[v].end(), std::make_pair(id, (int32_t)-1));
                if (it != kids[v].end() && it->first == id) {
                    v = it->second;
                } else {
                    const int32_t nv = (int32_t)kids.size();
                    kids[v].insert(it, std::make_pair(id, nv));
                    kids.emplace_back();
                    t.terminal.push_back(-1);
                    v = nv;
                }
            }
            if (t.terminal[v] >= 0) throw std::invalid_argument("constraint: a phrase is given twice");
            t.terminal[v] = (int32_t)q;
        }
        kids.emplace_back();  // the dead node
        t.terminal.push_back(-1);
        t.edge_off.push_back(0);
        for (const auto& e : kids) {
            for (const auto& pr : e) {
                t.edge_id.push_back(pr.first);
                t.edge_next.push_back(pr.second);
            }
            t.edge_off.push_back((int32_t)t.edge_id.size());
        }
        return t;
    }
    const WhisperConfig& config() const { return cfg_; }
    wm_model* handle() const { return model_; }

private:
    void need_model() const {
        if (!model_) throw std::runtime_error("Whisper: load() first");
    }
    wm_decode_opts opts(int max_loop, bool ignore_eot) const {
        wm_decode_opts o;
        std::memset(&o, 0, sizeof o);
        o.prompt = prompt_.data();
        o.n_prompt = (int)prompt_.size();
        o.eot = eot_;
        o.max_loop = max_loop;
        o.pos_mode = WM_POS_REF;  // start_pos = current_len - 1 (whisper.mojo:217)
        o.ignore_eot = ignore_eot ? 1 : 0;
        o.timestamp_begin = ts_begin_;
        o.no_timestamps_token = no_ts_;
        o.max_initial_timestamp_index = max_init_;
        return o;
    }
    static std::vector<std::vector<int>> unpack(const std::vector<int32_t>& toks, const std::vector<int32_t>& n, int B, int stride) {
        std::vector<std::vector<int>> out(B);
        for (int b = 0; b < B; ++b) out[b].assign(toks.begin() + (size_t)b * stride, toks.begin() + (size_t)b * stride + n[b]);
        return out;
    }
    // [B][lmax] table and lengths of per-utterance prompts -> lmax (0 without prompts)
    static int prompt_table(const std::vector<std::vector<int32_t>>& prompts, int B, std::vector<int32_t>& tab, std::vector<int32_t>& len) {
        int lmax = 0;
        for (const auto& r : prompts) lmax = std::max(lmax, (int)r.size());
        tab.assign((size_t)B * std::max(lmax, 1), 0);
        len.assign(B, 0);
        for (size_t b = 0; b < prompts.size() && b < (size_t)B; ++b) {
            len[b] = (int32_t)prompts[b].size();
            std::copy(prompts[b].begin(), prompts[b].end(), tab.begin() + b * lmax);
        }
        return lmax;
    }
    struct LangSlot {
        int B = 0, stride = 0, n_lang = 0;
        bool lp = false, ns = false;
    };
    template <typename Call> static LangResult lang_collect(const LangSlot& q, Call call) {
        LangResult r;
        std::vector<int32_t> toks((size_t)q.B * q.stride), n(q.B);
        std::vector<float> lp(q.lp ? (size_t)q.B * q.stride : 0);
        r.lang.assign(q.B, 0);
        r.lang_probs.assign((size_t)q.B * q.n_lang, 0.f);
        if (q.lp) r.avg_logprob.assign(q.B, 0.f);
        if (q.ns) r.no_speech_prob.assign(q.B, 0.f);
        check(call(toks.data(), n.data(), q.lp ? lp.data() : nullptr, q.lp ? r.avg_logprob.data() : nullptr,
                   q.ns ? r.no_speech_prob.data() : nullptr, r.lang.data(), r.lang_probs.data()));
        r.ids = unpack(toks, n, q.B, q.stride);
        if (q.lp) {
            r.token_logprobs.assign(q.B, {});
            for (int b = 0; b < q.B; ++b) r.token_logprobs[b].assign(lp.begin() + (size_t)b * q.stride, lp.begin() + (size_t)b * q.stride + n[b]);
        }
        return r;
    }
    LangSlot lang_pend_[8] = {};
    WhisperConfig cfg_;
    std::vector<int32_t> prompt_{PROMPT, PROMPT + 4};
    int32_t eot_ = EOT;
    int ts_begin_ = 0, no_ts_ = -1, max_init_ = -1;
    wm_config wcfg_{};
    int device_ = 0;
    wm_model* model_ = nullptr;
    int top_k_ = 0;  // what set_top_k set on model_
    struct Pend {
        int B, stride;
    };
    Pend pend_[8] = {};
};

// tokenizer.mojo:4-28: vocab.txt, line index = id; decode drops <|...|>, maps "Ġ" to a space and the escaped "\n" to a
// newline — the reference's rendering, bug for bug (non-ASCII text stays in its byte-level symbols)
class Tokenizer {
public:
    explicit Tokenizer(const std::string& path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw std::runtime_error("Tokenizer: cannot open " + path);  // tokenizer.mojo:9 raises
        std::stringstream ss;
        ss << f.rdbuf();
        const std::string content = ss.str();
        size_t a = 0;
        for (;;) {  // content.split("\n"): a trailing newline yields a last empty entry, as in the reference
            const size_t b = content.find('\n', a);
            if (b == std::string::npos) {
                vocab_.push_back(content.substr(a));
                break;
            }
            vocab_.push_back(content.substr(a, b - a));
            a = b + 1;
        }
    }
    std::string decode(const std::vector<int>& tokens) const {
        static const std::string G = "\xC4\xA0";  // "Ġ" (U+0120) in UTF-8
        std::string result;
        for (int id : tokens) {
            if (id < 0 || id >= (int)vocab_.size()) continue;  // tokenizer.mojo:19
            const std::string& t = vocab_[id];
            if (t.size() >= 4 && t.compare(0, 2, "<|") == 0 && t.compare(t.size() - 2, 2, "|>") == 0) continue;
            std::string c = t;
            replace_all(c, G, " ");
            replace_all(c, "\\n", "\n");
            result += c;
        }
        return result;
    }
    size_t size() const { return vocab_.size(); }

private:
    static void replace_all(std::string& s, const std::string& from, const std::string& to) {
        for (size_t p = 0; (p = s.find(from, p)) != std::string::npos; p += to.size()) s.replace(p, from.size(), to);
    }
    std::vector<std::string> vocab_;
};

}  // namespace whisper_mi
