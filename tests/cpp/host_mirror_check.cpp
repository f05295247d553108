// Every public entry of the C++ host mirror (include/whisper_mi.hpp: class Whisper) that no other program calls, on the micro model
// with the synthetic weights (seed 0) and the synthetic mels / PCM of seeds 1000 + b.  argv[1] selects a mode; every
// result field is printed on a line of its own: a name, the number of values, then the values — integers in decimal, every float as
// its 8-hex-digit bit pattern, every double as 16 hex digits ("nan" for a NaN, whose payload the Python host does not keep); nested
// vectors go row by row.  tests/test_gpu_cpp_mirror.py builds the same lines from the Python host's results and compares the text.
//   host_mirror_check MODE      MODE: slots tt lp_ns score nbest align lang long resample chunked processors
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "whisper_mi.hpp"

using namespace whisper_mi;

namespace {

const std::vector<int32_t> PROMPT3{1, 2, 3};
const int32_t EOT = 900, NO_SPEECH = 939, PREV_SOT = 938;
const int TS_BEGIN = 941, NO_TS = 940, MAX_INIT = 50;
const std::vector<std::pair<int, int>> HEADS{{0, 1}, {1, 0}};
const std::vector<int32_t> LANGS{20, 7, 33, 12};

void put(float v) {
    uint32_t b;
    memcpy(&b, &v, 4);
    if (std::isnan(v)) printf(" nan");
    else printf(" %08x", b);
}
void put(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    if (std::isnan(v)) printf(" nan");
    else printf(" %016llx", (unsigned long long)b);
}
void put(int v) { printf(" %d", v); }
void put(int64_t v) { printf(" %lld", (long long)v); }

template <typename T> void line(const std::string& name, const std::vector<T>& v) {
    printf("%s %zu", name.c_str(), v.size());
    for (const T& x : v) put(x);
    printf("\n");
}
template <typename T> void rows(const std::string& name, const std::vector<std::vector<T>>& v) {
    for (const auto& r : v) line(name, r);
}
template <typename T> void one(const std::string& name, T v) { line(name, std::vector<T>{v}); }

struct Micro {
    WhisperConfig cfg = WhisperConfig::micro();
    std::vector<float> w;
    size_t per;
    Micro() : w(cfg.weight_count()), per((size_t)cfg.n_mels * cfg.n_frames()) {
        const wm_dims d = cfg.dims();
        wm_synth_weights(&d, 0, w.data());
    }
    // [n][n_mels][n_frames], seeds 1000 + first + b
    std::vector<float> mels(int n, int first = 0) const {
        std::vector<float> m(n * per);
        for (int b = 0; b < n; ++b) wm_synth_mel_host(1000 + first + b, cfg.n_mels, cfg.n_frames(), m.data() + b * per);
        return m;
    }
    // [B][n_mels][T]: utterance b is the windows of seeds 1000 * (seed0 + b) + k side by side, cropped to T frames
    std::vector<float> long_mels(int B, int T, int seed0) const {
        const int F = cfg.n_frames();
        std::vector<float> out((size_t)B * cfg.n_mels * T), win(per);
        for (int b = 0; b < B; ++b)
            for (int k = 0; k * F < T; ++k) {
                wm_synth_mel_host(1000 * (uint64_t)(seed0 + b) + k, cfg.n_mels, F, win.data());
                for (int r = 0; r < cfg.n_mels; ++r)
                    for (int c = 0; c < F && k * F + c < T; ++c) out[((size_t)b * cfg.n_mels + r) * T + k * F + c] = win[(size_t)r * F + c];
            }
        return out;
    }
    void load(Whisper& m) const {
        m.load(w.data(), w.size());
        m.set_prompt(PROMPT3, EOT);
        if (!m.handle() || m.config().d_model != cfg.d_model || m.config().vocab_size != cfg.vocab_size)
            throw std::runtime_error("load: no model handle, or another config than the one given");
    }
};

// [B][stride] samples in [-1, 1.5] scaled by 1 / 4 (exact): row b is the synthetic mel generator's stream of seed 1000 + b
std::vector<float> pcm_rows(int B, int stride) {
    std::vector<float> p((size_t)B * stride);
    for (int b = 0; b < B; ++b) wm_synth_mel_host(1000 + b, 1, stride, p.data() + (size_t)b * stride);
    for (float& v : p) v *= 0.25f;
    return p;
}

void print_score(const std::string& tag, const Whisper::ScoreResult& r) {
    rows(tag + ".lp", r.token_logprobs);
    line(tag + ".sum", r.sum_logprob);
    line(tag + ".avg", r.avg_logprob);
    rows(tag + ".top", r.top_ids);
}

void print_lang(const std::string& tag, const Whisper::LangResult& r) {
    rows(tag + ".ids", r.ids);
    line(tag + ".lang", r.lang);
    line(tag + ".probs", r.lang_probs);
    rows(tag + ".lp", r.token_logprobs);
    line(tag + ".avg", r.avg_logprob);
    line(tag + ".nsp", r.no_speech_prob);
}

void print_long(const std::string& tag, const std::vector<Whisper::LongResult>& res) {
    for (size_t b = 0; b < res.size(); ++b) {
        const std::string u = tag + ".u" + std::to_string(b);
        line(u + ".seq", res[b].sequence);
        one(u + ".nseg", (int)res[b].segments.size());
        for (const auto& sg : res[b].segments) {
            line(u + ".seg.span", std::vector<double>{sg.start, sg.end});
            line(u + ".seg.tokens", sg.tokens);
            line(u + ".seg.quality", std::vector<float>{sg.avg_logprob, sg.no_speech_prob});
            line(u + ".seg.tt", sg.token_timestamps);
        }
        one(u + ".nwin", (int)res[b].windows.size());
        for (const auto& w : res[b].windows) {
            line(u + ".win.seek", std::vector<int64_t>{w.seek, w.skipped ? 1 : 0});
            line(u + ".win.quality", std::vector<float>{w.avg_logprob, w.no_speech_prob});
        }
        line(u + ".times", res[b].token_times);
    }
}

int mode_slots(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto a = k.mels(3, 0), b = k.mels(2, 3);
    m.transcribe_submit(a.data(), 3, 0, 9);
    m.transcribe_submit(b.data(), 2, 1, 11);
    const auto r1 = m.transcribe_wait(1);
    const auto r0 = m.transcribe_wait(0);
    rows("wait1", r1);
    rows("wait0", r0);
    rows("batch0", m.transcribe_batch(a.data(), 3, 9));
    rows("batch1", m.transcribe_batch(b.data(), 2, 11));
    return 0;
}

int mode_tt(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3);
    m.set_alignment_heads(HEADS);
    std::vector<std::vector<float>> t;
    rows("full.ids", m.transcribe_batch_tt(mel.data(), 3, t, 10));
    rows("full.times", t);
    rows("ragged.ids", m.transcribe_batch_tt(mel.data(), 3, t, 10, {200, 120, 60}));
    rows("ragged.times", t);
    m.set_alignment_heads({});
    rows("plain.ids", m.transcribe_batch(mel.data(), 3, 10));
    return 0;
}

int mode_lp_ns(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3);
    std::vector<std::vector<float>> lp;
    std::vector<float> avg, nsp;
    rows("shared.ids", m.transcribe_batch_lp_ns(mel.data(), 3, NO_SPEECH, lp, avg, nsp, 9));
    rows("shared.lp", lp);
    line("shared.avg", avg);
    line("shared.nsp", nsp);
    rows("rows.ids", m.transcribe_batch_lp_ns(mel.data(), 3, NO_SPEECH, lp, avg, nsp, 9, {{1, 2}, {11, 12, 13, 1, 2}, {21, 1, 2}}, 2));
    rows("rows.lp", lp);
    line("rows.avg", avg);
    line("rows.nsp", nsp);
    return 0;
}

const std::vector<std::vector<int32_t>> SCORE_IDS{{1, 2, 3, 40, 41, 42, 43}, {1, 7}, {1, 2, 3, 50, 51}};

int mode_score(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3);
    print_score("plain", m.score(mel.data(), 3, SCORE_IDS, {}, true));
    print_score("ctx", m.score(mel.data(), 3, SCORE_IDS, {3, 1, 3}, true));
    print_score("notop", m.score(mel.data(), 3, SCORE_IDS, {3, 1, 3}));
    return 0;
}

int mode_nbest(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 4);
    k.load(m);
    const auto mel = k.mels(2);
    const std::vector<std::vector<std::vector<int32_t>>> cand{{{1, 2, 3, 40, 41, 42}, {1, 2, 3, 50}, {1, 2, 3, 60, 61, 62, 63, 64}}, {{1, 2, 3, 70, 71}}};
    for (int normalize = 0; normalize < 2; ++normalize) {
        const std::string tag = normalize ? "norm" : "sum";
        const auto r = m.score_candidates(mel.data(), 2, cand, {3, 3, 3, 2}, normalize != 0, true);
        print_score(tag, r.rows);
        line(tag + ".n_cand", r.n_cand);
        line(tag + ".row0", r.row0);
        line(tag + ".order", r.order);
        line(tag + ".best", r.best);
        line(tag + ".posterior", r.posterior);
    }
    return 0;
}

int mode_align(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3);
    m.set_alignment_heads(HEADS);
    const std::vector<std::vector<int32_t>> ids{{1, 2, 3, 40, 41, 42, 43}, {1, 7, 8}, {1, 2, 3, 50, 51}};
    Whisper::ScoreResult sc;
    rows("plain.times", m.align(mel.data(), 3, ids, {}, {}, &sc));
    print_score("plain", sc);
    rows("ragged.times", m.align(mel.data(), 3, ids, {3, 1, 3}, {200, 120, 60}, &sc));
    print_score("ragged", sc);
    rows("noscore.times", m.align(mel.data(), 3, ids, {3, 1, 3}, {200, 120, 60}));
    return 0;
}

int mode_lang(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3), two = k.mels(2, 3);
    std::vector<float> probs;
    line("detect.ids", m.detect_language(mel.data(), 3, LANGS, 1, &probs));
    line("detect.probs", probs);
    print_lang("plain", m.transcribe_batch_lang(mel.data(), 3, LANGS, 9));
    const std::vector<std::vector<int32_t>> pr3{{1, 2, 3}, {11, 12, 1, 2, 3}, {21, 1, 2, 3}}, pr2{{31, 32, 33, 1, 2, 3}, {1, 2, 3}};
    print_lang("rows", m.transcribe_batch_lang(mel.data(), 3, LANGS, 9, pr3, 3, true, NO_SPEECH));
    m.transcribe_submit_lang(mel.data(), 3, 0, LANGS, 8);
    m.transcribe_submit_lang(two.data(), 2, 1, {7, 33, 12, 20, 45}, 10, pr2, 3, true, NO_SPEECH);
    const auto r1 = m.transcribe_wait_lang(1);
    const auto r0 = m.transcribe_wait_lang(0);
    print_lang("wait1", r1);
    print_lang("wait0", r0);
    return 0;
}

int mode_long(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    m.set_timestamps(TS_BEGIN, NO_TS, MAX_INIT);
    const int B = 3, T = 500, L = 12;
    const auto mel = k.long_mels(B, T, 95);
    const std::vector<int32_t> nf{500, 330, 40}, pids{PREV_SOT, 11, 12, 13, 14};
    print_long("plain", m.transcribe_long(mel.data(), B, T, nf, L));
    print_long("full", m.transcribe_long(mel.data(), B, T, {}, L));
    print_long("first", m.transcribe_long(mel.data(), B, T, nf, L, true, pids, false, PREV_SOT));
    print_long("all", m.transcribe_long(mel.data(), B, T, nf, L, true, pids, true, PREV_SOT));
    Whisper::LongThresholds th;
    th.use_logprob_threshold = true;
    th.logprob_threshold = -1.0f;
    th.no_speech_token = NO_SPEECH;
    print_long("lpth", m.transcribe_long(mel.data(), B, T, nf, L, false, {}, false, PREV_SOT, &th));
    th.logprob_threshold = 0.0f;
    th.use_no_speech_threshold = true;
    th.no_speech_threshold = 0.0f;  // every window's no_speech_prob lies above it: all are skipped, no utterance has a segment
    print_long("skipall", m.transcribe_long(mel.data(), B, T, nf, L, false, {}, false, PREV_SOT, &th));
    th.no_speech_threshold = 0.00079f;  // between the windows' values (0.000788 .. 0.000795): some are skipped, some kept
    print_long("skipsome", m.transcribe_long(mel.data(), B, T, nf, L, false, {}, false, PREV_SOT, &th));
    std::vector<int32_t> lang;
    print_long("lang", m.transcribe_long(mel.data(), B, T, nf, L, false, {}, false, PREV_SOT, nullptr, LANGS, &lang));
    line("lang.out", lang);
    m.set_alignment_heads(HEADS);
    print_long("tt", m.transcribe_long(mel.data(), B, T, nf, L, false, {}, false, PREV_SOT, nullptr, {}, nullptr, true));
    lang.clear();
    print_long("ttlang", m.transcribe_long(mel.data(), B, T, nf, L, true, pids, false, PREV_SOT, nullptr, LANGS, &lang, true));
    line("ttlang.out", lang);
    return 0;
}

int mode_resample(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 2);
    k.load(m);
    const auto f = pcm_rows(2, 800);
    rows("f32", m.resample(f.data(), WM_F32, {700, 333}, 800, 8000));
    const auto g = pcm_rows(2, 1200);
    std::vector<int16_t> q(g.size());
    for (size_t i = 0; i < g.size(); ++i) q[i] = (int16_t)(g[i] * 32768.0f);
    rows("i16", m.resample(q.data(), WM_I16, {1000, 441}, 1200, 44100));
    return 0;
}

int mode_chunked(const Micro& k) {
    // the vocabulary as tests/test_gpu_chunked_ts.py lays it out: specials from 890, timestamps from 899
    const int32_t first_special = 890;
    const int chunk = 32000, L = 10, stride = 70000;
    Whisper m(k.cfg, WM_F32, -1, 2);
    k.load(m);
    m.set_prompt({891, 892, 893}, first_special);
    m.set_repeat_options(1.0f, 2);
    const auto pcm = pcm_rows(2, stride);
    const std::vector<int32_t> n{70000, 50000};
    auto plain = [&](const std::string& tag, const std::vector<Whisper::ChunkedResult>& res) {
        for (size_t r = 0; r < res.size(); ++r) {
            const std::string u = tag + ".r" + std::to_string(r);
            line(u + ".seq", res[r].sequence);
            one(u + ".nchunks", (int)res[r].chunks.size());
            for (const auto& c : res[r].chunks) {
                line(u + ".chunk.at", std::vector<int>{c.start, c.len, c.stride_left, c.stride_right});
                line(u + ".chunk.ids", c.tokens);
            }
        }
    };
    plain("chunks", m.transcribe_chunked(pcm.data(), n, stride, chunk, -1, -1, true, L, {}, first_special));
    plain("merged", m.transcribe_chunked(pcm.data(), n, stride, chunk, 4000, 3000, false, L, {}, first_special));
    plain("lang", m.transcribe_chunked(pcm.data(), n, stride, chunk, -1, -1, true, L, {895, 894, 896}, first_special));
    m.set_timestamps(899, 898, 50);
    m.set_alignment_heads(HEADS);
    for (int word = 0; word < 2; ++word) {
        const auto res = m.transcribe_chunked_ts(pcm.data(), n, stride, word != 0, chunk, -1, -1, L, first_special);
        for (size_t r = 0; r < res.size(); ++r) {
            const std::string u = std::string(word ? "word" : "segs") + ".r" + std::to_string(r);
            line(u + ".seq", res[r].sequence);
            one(u + ".nseg", (int)res[r].segments.size());
            for (const auto& sg : res[r].segments) {
                line(u + ".seg.span", std::vector<double>{sg.start, sg.end});
                line(u + ".seg.tokens", sg.tokens);
                std::vector<double> flat;
                for (const auto& p : sg.token_timestamps) flat.insert(flat.end(), {p.first, p.second});
                line(u + ".seg.pairs", flat);
            }
        }
    }
    return 0;
}

int mode_processors(const Micro& k) {
    Whisper m(k.cfg, WM_F32, -1, 3);
    k.load(m);
    const auto mel = k.mels(3);
    auto run = [&](const std::string& tag) {
        std::vector<std::vector<float>> lp;
        std::vector<float> avg;
        rows(tag + ".ids", m.transcribe_batch_lp(mel.data(), 3, lp, avg, 10));
        rows(tag + ".lp", lp);
        line(tag + ".avg", avg);
    };
    run("plain");
    m.set_repeat_options(1.3f, 2);
    run("repeat");
    m.set_repeat_options(1.0f, 0);
    m.set_sequence_bias({{{13}, 1.5f}, {{3, 17}, 2.0f}}, {{18}});
    run("bias");
    m.set_sequence_bias({}, {});
    m.set_constraint({{11, 12}, {13}, {14, 15, 16}});
    run("constraint");
    line("constraint.match", m.constraint_match(3));
    m.set_constraint({});
    m.set_timestamps(TS_BEGIN, NO_TS, MAX_INIT);
    run("timestamps");
    m.set_timestamps(0, -1, -1);
    run("again");
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    try {
        const Micro k;
        if (mode == "slots") return mode_slots(k);
        if (mode == "tt") return mode_tt(k);
        if (mode == "lp_ns") return mode_lp_ns(k);
        if (mode == "score") return mode_score(k);
        if (mode == "nbest") return mode_nbest(k);
        if (mode == "align") return mode_align(k);
        if (mode == "lang") return mode_lang(k);
        if (mode == "long") return mode_long(k);
        if (mode == "resample") return mode_resample(k);
        if (mode == "chunked") return mode_chunked(k);
        if (mode == "processors") return mode_processors(k);
        fprintf(stderr, "unknown mode %s\n", mode.c_str());
        return 2;
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
