// The C++ host mirror's top-k entry (include/whisper_mi.hpp: Whisper::set_top_k / top_k) on the micro model with the
// synthetic weights: two utterances, shared prompt (1 2 3 4) or, with a second argument, per-row prompts (1 2 3 4) and (2 3).
// Prints per utterance one line "ids ..." and one line "top id:bits ..." (bits: the log-prob's fp32 pattern in hex), which
// tests/test_gpu_topk.py compares with the Python host's result.
//   topk_check K MAX_LOOP [rows]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "whisper_mi.hpp"

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const int k = atoi(argv[1]), max_loop = atoi(argv[2]);
    const bool rows = argc > 3;
    using namespace whisper_mi;
    const WhisperConfig cfg = WhisperConfig::micro();
    const wm_dims d = cfg.dims();
    std::vector<float> w(cfg.weight_count());
    wm_synth_weights(&d, 0, w.data());
    const int B = 2;
    const size_t per = (size_t)cfg.n_mels * cfg.n_frames();
    std::vector<float> mels(B * per);
    for (int b = 0; b < B; ++b) wm_synth_mel_host(1000 + b, cfg.n_mels, cfg.n_frames(), mels.data() + b * per);
    try {
        Whisper m(cfg, WM_F32, -1, B);
        m.load(w.data(), w.size());
        m.set_prompt({1, 2, 3, 4}, -1);
        m.set_top_k(k);
        std::vector<std::vector<float>> lps;
        std::vector<float> avg;
        const std::vector<std::vector<int32_t>> prompts = rows ? std::vector<std::vector<int32_t>>{{1, 2, 3, 4}, {2, 3}} : std::vector<std::vector<int32_t>>{};
        const auto ids = m.transcribe_batch_lp(mels.data(), B, lps, avg, max_loop, prompts);
        const auto top = m.top_k(ids, rows ? std::vector<int>{4, 2} : std::vector<int>{4}, max_loop);
        m.set_top_k(0);
        for (int b = 0; b < B; ++b) {
            printf("ids");
            for (int t : ids[b]) printf(" %d", t);
            printf("\ntop");
            for (size_t i = 0; i < top[b].ids.size(); ++i) {
                uint32_t bits;
                memcpy(&bits, &top[b].logprobs[i], 4);
                printf(" %d:%08x", top[b].ids[i], bits);
            }
            printf("\n");
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
