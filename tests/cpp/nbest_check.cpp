// Host check of include/whisper_mi.hpp's Whisper::nbest_table: prints the flat table of a fixed candidate list, one array
// per line, for tests/test_nbest_cpp.py to compare with the Python host's _lib.nbest_args.  Host code only: nothing of the library is
// called, so it also builds and runs stand-alone under -fsanitize=address,undefined.
//   nbest_check            the arrays of the fixed list
//   nbest_check bad        a wrong clip count, an empty clip and a wrong context_len count must each throw (exit 0 when all do)
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "whisper_mi.hpp"

static void line(const char* name, const std::vector<int32_t>& v) {
    std::printf("%s", name);
    for (int32_t x : v) std::printf(" %d", x);
    std::printf("\n");
}
using Cands = std::vector<std::vector<std::vector<int32_t>>>;
static bool throws(int U, const Cands& c, const std::vector<int32_t>& ctx) {
    try {
        (void)whisper_mi::Whisper::nbest_table(U, c, ctx);
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

int main(int argc, char** argv) {
    // 1, 4 and 2 candidates of unequal lengths, the longest row in the middle clip
    const Cands cands = {{{1, 2, 3}}, {{4, 5}, {6, 7, 8, 9, 10, 11, 12}, {1, 1}, {9, 9, 9}}, {{2, 3, 4, 5, 6}, {9, 8}}};
    if (argc > 1 && !std::strcmp(argv[1], "bad")) {
        const bool ok = throws(2, cands, {}) && throws(0, {}, {}) && throws(2, {{{1, 2}}, {}}, {}) && throws(3, cands, {1, 1, 1}) &&
                        !throws(3, cands, {1, 1, 2, 1, 1, 3, 1});
        if (!ok) std::fprintf(stderr, "a refusal is missing\n");
        return ok ? 0 : 1;
    }
    const auto t = whisper_mi::Whisper::nbest_table(3, cands, {});
    line("shape", {t.R, t.stride});
    line("tab", t.tab);
    line("len", t.len);
    line("n_cand", t.n_cand);
    line("row0", t.row0);
    line("utt_of", t.utt_of);
    return 0;
}
