// Host check of include/whisper_mi.hpp's Whisper::constraint_trie: prints the flattened trie of a fixed phrase list,
// one array per line, for tests/test_constraint_cpp.py to compare with the Python host's builder.  Host code only: nothing of the
// library is called, so it also builds and runs stand-alone under -fsanitize=address,undefined.
//   constraint_check            the arrays of the fixed list
//   constraint_check dup        a duplicate phrase must throw std::invalid_argument (exit 0 when it does)
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

int main(int argc, char** argv) {
    // shared prefixes, a phrase that is a prefix of another (both ways round in the list), fan-out 1 chains, ids out of order, and a
    // root fan-out of 640 behind them
    std::vector<std::vector<int32_t>> phrases = {{7, 3, 9}, {7, 3}, {7, 4}, {2}, {2, 2, 2, 2}, {11, 5, 5, 1, 0, 8}, {7, 3, 9, 9}, {0}, {11, 5}, {3, 7}};
    for (int32_t i = 0; i < 640; ++i) phrases.push_back({1000 + 3 * ((i * 37) % 640), i % 5});
    if (argc > 1 && !std::strcmp(argv[1], "dup")) {
        phrases.push_back({7, 4});
        try {
            (void)whisper_mi::Whisper::constraint_trie(phrases);
        } catch (const std::invalid_argument&) {
            return 0;
        }
        std::fprintf(stderr, "a duplicate phrase did not throw\n");
        return 1;
    }
    const auto t = whisper_mi::Whisper::constraint_trie(phrases);
    line("edge_off", t.edge_off);
    line("edge_id", t.edge_id);
    line("edge_next", t.edge_next);
    line("terminal", t.terminal);
    return 0;
}
