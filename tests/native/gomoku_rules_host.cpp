// Host build of csrc/gomoku_rules.h (the Renju / Omok predicates the device kernels and the host
// GomokuState share), for tests/test_gomoku_rules_cpu.py: a stand-alone program, so that it also
// runs under -fsanitize=address,undefined.
//
// stdin: one position per line, "bs renju omok n m0 .. m(n-1)" (moves alternate Black, White).
// stdout: per position one line of five ';'-separated fields -- the empty cells with a Renju
// overline, with a double four, with an Omok double three (cells separated by ','), the legal
// count of gomoku_forbidden_mask for the side to move, and its mask words in hex.
// Every verdict is computed twice where the shortcut applies (whole-board scan, and the windows
// through the cell only when the board as it stands has no shape): a disagreement is an error.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../alphazero-multi-game_amd/csrc/gomoku_rules.h"

int main() {
    int bs, renju, omok, n;
    int line = 0;
    while (std::scanf("%d %d %d %d", &bs, &renju, &omok, &n) == 4) {
        if (bs < 5 || bs > 19 || n < 0 || n > bs * bs) { std::fprintf(stderr, "line %d: bad header\n", line); return 2; }
        const int A = bs * bs;
        // the board alone in its allocation: a read past either end is the sanitizer's to catch
        std::vector<uint8_t> board(A, 0);
        for (int i = 0; i < n; ++i) {
            int m;
            if (std::scanf("%d", &m) != 1 || m < 0 || m >= A || board[m]) { std::fprintf(stderr, "line %d: bad move\n", line); return 2; }
            board[m] = (uint8_t)(1 + i % 2);
        }
        const uint8_t* b = board.data();
        const bool fours = gomoku_any_four_shape(b, bs, 0, 1), threes = gomoku_any_open_three(b, bs, 0, 1);
        // the strided form a wave shares: the union over the shares is the whole scan
        bool f64 = false, t64 = false;
        for (int l = 0; l < 64; ++l) { f64 |= gomoku_any_four_shape(b, bs, l, 64); t64 |= gomoku_any_open_three(b, bs, l, 64); }
        if (f64 != fours || t64 != threes) { std::fprintf(stderr, "line %d: strided base scan differs\n", line); return 1; }
        std::vector<int> over, four, three;
        for (int a = 0; a < A; ++a) {
            if (b[a]) continue;
            if (gomoku_overline(b, bs, a)) over.push_back(a);
            const bool d4 = gomoku_double_four(b, bs, a, true), d3 = gomoku_double_three(b, bs, a, true);
            if (!fours && gomoku_double_four(b, bs, a, false) != d4) { std::fprintf(stderr, "line %d cell %d: local fours differ\n", line, a); return 1; }
            if (!threes && gomoku_double_three(b, bs, a, false) != d3) { std::fprintf(stderr, "line %d cell %d: local threes differ\n", line, a); return 1; }
            if (d4) four.push_back(a);
            if (d3) three.push_back(a);
        }
        uint64_t mask[(19 * 19 + 63) / 64];
        const int legal = gomoku_forbidden_mask(b, bs, 1 + n % 2, renju, omok, mask);
        const std::vector<int>* lists[3] = {&over, &four, &three};
        for (const auto* l : lists) {
            for (size_t i = 0; i < l->size(); ++i) std::printf("%s%d", i ? "," : "", (*l)[i]);
            std::printf(";");
        }
        std::printf("%d;", legal);
        for (int w = 0; w < (A + 63) / 64; ++w) std::printf("%s%llx", w ? "," : "", (unsigned long long)mask[w]);
        std::printf("\n");
        ++line;
    }
    return 0;
}
