// gomoku_rules.h -- the Gomoku rule variants (Renju, Omok): which empty cells Black may not play.
//
// One statement of the rules for the device kernels (tree_kernels.hip) and the host GomokuState
// (cpp/src/gomoku_state.cpp), over a board of A = bs * bs bytes (0 empty, 1 black, 2 white; cell
// a = x * bs + y).  The target is the reference's GomokuRules with its accessor recursion repaired
// (patch P11), quirks included:
//
//   Renju   overline (a black run of six or more through the cell), or two four-shapes on the
//           WHOLE board with the stone added.  A four-shape is a window of 5, 6 or 7 cells on a
//           line with no white stone, exactly four black ones and an empty in-bounds cell just
//           outside either end.  The reference counts shapes greedily in scan order, dropping one
//           that shares three or more stones with an accepted one; "two or more" is therefore:
//           some shape shares fewer than three stones with the first shape of the scan.  Its
//           double-three test never forbids a cell, so there is none here.
//   Omok    overline, or two distinct open threes with the stone added, connected (some stone of
//           one within Chebyshev distance 1 of some stone of the other; a shared stone counts).
//           An open three is a 5-cell slice .BBB. with no BLACK stone just beyond either end (a
//           white stone or the edge there does not close it).
//   both    Renju decides.  White is never restricted.
//
// A stone added at `cand` creates only shapes that contain it and can remove any other, so when
// the board as it stands has no shape at all (the usual case) only the windows through `cand` are
// looked at; otherwise the whole board is scanned.  The callers compute that fact once per
// position (gomoku_any_four_shape / gomoku_any_open_three, strided so that a wave can share it).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AZ_GR_HD __host__ __device__ inline
#else
#define AZ_GR_HD inline
#endif

// directions of the reference's scans, in its order: (dx, dy) with a = x * bs + y
AZ_GR_HD int gomoku_dx(int d) { return d == 0 ? 0 : d == 3 ? -1 : 1; }
AZ_GR_HD int gomoku_dy(int d) { return d == 1 ? 0 : 1; }

// the board with a black stone added at cand (cand < 0: the board as it stands)
AZ_GR_HD int gomoku_at(const uint8_t* board, int cand, int a) { return a == cand ? 1 : board[a]; }

AZ_GR_HD bool gomoku_overline(const uint8_t* board, int bs, int a) {
    const int x0 = a / bs, y0 = a % bs;
    for (int d = 0; d < 4; ++d) {
        const int dx = gomoku_dx(d), dy = gomoku_dy(d);
        int run = 1;
        for (int s = -1; s <= 1; s += 2)
            for (int k = 1;; ++k) {
                const int x = x0 + s * k * dx, y = y0 + s * k * dy;
                if (x < 0 || y < 0 || x >= bs || y >= bs || board[x * bs + y] != 1) break;
                ++run;
            }
        if (run >= 6) return true;
    }
    return false;
}

// Is the window of ws cells from (x, y) along d a four-shape of board + cand?  stones: its four black
// cells, 9 bits each (no per-lane array: an array indexed at run time would live in scratch memory).
AZ_GR_HD bool gomoku_four_shape(const uint8_t* board, int bs, int cand, int x, int y, int d, int ws, uint64_t& stones) {
    const int dx = gomoku_dx(d), dy = gomoku_dy(d);
    const int xe = x + (ws - 1) * dx, ye = y + (ws - 1) * dy;
    if (xe < 0 || xe >= bs || ye >= bs) return false;
    int nb = 0;
    uint64_t set = 0;
    for (int k = 0; k < ws; ++k) {
        const int a = (x + k * dx) * bs + y + k * dy, v = gomoku_at(board, cand, a);
        if (v == 2) return false;
        if (v == 1) {
            if (++nb > 4) return false;
            set = set << 9 | (uint64_t)a;
        }
    }
    if (nb != 4) return false;
    stones = set;
    const int fx = x - dx, fy = y - dy, lx = xe + dx, ly = ye + dy;
    if (fx >= 0 && fx < bs && fy >= 0 && gomoku_at(board, cand, fx * bs + fy) == 0) return true;
    return lx >= 0 && lx < bs && ly < bs && gomoku_at(board, cand, lx * bs + ly) == 0;
}

// Where the reference's scan (origin x, origin y, direction, window size, start index; up to seven
// cells from every origin) meets this window first, as one ordered integer.
AZ_GR_HD int gomoku_scan_key(int x, int y, int d, int ws) {
    const int back = d == 0 ? y : d == 1 ? x : d == 2 ? (x < y ? x : y) : 0;   // d == 3 runs towards smaller x
    const int s = back < 7 - ws ? back : 7 - ws;
    const int ox = x - s * gomoku_dx(d), oy = y - s * gomoku_dy(d);
    return ((((ox * 32 + oy) * 4 + d) * 8 + ws) * 8) + s;
}

// Any four-shape on the board as it stands, among the windows that start at cells first, first + stride, ...
AZ_GR_HD bool gomoku_any_four_shape(const uint8_t* board, int bs, int first, int stride) {
    uint64_t stones;
    for (int c = first; c < bs * bs; c += stride)
        for (int d = 0; d < 4; ++d)
            for (int ws = 5; ws <= 7; ++ws)
                if (gomoku_four_shape(board, bs, -1, c / bs, c % bs, d, ws, stones)) return true;
    return false;
}

// stones two four-shapes share
AZ_GR_HD int gomoku_common4(uint64_t p, uint64_t q) {
    int n = 0;
    for (int i = 0; i < 36; i += 9)
        for (int j = 0; j < 36; j += 9) n += ((p >> i) & 511) == ((q >> j) & 511);
    return n;
}

// Two or more four-shapes (as the reference counts them) on board + a.  base_fours: the board as it
// stands has a four-shape (true is always safe; false confines the scan to the windows through a).
AZ_GR_HD bool gomoku_double_four(const uint8_t* board, int bs, int a, bool base_fours) {
    const int ax = a / bs, ay = a % bs;
    // the windows looked at: w = (c * 4 + d) * 3 + ws - 5 over every start cell c, or
    // w = (k * 4 + d) * 3 + ws - 5 with a the window's k-th cell
    const int nw = (base_fours ? bs * bs : 7) * 12;
    uint64_t F = 0, S = 0;
    int fkey = 0x7fffffff, shapes = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int w = 0; w < nw; ++w) {
            const int ws = 5 + w % 3, d = (w / 3) % 4, c = w / 12;
            int x, y;
            if (base_fours) { x = c / bs; y = c % bs; }
            else {
                if (c >= ws) continue;
                x = ax - c * gomoku_dx(d); y = ay - c * gomoku_dy(d);
                if (x < 0 || x >= bs || y < 0) continue;
            }
            if (!gomoku_four_shape(board, bs, a, x, y, d, ws, S)) continue;
            if (pass == 0) {
                ++shapes;
                const int key = gomoku_scan_key(x, y, d, ws);
                if (key < fkey) { fkey = key; F = S; }
            } else if (gomoku_common4(F, S) < 3) return true;
        }
        if (shapes < 2) return false;
    }
    return false;
}

AZ_GR_HD bool gomoku_renju_forbidden(const uint8_t* board, int bs, int a, bool base_fours) {
    return gomoku_overline(board, bs, a) || gomoku_double_four(board, bs, a, base_fours);
}

// Is the 5-cell slice from (x, y) along d an open three .BBB. of board + cand?
AZ_GR_HD bool gomoku_open_three(const uint8_t* board, int bs, int cand, int x, int y, int d) {
    const int dx = gomoku_dx(d), dy = gomoku_dy(d);
    const int xe = x + 4 * dx, ye = y + 4 * dy;
    if (x < 0 || x >= bs || y < 0 || xe < 0 || xe >= bs || ye >= bs) return false;
    for (int k = 0; k < 5; ++k)
        if (gomoku_at(board, cand, (x + k * dx) * bs + y + k * dy) != (k == 0 || k == 4 ? 0 : 1)) return false;
    const int fx = x - dx, fy = y - dy, lx = xe + dx, ly = ye + dy;
    if (fx >= 0 && fx < bs && fy >= 0 && gomoku_at(board, cand, fx * bs + fy) == 1) return false;
    if (lx >= 0 && lx < bs && ly < bs && gomoku_at(board, cand, lx * bs + ly) == 1) return false;
    return true;
}

AZ_GR_HD bool gomoku_any_open_three(const uint8_t* board, int bs, int first, int stride) {
    for (int c = first; c < bs * bs; c += stride)
        for (int d = 0; d < 4; ++d)
            if (gomoku_open_three(board, bs, -1, c / bs, c % bs, d)) return true;
    return false;
}

// the stones of slices (x1, y1, d1) and (x2, y2, d2) come within Chebyshev distance 1
AZ_GR_HD bool gomoku_threes_connected(int x1, int y1, int d1, int x2, int y2, int d2) {
    for (int i = 1; i <= 3; ++i)
        for (int j = 1; j <= 3; ++j) {
            const int ex = x1 + i * gomoku_dx(d1) - x2 - j * gomoku_dx(d2), ey = y1 + i * gomoku_dy(d1) - y2 - j * gomoku_dy(d2);
            if (ex >= -1 && ex <= 1 && ey >= -1 && ey <= 1) return true;
        }
    return false;
}

// Two distinct connected open threes on board + a.  base_threes as base_fours above.
AZ_GR_HD bool gomoku_double_three(const uint8_t* board, int bs, int a, bool base_threes) {
    const int ax = a / bs, ay = a % bs;
    // slices: s = c * 4 + d over every start cell c, or s = (k - 1) * 4 + d with a the slice's k-th cell (k = 1..3)
    const int ns = (base_threes ? bs * bs : 3) * 4;
    for (int s1 = 0; s1 < ns; ++s1) {
        const int d1 = s1 % 4, c1 = s1 / 4;
        const int x1 = base_threes ? c1 / bs : ax - (c1 + 1) * gomoku_dx(d1), y1 = base_threes ? c1 % bs : ay - (c1 + 1) * gomoku_dy(d1);
        if (!gomoku_open_three(board, bs, a, x1, y1, d1)) continue;
        for (int s2 = s1 + 1; s2 < ns; ++s2) {
            const int d2 = s2 % 4, c2 = s2 / 4;
            const int x2 = base_threes ? c2 / bs : ax - (c2 + 1) * gomoku_dx(d2), y2 = base_threes ? c2 % bs : ay - (c2 + 1) * gomoku_dy(d2);
            if (gomoku_open_three(board, bs, a, x2, y2, d2) && gomoku_threes_connected(x1, y1, d1, x2, y2, d2)) return true;
        }
    }
    return false;
}

AZ_GR_HD bool gomoku_omok_forbidden(const uint8_t* board, int bs, int a, bool base_threes) {
    return gomoku_overline(board, bs, a) || gomoku_double_three(board, bs, a, base_threes);
}

// The rule in force forbids Black the empty cell a (Renju decides when both are set).
AZ_GR_HD bool gomoku_forbidden(const uint8_t* board, int bs, int renju, int omok, int a, bool base_shapes) {
    return renju ? gomoku_renju_forbidden(board, bs, a, base_shapes) : omok ? gomoku_omok_forbidden(board, bs, a, base_shapes) : false;
}
// the once-per-position fact gomoku_forbidden takes as base_shapes, over the strided share of the start cells
AZ_GR_HD bool gomoku_base_shapes(const uint8_t* board, int bs, int renju, int omok, int first, int stride) {
    return renju ? gomoku_any_four_shape(board, bs, first, stride) : omok ? gomoku_any_open_three(board, bs, first, stride) : false;
}

// Whole board: the forbidden cells of the side to move (player 1 black, 2 white) as a bit mask of
// (A + 63) / 64 words; returns the number of legal cells (empty and not forbidden).
AZ_GR_HD int gomoku_forbidden_mask(const uint8_t* board, int bs, int player, int renju, int omok, uint64_t* mask) {
    const int A = bs * bs;
    for (int w = 0; w < (A + 63) / 64; ++w) mask[w] = 0;
    const bool rules = player == 1 && (renju || omok);
    const bool base = rules && gomoku_base_shapes(board, bs, renju, omok, 0, 1);
    int legal = 0;
    for (int a = 0; a < A; ++a) {
        if (board[a]) continue;
        if (rules && gomoku_forbidden(board, bs, renju, omok, a, base)) mask[a >> 6] |= 1ull << (a & 63);
        else ++legal;
    }
    return legal;
}
