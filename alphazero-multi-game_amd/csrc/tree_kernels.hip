// tree_kernels.hip -- HIP kernels of the batched PUCT search (gfx950).
//
// One wavefront (64 lanes) per game.  Every fp32 operation that feeds the tree
// statistics is written in the reference's evaluation order and this file is
// compiled with -ffp-contract=off (no FMA contraction) and IEEE division/sqrt, so
// results are bit-identical to the reference CPU search:
//   k_select         ParallelMCTS::selectLeafWithPath + selectChildPuct + VL
//                    (src/mcts/parallel_mcts.cpp:456-563; mcts_node.cpp:61-119,168-196),
//                    leaf state (GomokuState::make_move, gomoku_state.cpp:681-722),
//                    terminal test (gomoku_rules.cpp:39-115), Zobrist hash (:620-656),
//                    TT lookup (transposition_table.cpp:44-84), feature planes (:207-258)
//   k_scan           deterministic compaction of the leaves that need the network
//   k_expand_backup  evaluator output -> softmax (torch_neural_network.cpp:296-316),
//                    TT store (:128-191), expandNodeWithPolicy (parallel_mcts.cpp:681-745),
//                    backpropagate(node, value, path) (:782-833)
//   k_select_action  getVisitCountDistribution (mcts_node.cpp:289-322), selectAction
//                    (parallel_mcts.cpp:987-1047), getRootValue (:1057-1063)
//   k_apply          makeMove + updateWithMove (parallel_mcts.cpp:1065-1108)
//   forbidden_mask_wave  Renju / Omok: the cells forbidden to Black at a leaf (gomoku_state.cpp:544-578
//                    with the predicates of gomoku_rules.h), for k_select's RULES instantiation
//   k_compact        subtree reuse: BFS copy of the new root's subtree into the other arena
//   k_noise          Dirichlet mix of addDirichletNoise (parallel_mcts.cpp:1158-1166)
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include "tree_kernels.h"
#include "leaf_planes.h"
#include "gomoku_rules.h"

namespace {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

// sum_{i < n} x[i] in index order from 0.0f (the reference's sequential float loops) by lane 0,
// 16 values per step read as four ds_read_b128 ahead of their adds; x is 16-B aligned and padded
// with +0.0f to a multiple of 16 entries (adding +0.0f to a non-negative sum changes no bit).
// Returns the sum on lane 0 only.
__device__ __forceinline__ float seq_sum_lds(const float* x, int n) {
    float s = 0.0f;
    const float4* q = reinterpret_cast<const float4*>(x);
    const int nq = (n + 15) / 16;
    if (nq <= 0) return s;
    // the next 16 values are read while the current 16 are added (the add chain, not the LDS
    // latency, is then the critical path)
    float4 a = q[0], b = q[1], c = q[2], d = q[3];
    for (int j = 0; j < nq; ++j) {
        float4 na = a, nb = b, nc = c, nd = d;
        if (j + 1 < nq) { na = q[4 * j + 4]; nb = q[4 * j + 5]; nc = q[4 * j + 6]; nd = q[4 * j + 7]; }
        s += a.x; s += a.y; s += a.z; s += a.w;
        s += b.x; s += b.y; s += b.z; s += b.w;
        s += c.x; s += c.y; s += c.z; s += c.w;
        s += d.x; s += d.y; s += d.z; s += d.w;
        a = na; b = nb; c = nc; d = nd;
    }
    return s;
}

// Cross-lane reductions without the LDS crossbar: DPP moves inside each 16-lane row (xor 1, xor 2,
// half-mirror, mirror: after the four steps every lane of a row holds the row's result), then the
// four rows' results read into scalars.  A __shfl_xor butterfly is six dependent ds_bpermute round
// trips; this is four DPP VALU steps and four v_readlane.  The combine is a total order, so the
// result does not depend on the combining order.
template <int CTRL>
__device__ __forceinline__ int dpp_mov(int v) { return __builtin_amdgcn_mov_dpp(v, CTRL, 0xF, 0xF, false); }
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_HALF_MIRROR = 0x141, DPP_MIRROR = 0x140;

// (r0 + i) mod ring for r0 < ring and i < ring (search creation checks ring >= NA)
__device__ __forceinline__ uint32_t ring_wrap(uint32_t x, int ring) {
    return x >= (uint32_t)ring ? x - (uint32_t)ring : x;
}

__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, __int_as_float(dpp_mov<DPP_XOR1>(__float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_mov<DPP_XOR2>(__float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_mov<DPP_HALF_MIRROR>(__float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_mov<DPP_MIRROR>(__float_as_int(v))));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

// first-max argmax over the wave: the largest score, ties to the smallest index (the reference's
// sequential first-max scan); returns wave-uniform (best, index)
__device__ __forceinline__ bool argmax_better(float s, int i, float bs, int bi) {
    return s > bs || (s == bs && i < bi);
}
template <int CTRL>
__device__ __forceinline__ void argmax_step(float& best, int& bi) {
    const float ob = __int_as_float(dpp_mov<CTRL>(__float_as_int(best)));
    const int oi = dpp_mov<CTRL>(bi);
    if (argmax_better(ob, oi, best, bi)) { best = ob; bi = oi; }
}
__device__ __forceinline__ void wave_argmax(float& best, int& bi) {
    argmax_step<DPP_XOR1>(best, bi);
    argmax_step<DPP_XOR2>(best, bi);
    argmax_step<DPP_HALF_MIRROR>(best, bi);
    argmax_step<DPP_MIRROR>(best, bi);
    float b = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), 0));
    int i = __builtin_amdgcn_readlane(bi, 0);
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        const float ob = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(best), 16 * r));
        const int oi = __builtin_amdgcn_readlane(bi, 16 * r);
        if (argmax_better(ob, oi, b, i)) { b = ob; i = oi; }
    }
    best = b; bi = i;
}
// v from a wave-uniform lane (v_readlane, no LDS round trip), returned in a VGPR: these values
// live across the descent, where scalar registers are the kernel's tight resource (spills)
__device__ __forceinline__ int lane_bcast(int v, int src) {
    const int x = __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(src));
    int r;
    asm("v_mov_b32 %0, %1" : "=v"(r) : "s"(x));
    return r;
}
__device__ __forceinline__ float lane_bcast(float v, int src) {
    return __int_as_float(lane_bcast(__float_as_int(v), src));
}
// lane src's 64-bit value as a wave-uniform (scalar) value; src wave-uniform
__device__ __forceinline__ uint64_t lane_read64(uint64_t v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive prefix sum across the wave
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// Diagnostic phase stamps (TreeDev.stamp_game >= 0, env AZ_TREE_STAMPS=<game>): [kernel][i] =
// s_memrealtime (100 MHz) in [0, 32), s_memtime (shader clock) in [32, 64); tools/tree_stamps.py.
__device__ unsigned long long g_tree_stamps[2][64];
__device__ __forceinline__ void tstamp(const TreeDev& t, int g, int k, int i) {
    if (g == t.stamp_game && threadIdx.x == 0) {
        g_tree_stamps[k][i] = __builtin_amdgcn_s_memrealtime();
        g_tree_stamps[k][32 + i] = __builtin_amdgcn_s_memtime();
    }
}

// GameResult (include/alphazero/core/igamestate.h:26-31)
enum { R_ONGOING = 0, R_DRAW = 1, R_WIN1 = 2, R_WIN2 = 3 };

// ParallelMCTS::convertToValue (parallel_mcts.cpp:973-985)
__device__ __forceinline__ float convert_value(int result, int player) {
    if (result == R_WIN1) return player == 1 ? 1.0f : -1.0f;
    if (result == R_WIN2) return player == 2 ? 1.0f : -1.0f;
    return 0.0f;
}

// count_direction / check_line_for_five (gomoku_rules.cpp:62-115): does the run of p's stones through cell a
// make five?  Lanes 0..7 walk the 8 rays (4 directions x 2 sides) at once, each capped
// at 5 cells (1 + min(L,5) + min(R,5) is 5 exactly when the run is 5, and >= 5 exactly when it is).
// Every lane of the wave must call it (wave-uniform arguments).
__device__ int five_at_wave(const uint8_t* board, int bs, int a, int p, int lane) {
    const int x0 = a / bs, y0 = a % bs;
    int run = 0;
    if (lane < 8) {
        const int d = lane >> 1, sg = (lane & 1) ? 1 : -1;
        const int dx = d == 0 ? 0 : 1, dy = d == 0 ? 1 : d == 1 ? 0 : d == 2 ? 1 : -1;   // {0,1},{1,0},{1,1},{1,-1}
        int x = x0 + sg * dx, y = y0 + sg * dy;
        while (run < 5 && x >= 0 && x < bs && y >= 0 && y < bs && board[x * bs + y] == p) {
            ++run; x += sg * dx; y += sg * dy;
        }
    }
    const int other = __shfl_xor(run, 1);
    const int len = board[a] == p ? 1 + run + other : -1;
    const bool win = lane < 8 && (lane & 1) == 0 && (p == 1 ? len == 5 : len >= 5);
    return __ballot(win) != 0ULL;
}

// Renju / Omok: the forbidden-cell mask of a Black-to-move position from its board in LDS, one wave
// per game (refresh_valid_moves_cache, gomoku_state.cpp:544-578, with the predicates of
// gomoku_rules.h).  First the wave shares one scan of the board as it stands (lane l: the windows
// that start at cells l, l + 64, ...): does it hold a four-shape (Renju) / an open three (Omok) at
// all?  Then every lane judges its own candidate cells -- without a standing shape only the windows
// through the candidate (84 of 5 to 7 cells, or 12 slices), else the whole board -- and a ballot
// per 64 cells is the mask word, written by lane 0.  Returns the legal count (empty cells not
// forbidden).  Every lane of the wave must call it; the board must be complete (after a barrier).
__device__ int forbidden_mask_wave(const TreeDev& t, const uint8_t* board, int lane, uint64_t* out) {
    const bool base = __ballot(gomoku_base_shapes(board, t.bs, t.renju, t.omok, lane, 64)) != 0ULL;
    int legal = 0;
    for (int c0 = 0; c0 < t.A; c0 += 64) {
        const int a = c0 + lane;
        const bool empty = a < t.A && board[a] == 0;
        const bool f = empty && gomoku_forbidden(board, t.bs, t.renju, t.omok, a, base);
        const unsigned long long m = __ballot(f);
        legal += __popcll(__ballot(empty)) - __popcll(m);
        if (lane == 0) out[c0 >> 6] = m;
    }
    return legal;
}

// getPuctScore (mcts_node.cpp:61-119).  parentDepth: depth of the node being selected
// FROM (root = 0); the reference negates Q exactly when that node is at depth 1 (:88-93).
__device__ __forceinline__ float puct_score(int visits, float W, int VL, float P, int parentDepth, int pN, int pVL,
                                            float pW, float cpuct, float fpu, float sqrtPV) {
    if (visits == 0) return FLT_MAX;
    float q = 0.0f;
    int act = visits - VL;
    if (act > 0) q = W / (float)act;
    if (parentDepth == 1) q = -q;
    if (act <= 0 && fpu > 0.0f) {
        int pa = pN - pVL;
        q = pa > 0 ? pW / (float)pa - fpu : -fpu;
    }
    float u = cpuct * P * sqrtPV / (1.0f + (float)visits);
    float div = 0.0f;
    if (visits < 5) div = 0.05f * (float)(5 - visits);
    return q + u + div;
}

// getProgressiveBiasScore (mcts_node.cpp:121-166): getAdjustedValue (:479-491) with getPuctScore's
// depth-1 negation, cPuct * prior * max(0.1, 1 / sqrt(1 + N)) and, for Go only, 0.02 * parentVisits /
// (1 + N); no FPU and no diversity term.  std::max(0.1f, x) keeps 0.1f when x is NaN (N < -1).
__device__ __forceinline__ float pbias_score(int visits, float W, int VL, float P, int parentDepth, int pN, float cpuct,
                                             bool go) {
    if (visits == 0) return FLT_MAX;
    const int act = visits - VL;
    float q = act <= 0 ? 0.0f : W / (float)act;
    if (parentDepth == 1) q = -q;
    const float r = 1.0f / sqrtf(1.0f + (float)visits);
    const float w = 0.1f < r ? r : 0.1f;
    const float e = cpuct * P * w;
    float gb = 0.0f;
    if (go) gb = 0.02f * (float)pN / (1.0f + (float)visits);
    return q + e + gb;
}
// getUcbScore (mcts_node.cpp:38-59): FLT_MAX unvisited, else the constant 0.5f + 1.5f * 0.5f *
// sqrt(1.0f) / (1.0f + 1.0f).  Every score exceeds -FLT_MAX, so selectChildUcb's random pick
// (parallel_mcts.cpp:589-599) is never reached and rng_ is not drawn.
__device__ __forceinline__ float ucb_score(int visits) { return visits == 0 ? FLT_MAX : 0.875f; }

// HashEvaluator key (oracle/ref_harness.cpp hash_eval)
__device__ uint64_t hash_eval_key(uint64_t zhash, const int* hist6) {
    uint64_t key = splitmix64(zhash ^ 0x5A17C0DEULL);
    for (int i = 0; i < 6; ++i) key = splitmix64(key + (uint64_t)(uint32_t)(hist6[i] + 2));
    return key;
}
__device__ __forceinline__ float hash_eval_p(uint64_t key, int a) {
    uint64_t r = splitmix64(key ^ ((uint64_t)(a + 1) * 0x9E3779B97F4A7C15ULL));
    return (float)(uint32_t)(r >> 40) * (1.0f / 16777216.0f);
}
__device__ __forceinline__ float hash_eval_v(uint64_t key) {
    uint64_t rv = splitmix64(key ^ 0x76A1ULL);
    return ((float)(int32_t)(uint32_t)(rv >> 40) - 8388608.0f) * (1.0f / 8388608.0f);
}

// std::mt19937 (libstdc++ _M_gen_rand / operator()) for RandomPolicyNetwork.
__device__ uint32_t mt_next(uint32_t* st) {
    uint32_t* x = st;
    uint32_t& p = st[624];
    if (p >= 624) {
        const uint32_t up = 0x80000000u, lo = 0x7fffffffu;
        for (int k = 0; k < 624 - 397; ++k) {
            uint32_t y = (x[k] & up) | (x[k + 1] & lo);
            x[k] = x[k + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        for (int k = 624 - 397; k < 623; ++k) {
            uint32_t y = (x[k] & up) | (x[k + 1] & lo);
            x[k] = x[k + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        uint32_t y = (x[623] & up) | (x[0] & lo);
        x[623] = x[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        p = 0;
    }
    uint32_t z = x[p++];
    z ^= (z >> 11) & 0xffffffffu;
    z ^= (z << 7) & 0x9d2c5680u;
    z ^= (z << 15) & 0xefc60000u;
    z ^= (z >> 18);
    return z;
}
// std::mt19937(seed) seeding (libstdc++ mersenne_twister_engine::seed)
__device__ void mt_seed(uint32_t* st, uint32_t seed) {
    st[0] = seed;
    for (int i = 1; i < 624; ++i) st[i] = 1812433253u * (st[i - 1] ^ (st[i - 1] >> 30)) + (uint32_t)i;
    st[624] = 624;
}
// uniform_real_distribution<float>(a, b) over generate_canonical<float, 24>
__device__ float mt_uniform(uint32_t* st, float a, float b) {
    float c = (float)mt_next(st) / 4294967296.0f;
    if (c >= 1.0f) c = __uint_as_float(0x3F7FFFFFu);   // nextafter(1, 0)
    return (c * (b - a)) + a;
}

struct GamePtrs {
    int* N; float* W; int* VL; float* P; int* first; int16_t* act; int16_t* cnt; uint8_t* flag;
};
__device__ __forceinline__ GamePtrs game_nodes(const Nodes& nd, size_t base) {
    GamePtrs p;
    p.N = nd.N + base; p.W = nd.W + base; p.VL = nd.VL + base; p.P = nd.P + base;
    p.first = nd.first + base; p.act = nd.act + base; p.cnt = nd.cnt + base; p.flag = nd.flag + base;
    return p;
}
// node i as a new node: no visits, no children, no move
__device__ __forceinline__ void node_clear(const GamePtrs& nd, int i) {
    nd.N[i] = 0; nd.W[i] = 0.0f; nd.VL[i] = 0; nd.P[i] = 0.0f;
    nd.first[i] = -1; nd.act[i] = -1; nd.cnt[i] = 0; nd.flag[i] = 0;
}

// Leaf state = root state + path moves: k_select and k_expand_backup build the Gomoku leaf board
// inline from the root board (loaded up front) and the path actions (sact[i], i = 1..depth):
// path cells are distinct, so the moves go down lane-parallel, and the Zobrist hash is the root
// hash XOR the moves' piece keys XOR the side-to-move keys (gomoku_state.cpp:620-656).

// The leaf record of a Gomoku leaf (leaf_planes.h): board, side to move, last six moves.
__device__ void write_leafrec(const TreeDev& t, int g, int lane, const uint8_t* board, const int* hist6, int player) {
    uint8_t* rec = t.leafrec + (size_t)g * AZ_REC_BYTES;
    for (int a = lane; a < t.A; a += 64) rec[a] = board[a];
    int* meta = reinterpret_cast<int*>(rec + AZ_REC_META);
    if (lane == 0) {
        meta[0] = player; meta[1] = -1;
#pragma unroll
        for (int i = 0; i < 6; ++i) meta[2 + i] = hist6[i];
    }
}

// ---------------------------------------------------------------------------
// Go (GoState(bs, t.komi, t.chinese, t.superko): go_state.cpp / go_rules.cpp).  Rules code runs
// on lane 0 over the game's LDS board (a few hundred LDS operations per move; the network
// forward of the same step is four orders of magnitude longer); per-point work is lane-parallel.
struct GoLds {
    int16_t list[AZ_MAXA];       // BFS list / stack
    int16_t mark[AZ_MAXA];       // visit stamps
    int16_t gid[AZ_MAXA];        // group label of every stone: the group's smallest point (-1 empty)
    int glib[AZ_MAXA];           // distinct liberties of the group labelled l
    uint64_t gxor[AZ_MAXA];      // XOR of the group's piece keys
    uint64_t phist[AZ_DMAX];     // position hashes pushed along the selection path
    uint64_t pkey[AZ_DMAX];      // piece key of the stone path move i places (go_build_leaf prefetch)
    int nph, stamp;
    int cap[2];                  // stones captured by black / white up to the leaf (root counters + the path's)
};

__device__ __forceinline__ int go_adj(int pos, int bs, int A, int* nb) {   // getAdjacentPositions (:800-816)
    const int x = pos % bs;
    int n = 0;
    if (pos >= bs) nb[n++] = pos - bs;
    if (x + 1 < bs) nb[n++] = pos + 1;
    if (pos + bs < A) nb[n++] = pos + bs;
    if (x > 0) nb[n++] = pos - 1;
    return n;
}

__device__ void go_clear_marks(GoLds& L, int A, int lane) {
    for (int a = lane; a < A; a += 64) L.mark[a] = -1;
    if (lane == 0) L.stamp = 0;
    __syncthreads();
}

// makeMove (go_state.cpp:192-257) on lane 0: place, remove libertyless opponent groups (only
// groups adjacent to the new stone can have none), ko point, stones hash.  Returns 1 when the
// move pushes a position (stone moves), 0 for a pass.
// key (optional): the placed stone's piece key, already loaded (go_build_leaf prefetches a path's keys)
// cap (optional): capture counters {by black, by white}; the mover's grows by the stones removed
__device__ int go_play_seq(const TreeDev& t, uint8_t* b, GoLds& L, int a, int p, int& ko, int& passes, uint64_t& bh,
                           const uint64_t* key = nullptr, int* cap = nullptr) {
    const int bs = t.bs, A = t.A;
    if (a < 0) { ++passes; ko = -1; return 0; }
    passes = 0;
    b[a] = (uint8_t)p;
    bh ^= key ? *key : t.zpiece[(size_t)(p - 1) * A + a];
    const int opp = 3 - p;
    int ngroups = 0, nstones = 0, last = -1;
    int nb[4];
    const int k = go_adj(a, bs, A, nb);
    const int base = L.stamp;          // stamps of this call are > base
    for (int j = 0; j < k; ++j) {
        const int s0 = nb[j];
        if (b[s0] != opp || L.mark[s0] > base) continue;   // empty / own / group already examined
        const int st = ++L.stamp;
        int n = 0;
        L.list[n++] = (int16_t)s0;
        L.mark[s0] = (int16_t)st;
        bool lib = false;
        for (int i = 0; i < n; ++i) {
            int nb2[4];
            const int k2 = go_adj(L.list[i], bs, A, nb2);
            for (int q = 0; q < k2; ++q) {
                const int c = nb2[q];
                if (b[c] == 0) lib = true;
                else if (b[c] == opp && L.mark[c] != st) { L.mark[c] = (int16_t)st; L.list[n++] = (int16_t)c; }
            }
        }
        if (!lib) {
            for (int i = 0; i < n; ++i) {
                const int c = L.list[i];
                b[c] = 0;
                bh ^= t.zpiece[(size_t)(opp - 1) * A + c];
            }
            ++ngroups;
            nstones += n;
            last = L.list[0];
        }
    }
    ko = (ngroups == 1 && nstones == 1) ? last : -1;
    if (cap) cap[p - 1] += nstones;
    return 1;
}

// updateHash (go_state.cpp:846-877)
__device__ __forceinline__ uint64_t go_hash(const TreeDev& t, uint64_t bh, int player, int ko) {
    uint64_t h = bh ^ t.zplayer[player - 1];
    if (ko >= 0) h ^= t.zko[ko];
    return h ^ t.zconst;
}

// Piece keys of a wave's points (point a = lane + 64 i): of the stone on it (st) and of a stone of
// `player` on an empty point (pl, the superko candidates) -- all loads issued at once, one L2 round
// trip ahead of go_groups / go_legal, whose per-point loops otherwise waited for one per chunk.
constexpr int GO_PTS = (AZ_MAXA + 63) / 64;
struct GoKeys {
    uint64_t st[GO_PTS], pl[GO_PTS];
};
__device__ __forceinline__ void go_keys(const TreeDev& t, const uint8_t* b, int player, int lane, GoKeys& K) {
    const int A = t.A;
#pragma unroll
    for (int i = 0; i < GO_PTS; ++i) {
        const int a = lane + 64 * i;
        const int c = a < A ? b[a] : 0;
        K.st[i] = c ? t.zpiece[(size_t)(c - 1) * A + a] : 0ULL;
        K.pl[i] = (a < A && !c) ? t.zpiece[(size_t)(player - 1) * A + a] : 0ULL;
    }
}

// Every group of the board (visible to all threads after the call): label gid = the group's
// smallest point index (-1 on empty points), glib[label] its distinct liberties and, with keys (one
// wave: tid = lane, nthr = 64), gxor[label] the XOR of its piece keys.  Thread-parallel over the
// points (tid of nthr): min-label propagation with pointer jumping over same-colour neighbours until
// no label moves, then one liberty per (empty point, adjacent group) pair and one key per stone --
// integers, so the same results as a sequential flood fill (which held the lane-0 chain of dependent
// LDS / L2 accesses here).  The leaf record and the dataset planes need the liberties only.
__device__ void go_groups(const TreeDev& t, const uint8_t* b, GoLds& L, int tid, int nthr, const GoKeys* K = nullptr) {
    const int bs = t.bs, A = t.A;
    for (int a = tid; a < A; a += nthr) {
        L.gid[a] = b[a] ? (int16_t)a : (int16_t)-1;
        L.glib[a] = 0;
        if (K) L.gxor[a] = 0;
    }
    __syncthreads();
    for (;;) {
        bool moved = false;
        for (int a = tid; a < A; a += nthr) {
            const int c = b[a];
            if (!c) continue;
            int m = L.gid[a];
            int nb[4];
            const int k = go_adj(a, bs, A, nb);
            for (int q = 0; q < k; ++q)
                if (b[nb[q]] == c) m = min(m, (int)L.gid[nb[q]]);
            m = min(m, (int)L.gid[m]);                    // jump to the label's own label
            if (m < L.gid[a]) { L.gid[a] = (int16_t)m; moved = true; }
        }
        if (!__syncthreads_or(moved)) break;
    }
    if (K) {
#pragma unroll
        for (int i = 0; i < GO_PTS; ++i) {
            const int a = tid + 64 * i;
            if (a < A && b[a]) atomicXor(reinterpret_cast<unsigned long long*>(&L.gxor[L.gid[a]]), K->st[i]);
        }
    }
    for (int a = tid; a < A; a += nthr) {
        if (b[a]) continue;
        int nb[4], seen[4], ns = 0;
        const int k = go_adj(a, bs, A, nb);
        for (int q = 0; q < k; ++q) {
            if (!b[nb[q]]) continue;
            const int gl = L.gid[nb[q]];
            bool dup = false;
            for (int r = 0; r < ns; ++r) dup |= seen[r] == gl;
            if (!dup) { seen[ns++] = gl; atomicAdd(&L.glib[gl], 1); }
        }
    }
    __syncthreads();
}

// GoRules::getTerritoryOwnership + calculateScores (go_rules.cpp:211-361) -> GameResult of a finished
// game (go_state.cpp:295-312).  Chinese rules: stones + territory; Japanese: territory + prisoners,
// each side credited with the OPPONENT's captures as the reference does (:336-353); then the komi.
// cap: stones captured by black / white.  Lane 0.
__device__ int go_result_seq(const TreeDev& t, const uint8_t* b, GoLds& L, const int* cap) {
    const int bs = t.bs, A = t.A;
    float bsc = 0.0f, wsc = 0.0f;
    const int st = ++L.stamp;
    if (t.chinese) {
        for (int p0 = 0; p0 < A; ++p0) {
            if (b[p0] == 1) { bsc += 1.0f; continue; }
            if (b[p0] == 2) { wsc += 1.0f; continue; }
        }
    }
    for (int p0 = 0; p0 < A; ++p0) {
        if (b[p0] != 0 || L.mark[p0] == st) continue;
        int n = 0;
        bool tb = false, tw = false;
        L.list[n++] = (int16_t)p0;
        L.mark[p0] = (int16_t)st;
        for (int i = 0; i < n; ++i) {
            int nb[4];
            const int k = go_adj(L.list[i], bs, A, nb);
            for (int q = 0; q < k; ++q) {
                const int e = nb[q];
                if (b[e] == 0) { if (L.mark[e] != st) { L.mark[e] = (int16_t)st; L.list[n++] = (int16_t)e; } }
                else if (b[e] == 1) tb = true;
                else tw = true;
            }
        }
        if (tb && !tw) bsc += (float)n;
        else if (tw && !tb) wsc += (float)n;
    }
    if (!t.chinese) { bsc += (float)cap[1]; wsc += (float)cap[0]; }
    wsc += t.komi;
    if (bsc > wsc) return R_WIN1;
    if (wsc > bsc) return R_WIN2;
    return R_DRAW;
}

// Leaf state of a Go game = root state + path moves (lane 0), with the position hashes the path
// pushes (for positional superko at expansion).
__device__ void go_build_leaf(const TreeDev& t, int g, int lane, const int* sact, int depth,
                              uint8_t* board, GoLds& L, int* hist6, int& player, int& ko, int& passes, uint64_t& bh,
                              uint64_t& hash) {
    const int A = t.A;
    const uint8_t* rb = t.rboard + (size_t)g * A;
    for (int a = lane; a < A; a += 64) board[a] = rb[a];
    go_clear_marks(L, A, lane);
    {   // the piece keys of the stones the path places, loaded lane-parallel ahead of the replay
        const int p0 = t.rplayer[g];
        for (int i = 1 + lane; i <= depth; i += 64) {
            const int a = sact[i];
            const int p = (i & 1) ? p0 : 3 - p0;
            L.pkey[i] = a >= 0 ? t.zpiece[(size_t)(p - 1) * A + a] : 0ULL;
        }
    }
    __syncthreads();
    if (lane == 0) {
        int p = t.rplayer[g], k = t.rko[g], ps = t.rpass[g];
        uint64_t h = t.rhash[g];
        int nph = 0;
        int cap[2] = {t.rcap[2 * g], t.rcap[2 * g + 1]};
        for (int i = 1; i <= depth; ++i) {
            const int a = sact[i];
            if (go_play_seq(t, board, L, a, p, k, ps, h, &L.pkey[i], cap)) L.phist[nph++] = go_hash(t, h, p, k);
            p = 3 - p;
        }
        L.nph = nph;
        L.cap[0] = cap[0]; L.cap[1] = cap[1];
        L.list[0] = (int16_t)p; L.list[1] = (int16_t)k; L.list[2] = (int16_t)ps;
        L.gxor[0] = h;
    }
    __syncthreads();
    player = L.list[0]; ko = L.list[1]; passes = L.list[2]; bh = L.gxor[0];
    __syncthreads();
    hash = go_hash(t, bh, player, ko);
    for (int i = 0; i < 6; ++i) {
        if (i < depth) hist6[i] = sact[depth - i];
        else hist6[i] = t.rhist[g * 6 + (i - depth)];
    }
}

// The selected Go leaf's position for its expansion (AZ_GOLEAF_BYTES per game): the expansion reads
// it back in one round trip instead of replaying the path's moves, captures and hashes on lane 0 a
// second time.  go_build_leaf must have run (board, L.phist / L.nph in LDS).
__device__ void go_store_leaf(const TreeDev& t, int g, int lane, const uint8_t* board, const GoLds& L, int player,
                              int ko, int passes, uint64_t bh) {
    uint8_t* dst = t.goleaf + (size_t)g * AZ_GOLEAF_BYTES;
    for (int a = lane; a < t.A; a += 64) dst[a] = board[a];
    const int nph = L.nph;
    uint64_t* ph = reinterpret_cast<uint64_t*>(dst + 416);
    for (int r = lane; r < nph; r += 64) ph[r] = L.phist[r];
    if (lane == 0) {
        int* meta = reinterpret_cast<int*>(dst + 384);
        meta[0] = player; meta[1] = ko; meta[2] = passes; meta[3] = nph;
        *reinterpret_cast<uint64_t*>(dst + 400) = bh;
    }
}
// go_build_leaf's results from the stored leaf state (same values: the replay is deterministic)
// q: the leaf slot the state was stored under (the game itself without leaf parallelism)
__device__ void go_load_leaf(const TreeDev& t, int g, int q, int lane, const int* sact, int depth, uint8_t* board, GoLds& L,
                             int* hist6, int& player, int& ko, int& passes, uint64_t& bh, uint64_t& hash) {
    const int A = t.A;
    const uint8_t* src = t.goleaf + (size_t)q * AZ_GOLEAF_BYTES;
    const int* meta = reinterpret_cast<const int*>(src + 384);
    player = meta[0]; ko = meta[1]; passes = meta[2];
    const int nph = meta[3];
    bh = *reinterpret_cast<const uint64_t*>(src + 400);
    for (int a = lane; a < A; a += 64) board[a] = src[a];
    const uint64_t* ph = reinterpret_cast<const uint64_t*>(src + 416);
    for (int r = lane; r < nph; r += 64) L.phist[r] = ph[r];
    go_clear_marks(L, A, lane);
    if (lane == 0) L.nph = nph;
    __syncthreads();
    hash = go_hash(t, bh, player, ko);
    for (int i = 0; i < 6; ++i) {
        if (i < depth) hist6[i] = sact[depth - i];
        else hist6[i] = t.rhist[g * 6 + (i - depth)];
    }
}

// The leaf record of a Go leaf (leaf_planes.h; planes of go_state.cpp:338-420): board, side to
// move, ko point and min(10, group liberties) per stone (go_groups() must have run).
__device__ void go_write_leafrec(const TreeDev& t, int g, int lane, const uint8_t* b, const GoLds& L, int player, int ko) {
    uint8_t* rec = t.leafrec + (size_t)g * AZ_REC_BYTES;
    for (int a = lane; a < t.A; a += 64) {
        rec[a] = b[a];
        rec[AZ_REC_LIBS + a] = b[a] ? (uint8_t)min(10, (int)L.glib[L.gid[a]]) : 0;
    }
    int* meta = reinterpret_cast<int*>(rec + AZ_REC_META);
    if (lane == 0) meta[0] = player;
    if (lane == 1) meta[1] = ko;
    if (lane < 6) meta[2 + lane] = -1;
}

// getLegalMoves (go_state.cpp:116-160): pass, then every empty non-ko point that is not suicide
// (GoRules::isSuicidalMove) and whose resulting position -- same side to move, the old ko point --
// is not in position_history_ (root history + the path's pushes; enforce_superko only).  Needs go_groups().
// rh[0, nr): the position history the candidates are held against (go_legal: the game's root history)
__device__ __forceinline__ int go_legal_hist(const TreeDev& t, const uint64_t* rh, const int nr, int lane, const uint8_t* b,
                                             const GoLds& L, int player, int ko, uint64_t bh, int* legal, const GoKeys& K) {
    const int A = t.A, bs = t.bs;
    const int opp = 3 - player;
    const uint64_t tail = t.zplayer[player - 1] ^ (ko >= 0 ? t.zko[ko] : 0ULL) ^ t.zconst;
    if (lane == 0) legal[0] = -1;
    int n = 1;
    const uint64_t hv0 = lane < nr ? rh[lane] : 0ULL;      // the root history's first 64 positions, one per lane
#pragma unroll
    for (int ci = 0; ci < GO_PTS; ++ci) {
        const int c0 = 64 * ci;
        if (c0 >= A) break;
        const int a = c0 + lane;
        bool ok = a < A && b[a] == 0 && a != ko;
        uint64_t hc = 0;                                    // the candidate's resulting position
        if (ok) {
            int nb[4];
            const int k = go_adj(a, bs, A, nb);
            bool alive = false;
            int capg[4], nc = 0;
            uint64_t h = bh ^ K.pl[ci];
            for (int q = 0; q < k; ++q) {
                const int e = nb[q];
                const int v = b[e];
                if (v == 0) { alive = true; continue; }
                const int gi = L.gid[e];
                if (v == player) { if (L.glib[gi] >= 2) alive = true; continue; }
                if (L.glib[gi] == 1) {                // its only liberty is a: captured
                    bool dup = false;
                    for (int r = 0; r < nc; ++r) dup |= capg[r] == gi;
                    if (!dup) { capg[nc++] = gi; h ^= L.gxor[gi]; }
                }
            }
            ok = alive || nc > 0;
            hc = h ^ tail;
        }
        // positional superko, wave-uniform: every candidate against the root history (64 entries per
        // coalesced load, broadcast lane by lane -- not one dependent L2 round trip per entry) and
        // the path's pushes (LDS)
        if (t.superko && __ballot(ok)) {
            for (int r0 = 0; r0 < nr; r0 += 64) {
                const uint64_t hv = r0 == 0 ? hv0 : (r0 + lane < nr ? rh[r0 + lane] : 0ULL);
                const int m = min(64, nr - r0);
                for (int j = 0; j < m; ++j) ok = ok && lane_read64(hv, j) != hc;
            }
            for (int r = 0; r < L.nph; ++r) ok = ok && L.phist[r] != hc;
        }
        const unsigned long long m = __ballot(ok);
        if (ok) legal[n + __popcll(m & ((1ULL << lane) - 1ULL))] = a;
        n += __popcll(m);
    }
    __syncthreads();
    return n;
}
__device__ int go_legal(const TreeDev& t, int g, int lane, const uint8_t* b, const GoLds& L, int player, int ko,
                        uint64_t bh, int* legal, const GoKeys& K) {
    return go_legal_hist(t, t.rposh + (size_t)g * t.hmax, t.superko ? t.rnposh[g] : 0, lane, b, L, player, ko, bh, legal, K);
}

}  // namespace

// ---------------------------------------------------------------------------
// K1: selection + virtual loss + leaf classification (+ planes for the network).
// K1.  IT = child records per lane per level (IT * 64 >= the action space).  Every level of the
// descent is ONE dependent round trip to memory: each lane loads all IT of its child records in
// full (N, W, VL, P and the child's own header first / cnt / flag / act) before the PUCT scores,
// and the winner's record is broadcast from its lane, so the next level needs no header load.
// What an expansion hands to the selection that follows it in the same wave (k_expand_select):
// the root's statistics after the backup and its header (first child, count, flag: from the
// root-header record k_select keeps, or as the expansion just set them), so the selection starts
// its descent without a round trip for the root.
struct RootHint {
    int valid;                   // the expansion's backup ran: the fields below are current
    int N, VL; float W;
    int first, cnt, flag;
};

// LDS of the selection and of the expansion: separate structs so that the fused k_expand_select
// overlays them (a union: the selection starts after the expansion's last LDS access and a block
// barrier) and shares one GoLds -- 12.3 KB per block instead of 21.1 KB, so 13 blocks fit a CU and
// C3's 2048 one-wave blocks (8 per CU) run in one round instead of two (7 per CU fitted at 21.1 KB)
struct SelLds {
    uint8_t board[AZ_MAXA];
    int spath[AZ_DMAX];
    int sact[AZ_DMAX];
    int sN[AZ_DMAX], sVL[AZ_DMAX];
    float sW[AZ_DMAX];
};
constexpr int EXP_NPAD = ((AZ_MAXNA + 63) / 64) * 64;   // pol / lp padded with +0.0f for seq_sum_lds
struct ExpLds {
    __attribute__((aligned(16))) float pol[EXP_NPAD];
    __attribute__((aligned(16))) float lp[EXP_NPAD];
    uint8_t board[AZ_MAXA];
    int spath[AZ_DMAX];
    int sact[AZ_DMAX];
    int legal[AZ_MAXNA];
    float s_scalar[2];
};

// OPT: the search options of az_search_cfg (TreeDev sel / max_depth / use_wid ...) are in force; the
// default instantiation (OPT = false) is the plain PUCT search and reads none of them.
// RULES: Renju / Omok (TreeDev renju / omok) are in force: a Black-to-move leaf gets its forbidden-cell
// mask (t.gforb, which the expansion reads) and is a DRAW when no legal cell is left (is_stalemate).
// WAVE: descent wj of a wave of leaf-parallel descents (k_wave_select, handle setting leaves = wK > 1): its
// scratch is leaf slot q = g * wK + wj.  The descent leaves its virtual loss on the tree for its wave-mates and
// only classifies the leaf for the batch (terminal / needs the network): the TT probe reads the entry without
// counting a lookup or a visit -- the completion (expand_game's WAVE instantiation) probes again, in descent
// order, against the table and the leaf as its mates' completions left them.
template <int IT, bool OPT, bool RULES, bool WAVE = false>
__device__ __forceinline__ void select_game(const TreeDev& t, int mode, const RootHint* hint, SelLds& SL, GoLds& gl,
                                            int wj = 0, int wK = 1) {
    const int g = blockIdx.x;
    const int q = WAVE ? g * wK + wj : g;             // leaf slot: the index of the per-step scratch
    const int lane = threadIdx.x;
    auto& board = SL.board;
    auto& spath = SL.spath;
    auto& sact = SL.sact;
    auto& sN = SL.sN;
    auto& sVL = SL.sVL;
    auto& sW = SL.sW;
    const bool go = t.game == GAME_GO;
    if (g >= t.G) return;
    // per-game inputs that do not depend on the tree, loaded before anything waits
    constexpr int BK = (AZ_MAXA + 63) / 64;
    const int A = t.A;
    const int active = t.active[g];
    const int root = t.rnode[g];
    uint8_t rb[BK];
#pragma unroll
    for (int k = 0; k < BK; ++k) rb[k] = lane + 64 * k < A ? t.rboard[(size_t)g * A + lane + 64 * k] : 0;
    const int p0 = t.rplayer[g], rstones = t.rstones[g], gres = t.gresult[g];
    const uint64_t rhash = t.rhash[g], zpl0 = t.zplayer[0], zpl1 = t.zplayer[1];
    const int rhist = lane < 6 ? t.rhist[g * 6 + lane] : -1;
    long long* cnt = t.cnt + (size_t)g * AZ_NCNT;
    const long long c_look = cnt[CNT_LOOKUPS], c_hits = cnt[CNT_HITS], c_bytes = cnt[CNT_BYTES_SEL];
    tstamp(t, g, 0, 0);
    if (!active) {
        if (lane == 0) { t.lstatus[q] = ST_NONE; t.need_eval[q] = 0; }
        return;
    }
    const size_t base = (size_t)g * t.ncap;
    GamePtrs nd = game_nodes(t.nd, base);
    uint64_t zx = 0;             // XOR of the path moves' piece keys (Gomoku), loaded level by level
    int depth = 0;
    int node = root;
    int status = ST_NONE;
    float value = 0.0f;
    long long scanned = 0;       // child records read by the PUCT scans (25 B each)
    int widened = 0;             // children progressive widening decremented and wrote back (12 B each)
    const bool hv = hint && hint->valid;
    int4 rhdr0 = int4{0, 0, 0, 0};
    uint8_t nflag = hv ? (uint8_t)hint->flag : nd.flag[root];   // flag of the current node (the leaf's after the descent)

    if (mode != MODE_SIM) {
        // Root expansion: expandNode (noise) / search() root branch.
        if ((nflag & (FL_EXPANDED | FL_TERMINAL)) || gres != R_ONGOING) {
            if (lane == 0) { t.lstatus[q] = ST_NONE; t.need_eval[q] = 0; }
            return;
        }
        if (lane == 0) spath[0] = root;
    } else {
        // selectLeafWithPath: VL on the root, then PUCT descent.
        int rN = hv ? hint->N : nd.N[root], rVL = hv ? hint->VL : nd.VL[root];
        float rW = hv ? hint->W : nd.W[root];
        int fc = hv ? hint->first : nd.first[root], nc = hv ? hint->cnt : nd.cnt[root];
        rhdr0 = int4{fc, nc, (int)nflag, 0};            // the root's header (its flag as it ends below)
        rN += t.vl; rVL += t.vl; rW = rW - (float)t.vl;           // addVirtualLoss (root, first)
        if (lane == 0) spath[0] = root;
        tstamp(t, g, 0, 1);
        int pN = rN, pVL = rVL;
        float pW = rW;
        const int maxd = OPT ? t.max_depth : 1000;      // maxSearchDepth (parallel_mcts.cpp:469)
        while (true) {
            if (!(nflag & FL_EXPANDED) || (nflag & FL_TERMINAL) || depth >= maxd || nc <= 0) break;
            scanned += nc;
            const float sq = sqrtf((float)pN);
            // getProgressiveWideningCount(pN, nc) (parallel_mcts.cpp:1299-1313) from the host's table,
            // loaded with the level's child records: 1 at pN <= 0, every child past a complete table
            int wcount = nc;
            if (OPT && t.use_wid) {
                if (pN <= 0) wcount = 1;
                else if (pN < t.wid_len) wcount = min(t.wid_tab[pN], nc);
                else if (!t.wid_complete && lane == 0) atomicOr(t.err, ERR_WIDEN);
            }
            int cN[IT], cVL[IT], cF[IT], cC[IT], cA[IT], cFl[IT];
            float cW[IT], cP[IT];
#pragma unroll
            for (int k = 0; k < IT; ++k) {                 // all loads of the level before any use
                const int c = fc + min(lane + 64 * k, nc - 1);
                cN[k] = nd.N[c]; cW[k] = nd.W[c]; cVL[k] = nd.VL[c]; cP[k] = nd.P[c];
                cF[k] = nd.first[c]; cC[k] = nd.cnt[c]; cA[k] = nd.act[c]; cFl[k] = nd.flag[c];
            }
            int lim = nc;                                  // children the argmax looks at
            bool dec[IT];
            if (OPT && t.use_wid) {
                // selectLeafWithPath (:471-485): every child i >= count that has visitCount < 1 gets
                // addVirtualLoss(-virtualLoss) -- N -= vl, VL -= vl, W - (float)(-vl) -- on every pass,
                // before the children are scored; the scan stops at count only from minVisitsForWidening
                // parent visits on (:545-552), so below that a child just decremented can be picked
                const bool cut = nc > 1 && wcount < nc;
#pragma unroll
                for (int k = 0; k < IT; ++k) {
                    const int i = lane + 64 * k;
                    dec[k] = cut && i < nc && i >= wcount && cN[k] < 1;
                    if (dec[k]) { cN[k] -= t.vl; cVL[k] -= t.vl; cW[k] = cW[k] - (float)(-t.vl); }
                }
                if (pN >= t.wid_min) lim = wcount;
            }
            float best = -FLT_MAX;
            int bi = INT_MAX, bk = 0;
#pragma unroll
            for (int k = 0; k < IT; ++k) {
                const int i = lane + 64 * k;
                if (i < lim) {
                    float s;
                    if (OPT && t.sel == SEL_UCB) s = ucb_score(cN[k]);
                    else if (OPT && t.sel == SEL_PROGRESSIVE_BIAS) s = pbias_score(cN[k], cW[k], cVL[k], cP[k], depth, pN, t.cpuct, go);
                    else s = puct_score(cN[k], cW[k], cVL[k], cP[k], depth, pN, pVL, pW, t.cpuct, t.fpu, sq);
                    if (s > best) { best = s; bi = i; bk = k; }
                }
            }
            int bN = cN[0], bVL = cVL[0], bF = cF[0], bC = cC[0], bA = cA[0], bFl = cFl[0];
            float bW = cW[0];
#pragma unroll
            for (int k = 1; k < IT; ++k)
                if (bk == k) { bN = cN[k]; bVL = cVL[k]; bF = cF[k]; bC = cC[k]; bA = cA[k]; bFl = cFl[k]; bW = cW[k]; }
            wave_argmax(best, bi);
            if (OPT && t.use_wid) {
                // the decremented children back to the tree, lane-parallel; the selected one is a path
                // node: its statistics are written with the virtual loss below
#pragma unroll
                for (int k = 0; k < IT; ++k) {
                    const int i = lane + 64 * k;
                    const bool w = dec[k] && i != bi;
                    if (w) { const int c = fc + i; nd.N[c] = cN[k]; nd.VL[c] = cVL[k]; nd.W[c] = cW[k]; }
                    widened += __popcll(__ballot(w));
                }
            }
            if (bi == INT_MAX) break;
            if (depth + 1 >= AZ_DMAX) { if (lane == 0) atomicOr(t.err, ERR_PATH); break; }
            const int src = bi & 63;
            pN = lane_bcast(bN, src); pVL = lane_bcast(bVL, src); pW = lane_bcast(bW, src);
            nflag = (uint8_t)lane_bcast(bFl, src);
            const int act = lane_bcast(bA, src);
            node = fc + bi;
            fc = lane_bcast(bF, src); nc = lane_bcast(bC, src);
            ++depth;
            // the node's statistics as loaded: its virtual loss below needs no second read
            if (lane == 0) { spath[depth] = node; sact[depth] = act; sN[depth] = pN; sVL[depth] = pVL; sW[depth] = pW; }
            // its piece key lands while the next level's records load (no extra round trip)
            if (!go) zx ^= t.zpiece[(size_t)((depth & 1) ? p0 - 1 : 2 - p0) * A + act];
        }
        tstamp(t, g, 0, 2);
        // addVirtualLoss on every path node, root a second time (parallel_mcts.cpp:293-295), on the
        // statistics the descent loaded (the wave is the tree's only writer); the post-VL values also
        // go to the path record (pstat), which the expansion's backup reads instead of the nodes
        // (WAVE: no path record -- the nodes change under the wave-mates' descents and completions, so
        // the completion reads them again)
        int4* ps = t.pstat + (size_t)g * AZ_DMAX;
        if (lane == 0) {
            rN += t.vl; rVL += t.vl; rW = rW - (float)t.vl;
            nd.N[root] = rN; nd.VL[root] = rVL; nd.W[root] = rW;
            if (!WAVE) ps[0] = int4{rN, rVL, __float_as_int(rW), depth == 0 ? (int)nflag : 0};
        }
        __syncthreads();
        for (int i = 1 + lane; i <= depth; i += 64) {
            const int n = spath[i];
            const int N = sN[i] + t.vl, VL = sVL[i] + t.vl;
            const float W = sW[i] - (float)t.vl;
            nd.N[n] = N; nd.VL[n] = VL; nd.W[n] = W;
            if (!WAVE) ps[i] = int4{N, VL, __float_as_int(W), i == depth ? (int)nflag : 0};   // .w: the leaf's flag
        }
    }
    __syncthreads();

    int hist6[6];
    int player, stones = 0;
    uint64_t hash;
    int gko = -1, gpass = 0;
    uint64_t gbh = 0;
    if (go) {
        go_build_leaf(t, g, lane, sact, depth, board, gl, hist6, player, gko, gpass, gbh, hash);
        go_store_leaf(t, q, lane, board, gl, player, gko, gpass, gbh);
    } else {
        // leaf board = root board + path moves (distinct cells, lane-parallel); hash = root hash ^
        // the path's piece keys ^ the side-to-move keys (build_leaf, on registers already loaded)
#pragma unroll
        for (int k = 0; k < BK; ++k) if (lane + 64 * k < A) board[lane + 64 * k] = rb[k];
        __syncthreads();
        for (int i = 1 + lane; i <= depth; i += 64) board[sact[i]] = (uint8_t)((i & 1) ? p0 : 3 - p0);
        player = (depth & 1) ? 3 - p0 : p0;
        stones = rstones + depth;
        hash = rhash ^ zx ^ (p0 == 1 ? zpl0 : zpl1) ^ (player == 1 ? zpl0 : zpl1);
        for (int i = 0; i < 6; ++i) hist6[i] = i < depth ? sact[depth - i] : lane_bcast(rhist, i - depth);
        __syncthreads();
    }
    int nlegal = 1;              // RULES: legal cells of a Black-to-move leaf that is not known to be over
    if (RULES && !go && player == 1 && !(nflag & FL_TERMINAL))
        nlegal = forbidden_mask_wave(t, board, lane, t.gforb + (size_t)q * AZ_FORB_WORDS);
    tstamp(t, g, 0, 3);
    const int leaf = node;
    int store = 0;
    uint64_t ref = 0;
    int hslot = 0;
    bool wskip = false;                 // WAVE: the leaf cannot need the evaluator (no batch row)
    long long d_look = 0, d_hits = 0;   // counter increments (written once at the end)

    if (mode == MODE_SIM) {
        const uint8_t f = nflag;
        int result = R_ONGOING;
        if (f & FL_TERMINAL) {
            status = ST_TERMINAL;
            value = convert_value((f >> 2) & 3, player);
        } else {
            if (depth == 0) {
                result = gres;
            } else if (go) {
                // GoState::isTerminal: two consecutive passes; area score (go_state.cpp:291-312)
                if (gpass >= 2) {
                    int r = 0;
                    if (lane == 0) r = go_result_seq(t, board, gl, gl.cap);
                    result = lane_bcast(r, 0);
                }
            } else {
                const int a = sact[depth];
                if (five_at_wave(board, t.bs, a, 3 - player, lane)) result = (3 - player) == 1 ? R_WIN1 : R_WIN2;
                else if (stones >= t.A) result = R_DRAW;
                else if (RULES && nlegal == 0) result = R_DRAW;   // Black has no legal cell (is_stalemate)
            }
            if (result != R_ONGOING) {
                status = ST_TERMINAL;
                value = convert_value(result, player);
                if (lane == 0) nd.flag[leaf] = (uint8_t)(f | FL_TERMINAL | (result << 2));
                if (depth == 0) rhdr0.z = (int)(uint8_t)(f | FL_TERMINAL | (result << 2));
            } else if (f & FL_EXPANDED) {
                // an expanded leaf: a childless node (releaseMemory pruned its children) or the depth
                // cap.  runSingleSimulation still looks it up in the TT (parallel_mcts.cpp:319-335) and
                // takes the cached value on a hit (no re-expansion), node->getValue() otherwise (:340-344)
                const size_t tb = (size_t)g * t.tt_slots;
                const int hs = (int)(hash & t.tt_mask);
                const int vis = t.tt_visits[tb + hs];
                const uint64_t th = t.tt_hash[tb + hs];
                const float tv = t.tt_value[tb + hs];
                if (WAVE) {
                    status = ST_EXPANDED;              // never evaluated; the completion makes the lookup
                } else if (vis > 0 && th == hash) {
                    status = ST_EXPVAL;
                    value = tv;
                    if (lane == 0) t.tt_visits[tb + hs] = vis + 1;
                    d_look += 1; d_hits += 1;
                } else {
                    status = ST_EXPANDED;
                    d_look += 1;
                }
            }
        }
    } else if (!go && stones >= t.A) {
        // expandNode: no legal moves -> terminal (parallel_mcts.cpp:646-654); a Go state always
        // has the pass
        if (lane == 0) {
            nd.flag[leaf] = (uint8_t)(nflag | FL_TERMINAL | FL_EXPANDED | (R_DRAW << 2));   // no lookups: counters unchanged
            t.lstatus[q] = ST_NONE; t.need_eval[q] = 0;
        }
        return;
    }

    tstamp(t, g, 0, 4);
    if (status == ST_NONE) {
        // Transposition table (direct-mapped emulation, transposition_table.cpp:44-191)
        const size_t tb = (size_t)g * t.tt_slots;
        hslot = (int)(hash & t.tt_mask);
        const int vis = t.tt_visits[tb + hslot];     // the whole entry in one round trip
        const uint64_t th = t.tt_hash[tb + hslot];
        const float tv = t.tt_value[tb + hslot];
        const uint64_t tr = t.tt_ref[tb + hslot];
        const bool hit = vis > 0 && th == hash;
        if (WAVE) {
            // An unexpanded, ongoing leaf: the completion decides between a TT hit, a wave-mate's expansion
            // and an evaluation.  It can need the evaluator unless the entry is a hit no wave-mate's store
            // can replace (visits >= 5 never drop): every other leaf gets its record and a batch row
            status = ST_EVAL;
            wskip = hit && vis >= 5;
            if (!wskip) {
                if (go) {
                    go_groups(t, board, gl, lane, 64);
                    go_write_leafrec(t, q, lane, board, gl, player, gko);
                } else {
                    write_leafrec(t, q, lane, board, hist6, player);
                }
            }
        } else if (hit) {
            status = ST_TTHIT;
            value = tv;
            ref = tr;
            if (lane == 0) t.tt_visits[tb + hslot] = vis + (mode == MODE_ROOT_SEARCH ? 2 : 1);
            d_look += 1; d_hits += 1;
        } else {
            status = ST_EVAL;
            store = (vis == 0 || vis < 5) ? 1 : 0;     // empty slot, or shouldReplace (visits < 5)
            d_look += (mode == MODE_ROOT_SEARCH ? 1 : 2);
            tstamp(t, g, 0, 5);
            if (go) {
                go_groups(t, board, gl, lane, 64);
                go_write_leafrec(t, q, lane, board, gl, player, gko);
            } else {
                write_leafrec(t, q, lane, board, hist6, player);
            }
        }
    }
    if (lane == 0) {
        t.lstatus[q] = status;
        t.lvalue[q] = value;
        t.lhash[q] = hash;
        t.ttstore[q] = store;
        t.ttref[q] = ref;
        t.tthslot[q] = hslot;
        t.plen[q] = depth + 1;
        t.need_eval[q] = (status == ST_EVAL && !wskip && (t.eval_kind == 0 || t.eval_kind == 4)) ? 1 : 0;
        if (!WAVE && mode == MODE_SIM) t.rhdr[g] = rhdr0;        // the root-header record (the next expansion's hint)
    }
    for (int i = lane; i <= depth; i += 64) {
        t.path[(size_t)q * AZ_DMAX + i] = spath[i];
        t.pact[(size_t)q * AZ_DMAX + i] = i ? sact[i] : -1;
    }
    tstamp(t, g, 0, 6);
    if (!WAVE && lane == 0) { cnt[CNT_LOOKUPS] = c_look + d_look; cnt[CNT_HITS] = c_hits + d_hits; }
    if (lane == 0 && mode == MODE_SIM) {
        // algorithmic bytes: child scans (whole 25 B records: N, W, VL, P + the child's header),
        // root header (21 B), VL read-modify-write (12 B + 12 B) and piece key (8 B) per path
        // node, root board, TT probe (12 B, +20 on a hit), the leaf record (A board bytes + 32 B,
        // Go: + A liberty bytes) when the leaf goes to the network, path record (8 B per node)
        long long b = scanned * 25 + 21 + (long long)(depth + 1) * (24 + 8 + 8) + t.A + 12;
        if (status == ST_TTHIT) b += 20;
        if (status == ST_EVAL) b += (go ? 2LL : 1LL) * t.A + 32;
        if (OPT) b += 12LL * widened;                   // progressive widening's decrement writes
        cnt[CNT_BYTES_SEL] = c_bytes + b;
    }
    tstamp(t, g, 0, 7);
}

template <int IT, bool OPT, bool RULES>
__global__ __launch_bounds__(64) void k_select(const TreeDev* __restrict__ tp, int mode) {
    const TreeDev& t = *tp;                               // device-resident (tree_dev, search_host.hip): an 8-byte kernarg
    __shared__ SelLds SL;
    __shared__ GoLds gl;
    select_game<IT, OPT, RULES>(t, mode, nullptr, SL, gl);
}

extern "C" int az_diag_tree_stamps(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_stamps), sizeof(unsigned long long) * (n < 128 ? n : 128)) == hipSuccess ? 0 : -1;
}

namespace {
template <bool OPT, bool RULES>
void launch_select(const TreeDev* t, int NA, int G, int mode, hipStream_t st) {
    if (NA <= 128) hipLaunchKernelGGL((k_select<2, OPT, RULES>), dim3(G), dim3(64), 0, st, t, mode);
    else if (NA <= 256) hipLaunchKernelGGL((k_select<4, OPT, RULES>), dim3(G), dim3(64), 0, st, t, mode);
    else hipLaunchKernelGGL((k_select<(AZ_MAXNA + 63) / 64, OPT, RULES>), dim3(G), dim3(64), 0, st, t, mode);
}
}  // namespace
// opt / rules: tree_has_opts() / tree_has_rules() of the TreeDev behind t (the launchers take device pointers)
void az_launch_select(const TreeDev* t, int NA, int G, int mode, bool opt, bool rules, hipStream_t st) {
    if (rules) { if (opt) launch_select<true, true>(t, NA, G, mode, st); else launch_select<false, true>(t, NA, G, mode, st); }
    else if (opt) launch_select<true, false>(t, NA, G, mode, st);
    else launch_select<false, false>(t, NA, G, mode, st);
}

// Host evaluator: the moves from the root to every leaf of the evaluation batch (slot order).
__global__ void k_leaf_moves(TreeDev t, int* moves, int* len) {
    const int i = blockIdx.x;
    if (i >= *t.n_eval) return;
    const int g = t.eval_games[i];
    const int depth = t.plen[g] - 1;
    for (int j = threadIdx.x; j < depth; j += blockDim.x) moves[(size_t)i * AZ_DMAX + j] = t.pact[(size_t)g * AZ_DMAX + j + 1];
    if (threadIdx.x == 0) len[i] = depth;
}

// K2: deterministic compaction of the leaves that need the network (one block).
// n: the records scanned -- the games, or with leaf parallelism the G * K leaf slots (k_scan_leaves)
__device__ __forceinline__ void scan_leaves(const TreeDev& t, const int n) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (n + 1023) / 1024;
    const int b0 = tid * per;
    int s = 0;
    for (int i = 0; i < per; ++i) { int g = b0 + i; if (g < n) s += t.need_eval[g]; }
    part[tid] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int off = part[tid] - s;
    for (int i = 0; i < per; ++i) {
        int g = b0 + i;
        if (g < n) {
            if (t.need_eval[g]) { t.eval_slot[g] = off; t.eval_games[off] = g; ++off; }
            else t.eval_slot[g] = -1;
        }
    }
    if (tid == 1023) *t.n_eval = part[1023];
}
__global__ __launch_bounds__(1024) void k_scan(const TreeDev* __restrict__ tp) {
    const TreeDev& t = *tp;
    scan_leaves(t, t.G);
}
__global__ __launch_bounds__(1024) void k_scan_leaves(const TreeDev* __restrict__ tp, int n) {
    const TreeDev& t = *tp;
    scan_leaves(t, n);
}

// K2 of a handle whose slots are evaluated by different nets (az_search_set_slot_nets): the stable
// partition of the leaves that need a network by slot_net[g], one block.  Net k owns region k -- rows
// [k * G, (k + 1) * G) of eval_games (and of the logits / values its forward writes): a slot's row is
// k * G + its rank among net k's leaves in slot order, n_eval[k] counts them.  The four nets' scans run
// together (one int4 per thread); a net without a leaf gets n_eval[k] = 0.
__global__ __launch_bounds__(1024) void k_scan_nets(const TreeDev* __restrict__ tp, const uint8_t* __restrict__ slot_net,
                                                    int n_nets) {
    const TreeDev& t = *tp;
    __shared__ int4 part[1024];
    const int tid = threadIdx.x;
    const int G = t.G;
    const int per = (G + 1023) / 1024;
    const int b0 = tid * per;
    int s[AZ_SCAN_NETS] = {0, 0, 0, 0};
    for (int i = 0; i < per; ++i) {
        const int g = b0 + i;
        if (g < G && t.need_eval[g]) {
            const int k = min((int)slot_net[g], n_nets - 1);
#pragma unroll
            for (int j = 0; j < AZ_SCAN_NETS; ++j) s[j] += k == j;
        }
    }
    part[tid] = int4{s[0], s[1], s[2], s[3]};
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int4 v = tid >= o ? part[tid - o] : int4{0, 0, 0, 0};
        __syncthreads();
        int4 p = part[tid];
        p.x += v.x; p.y += v.y; p.z += v.z; p.w += v.w;
        part[tid] = p;
        __syncthreads();
    }
    const int4 incl = part[tid];
    int off[AZ_SCAN_NETS] = {incl.x - s[0], G + incl.y - s[1], 2 * G + incl.z - s[2], 3 * G + incl.w - s[3]};
    for (int i = 0; i < per; ++i) {
        const int g = b0 + i;
        if (g >= G) break;
        if (!t.need_eval[g]) { t.eval_slot[g] = -1; continue; }
        const int k = min((int)slot_net[g], n_nets - 1);
        int row = 0;
#pragma unroll
        for (int j = 0; j < AZ_SCAN_NETS; ++j)
            if (k == j) { row = off[j]; ++off[j]; }
        t.eval_slot[g] = row; t.eval_games[row] = g;
    }
    if (tid == 1023) {
        const int tot[AZ_SCAN_NETS] = {incl.x, incl.y, incl.z, incl.w};
        for (int k = 0; k < n_nets; ++k) t.n_eval[k] = tot[k];
    }
}

// K3: evaluator output -> TT store -> expansion -> backup.
// Latency layout: every per-game input (status, path, cached leaf value / hash / batch slot, root
// board, TT / ring / pool cursors, counters) is loaded before anything waits -- one round trip --
// then the leaf's network outputs and the path nodes' statistics -- the second and last one.
// The Gomoku leaf board is the root board plus the path moves (no Zobrist work: k_select stored
// the leaf hash); a Go leaf's position comes back from the state k_select stored (go_load_leaf).
// WAVE: completion wj of a wave (k_wave_expand; leaf slot q = g * wK + wj), applied after completions 0 .. wj-1 of
// the same game: what k_select's single descent could settle at selection time is settled here instead, on the
// tree and the table as the wave-mates left them -- the leaf's flag and the TT entry are read again (a mate may
// have expanded the leaf, stored its entry, or replaced the entry selection saw), the lookup / hit counters and
// the entry's visit count move here, and the backup reads the path nodes' statistics from the nodes (every path
// shares the root with its mates' backups), not from the path record.
template <bool OPT, bool RULES, bool WAVE = false>
__device__ __forceinline__ void expand_game(const TreeDev& t, int mode, ExpLds& EL, GoLds& gl, RootHint* hint = nullptr,
                                            int wj = 0, int wK = 1) {
    const int g = blockIdx.x;
    const int q = WAVE ? g * wK + wj : g;             // leaf slot: the index of the per-step scratch
    const int lane = threadIdx.x;
    if (hint && lane == 0) hint->valid = 0;
    constexpr int NPAD = EXP_NPAD;
    auto& board = EL.board;
    auto& spath = EL.spath;
    auto& sact = EL.sact;
    auto& pol = EL.pol;
    auto& legal = EL.legal;
    auto& lp = EL.lp;
    auto& s_scalar = EL.s_scalar;
    static_assert(AZ_DMAX <= 128, "two path entries per lane");
    constexpr int BK = (AZ_MAXA + 63) / 64, PK = (AZ_MAXNA + 63) / 64;
    const bool go = t.game == GAME_GO;
    if (g >= t.G) return;
    const int A = t.A, NA = t.NA;
    // ---- round trip 1
    const size_t pb = (size_t)q * AZ_DMAX;
    int status = t.lstatus[q];
    const int plen = t.plen[q];
    const float lvalue = t.lvalue[q];
    const uint64_t lhash = t.lhash[q];
    const int slot = t.eval_identity ? q : t.eval_slot[q];
    const int pth0 = t.path[pb + lane], pac0 = t.pact[pb + lane];
    const int pth1 = lane < AZ_DMAX - 64 ? t.path[pb + 64 + lane] : 0;
    const int pac1 = lane < AZ_DMAX - 64 ? t.pact[pb + 64 + lane] : -1;
    // the path nodes' statistics as k_select left them (pstat; entries past the path are stale and
    // unused) and, with an identity batch, the leaf's network outputs: no second round trip
    const bool sim = mode == MODE_SIM;
    int4 ps0 = int4{0, 0, 0, 0}, ps1 = int4{0, 0, 0, 0};
    if (sim && !WAVE) {
        ps0 = t.pstat[pb + lane];
        if (lane < AZ_DMAX - 64) ps1 = t.pstat[pb + 64 + lane];
    }
    const int4 rh = sim && !WAVE ? t.rhdr[g] : int4{0, 0, 0, 0};   // the root's header as k_select left it
    int rfirst = rh.x, rcnt = rh.y, rflag = rh.z;
    const bool lg_early = t.eval_identity && (t.eval_kind == 0 || t.eval_kind == 4);
    float lg[PK];
    float netv = 0.0f;
    if (lg_early) {
        const float* src = t.net_logits + (size_t)q * NA;
#pragma unroll
        for (int k = 0; k < PK; ++k) lg[k] = lane + 64 * k < NA ? src[lane + 64 * k] : 0.0f;
        netv = t.net_value[q];
    }
    uint8_t rb[BK];
#pragma unroll
    for (int k = 0; k < BK; ++k) rb[k] = lane + 64 * k < A ? t.rboard[(size_t)g * A + lane + 64 * k] : 0;
    const int p0 = t.rplayer[g], rstones = t.rstones[g], rfresh = t.rfresh[g];
    const int atop = t.atop[g];
    int ttstore = t.ttstore[q], tthslot = t.tthslot[q];
    const uint64_t ring_cur = t.ring_cur[g];
    uint64_t ttref = t.ttref[q];
    long long* cnt = t.cnt + (size_t)g * AZ_NCNT;
    const long long c_ev = cnt[CNT_EVALS], c_evt = cnt[CNT_EVALS_TOTAL], c_sims = cnt[CNT_SIMS], c_bytes = cnt[CNT_BYTES_EXP];
    tstamp(t, g, 1, 0);
    if (status == ST_NONE) return;
    // the identity batch's logits were loaded in round trip 1: land them in LDS now, so their wait is
    // that round trip's (the compiler would otherwise sink the loads to the softmax)
    if (lg_early && status == ST_EVAL) {
#pragma unroll
        for (int k = 0; k < PK; ++k) if (lane + 64 * k < NA) pol[lane + 64 * k] = lg[k];
    }
    tstamp(t, g, 1, 1);
    const size_t base = (size_t)g * t.ncap;
    GamePtrs nd = game_nodes(t.nd, base);
    const int depth = plen - 1;
    // ---- round trip 2 (batches that are not the identity): the leaf's network outputs
    // (WAVE: a leaf selection gave no batch row has slot -1 and loads nothing)
    const bool net_in = status == ST_EVAL && (t.eval_kind == 0 || t.eval_kind == 4) && (!WAVE || slot >= 0);
    if (net_in && !lg_early) {
        const float* src = t.net_logits + (size_t)slot * NA;
#pragma unroll
        for (int k = 0; k < PK; ++k) lg[k] = lane + 64 * k < NA ? src[lane + 64 * k] : 0.0f;
        netv = t.net_value[slot];
    }
    int bN0 = ps0.x, bVL0 = ps0.y, bN1 = ps1.x, bVL1 = ps1.y;
    float bW0 = __int_as_float(ps0.z), bW1 = __int_as_float(ps1.z);
    if (WAVE && sim) {
        // the path nodes as the earlier descents and completions of this wave left them (entries past the
        // path are stale: not loaded)
        if (lane <= depth) { bN0 = nd.N[pth0]; bVL0 = nd.VL[pth0]; bW0 = nd.W[pth0]; }
        if (lane + 64 <= depth) { bN1 = nd.N[pth1]; bVL1 = nd.VL[pth1]; bW1 = nd.W[pth1]; }
    }

    spath[lane] = pth0; sact[lane] = pac0;
    if (lane < AZ_DMAX - 64) { spath[64 + lane] = pth1; sact[64 + lane] = pac1; }
    int hist6[6]; int player; uint64_t hash = lhash;
    int gko = -1, gpass = 0;
    uint64_t gbh = 0;
    if (go) {
        __syncthreads();
        go_load_leaf(t, g, q, lane, sact, depth, board, gl, hist6, player, gko, gpass, gbh, hash);
    } else {
#pragma unroll
        for (int k = 0; k < BK; ++k) if (lane + 64 * k < A) board[lane + 64 * k] = rb[k];
        __syncthreads();
        if (lane >= 1 && lane <= depth) board[pac0] = (uint8_t)((lane & 1) ? p0 : 3 - p0);
        if (lane + 64 <= depth) board[pac1] = (uint8_t)(((lane + 64) & 1) ? p0 : 3 - p0);
        player = (depth & 1) ? 3 - p0 : p0;
        if (t.eval_kind == 1)
            for (int i = 0; i < 6; ++i) hist6[i] = i < depth ? sact[depth - i] : t.rhist[g * 6 + (i - depth)];
        __syncthreads();
    }
    tstamp(t, g, 1, 2);
    const int leaf = spath[depth];
    float value = lvalue;
    long long ev_add = 0;
    int wflag = 0;                                   // WAVE: the leaf's flag as completion wj finds it
    long long w_look = 0, w_hits = 0;
    if (WAVE && status != ST_TERMINAL) {
        // runSingleSimulation from its TT lookup on (parallel_mcts.cpp:319-346), now: a hit expands the leaf
        // unless a wave-mate did ("another thread expanded it"); a miss on an expanded leaf takes getValue();
        // otherwise evaluateState (its own lookup), store, expand
        wflag = nd.flag[leaf];
        const size_t tb = (size_t)g * t.tt_slots;
        tthslot = (int)(lhash & t.tt_mask);
        const int vis = t.tt_visits[tb + tthslot];
        const uint64_t th = t.tt_hash[tb + tthslot];
        const float tv = t.tt_value[tb + tthslot];
        const uint64_t tr = t.tt_ref[tb + tthslot];
        if (vis > 0 && th == lhash) {
            status = (wflag & FL_EXPANDED) ? ST_EXPVAL : ST_TTHIT;
            value = tv;
            ttref = tr;
            if (lane == 0) t.tt_visits[tb + tthslot] = vis + 1;
            w_look = 1; w_hits = 1;
        } else if (wflag & FL_EXPANDED) {
            status = ST_EXPANDED;
            w_look = 1;
        } else {
            status = ST_EVAL;
            ttstore = vis < 5 ? 1 : 0;               // empty slot, or shouldReplace (visits < 5)
            w_look = 2;
            if ((t.eval_kind == 0 || t.eval_kind == 4) && slot < 0) {   // no batch row: selection's rule is wrong
                if (lane == 0) atomicOr(t.err, ERR_BATCH);
                return;
            }
        }
    }
    // algorithmic bytes: path (4 + 4 B per level), root board, then below: policy / TT / ring,
    // new child records (25 B), VL-removal + backup read-modify-write (24 B per path node)
    long long kb = (long long)plen * 8 + A;

    if (status == ST_EVAL || status == ST_TTHIT) {
        // legal moves in child order (gomoku_state.cpp:531-578)
        int n = 0;
        const bool fresh = !go && (depth == 0) && rfresh;
        if (go) {
            GoKeys gk;
            go_keys(t, board, player, lane, gk);
            go_groups(t, board, gl, lane, 64, &gk);
            n = go_legal(t, g, lane, board, gl, player, gko, gbh, legal, gk);
        } else if (fresh) {
            for (int i = lane; i < A; i += 64) legal[i] = t.fresh_order[i];
            n = A - rstones;   // fresh root is the empty board
        } else {
            // RULES: a Black-to-move leaf's legal cells leave out the mask k_select built for it
            const uint64_t* forb = RULES && player == 1 ? t.gforb + (size_t)q * AZ_FORB_WORDS : nullptr;
            for (int c0 = 0; c0 < A; c0 += 64) {
                const int a = A - 1 - (c0 + lane);
                bool e = a >= 0 && board[a] == 0;
                if (RULES && forb && e) e = !((forb[a >> 6] >> (a & 63)) & 1ULL);
                const unsigned long long m = __ballot(e);
                const int pos = n + __popcll(m & ((1ULL << lane) - 1ULL));
                if (e) legal[pos] = a;
                n += __popcll(m);
            }
        }
        __syncthreads();
        tstamp(t, g, 1, 3);
        if (status == ST_EVAL || go) {
          if (status == ST_TTHIT) {
            // Go transposition hit: a position's legal set also depends on its history (superko),
            // so the ring keeps the cached policy itself (NA floats) and expandNodeWithPolicy's
            // gather is redone over the current legal set, as the reference does with entry.policy
            if (ring_cur - ttref > (uint64_t)t.ring) { if (lane == 0) atomicOr(t.err, ERR_RING); return; }
            const float* rbuf = t.ring_buf + (size_t)g * t.ring;
            const uint32_t r0 = (uint32_t)(ttref % (uint64_t)t.ring);
            for (int a = lane; a < NA; a += 64) pol[a] = rbuf[ring_wrap(r0 + a, t.ring)];
            __syncthreads();
          } else {
            ev_add = 1;
            if (t.eval_kind == 0) {
                float mx = -FLT_MAX;
#pragma unroll
                for (int k = 0; k < PK; ++k) if (lane + 64 * k < NA) mx = fmaxf(mx, lg[k]);
                tstamp(t, g, 1, 8);
                mx = wave_max(mx);
                tstamp(t, g, 1, 9);
                float e[PK];
#pragma unroll
                for (int k = 0; k < PK; ++k) {
                    e[k] = lane + 64 * k < NA ? expf(lg[k] - mx) : 0.0f;
                    pol[lane + 64 * k] = e[k];                 // +0.0f past NA
                }
                __syncthreads();
                tstamp(t, g, 1, 10);
                if (lane == 0) s_scalar[0] = seq_sum_lds(pol, NA);
                __syncthreads();
                tstamp(t, g, 1, 11);
                const float sum = s_scalar[0];
#pragma unroll
                for (int k = 0; k < PK; ++k)
                    if (lane + 64 * k < NA && sum > 0.0f) pol[lane + 64 * k] = e[k] / sum;
                value = netv;
                tstamp(t, g, 1, 4);
            } else if (t.eval_kind == 4) {
                // host evaluator (az_search_set_evaluator): the policy as NeuralNetwork::predict
                // returns it, used as is by expandNodeWithPolicy (parallel_mcts.cpp:886-901)
#pragma unroll
                for (int k = 0; k < PK; ++k) if (lane + 64 * k < NA) pol[lane + 64 * k] = lg[k];
                value = netv;
            } else if (t.eval_kind == 3) {
                // no network: 1/|legal| on the legal actions, value 0 (parallel_mcts.cpp:903-916)
                const float u = n > 0 ? 1.0f / (float)n : 0.0f;
                for (int a = lane; a < NA; a += 64) pol[a] = 0.0f;
                __syncthreads();
                for (int i = lane; i < n; i += 64) if (legal[i] >= 0) pol[legal[i]] = u;
                value = 0.0f;
            } else if (t.eval_kind == 1) {
                const uint64_t key = hash_eval_key(hash, hist6);
                for (int a = lane; a < NA; a += 64) pol[a] = hash_eval_p(key, a);
                value = hash_eval_v(key);
            } else {
                // RandomPolicyNetwork (random_policy_network.cpp:93-130): draws for legal a >= 0
                uint32_t* st = t.mt + (size_t)g * 625;
                for (int a = lane; a < NA; a += 64) pol[a] = 0.001f;
                __syncthreads();
                if (lane == 0) {
                    float sum = 0.0f;
                    for (int i = 0; i < n; ++i) {
                        if (legal[i] < 0) continue;
                        float u = mt_uniform(st, 0.0f, 1.0f); pol[legal[i]] = u; sum += u;
                    }
                    s_scalar[0] = sum;
                    s_scalar[1] = mt_uniform(st, -0.1f, 0.1f);
                }
                __syncthreads();
                const float sum = s_scalar[0];
                if (sum > 0.0f) for (int a = lane; a < NA; a += 64) pol[a] = pol[a] / sum;
                value = s_scalar[1];
            }
            __syncthreads();
            if (g == t.log_game && t.log_pol) {
                const int k = *t.log_n;
                if (k < t.log_cap) {
                    for (int a = lane; a < NA; a += 64) t.log_pol[(size_t)k * NA + a] = pol[a];
                    if (t.log_planes) {
                        const int npl = go ? 8 : 11;
                        const uint8_t* rec = t.leafrec + (size_t)q * AZ_REC_BYTES;
                        for (int a = lane; a < A; a += 64) {
                            float c[16];
                            az_leaf_planes(rec, go, t.bs, a, c);
#pragma unroll
                            for (int ch = 0; ch < 11; ++ch)
                                if (ch < npl) t.log_planes[((size_t)k * npl + ch) * A + a] = c[ch];
                        }
                    }
                    if (lane == 0) { t.log_val[k] = value; *t.log_n = k + 1; }
                }
            }
          }
            // expandNodeWithPolicy: gather, sequential sum, renormalise (parallel_mcts.cpp:702-724)
            float gv[PK];
#pragma unroll
            for (int k = 0; k < PK; ++k) {
                const int i = lane + 64 * k;
                gv[k] = i < n && legal[i] >= 0 ? pol[legal[i]] : 0.0f;   // pass: no prior
            }
#pragma unroll
            for (int k = 0; k < PK; ++k) lp[lane + 64 * k] = gv[k];   // +0.0f past n
            __syncthreads();
            tstamp(t, g, 1, 12);
            if (lane == 0) s_scalar[0] = seq_sum_lds(lp, n);
            __syncthreads();
            tstamp(t, g, 1, 13);
            const float ps = s_scalar[0];
            const float u = 1.0f / (float)n;
#pragma unroll
            for (int k = 0; k < PK; ++k)
                if (lane + 64 * k < n) lp[lane + 64 * k] = ps > 0.0f ? gv[k] / ps : u;
            tstamp(t, g, 1, 5);
        } else {
            // transposition hit: the stored priors are exactly the renormalised gather of
            // the cached policy over the same legal set (same position => same order).
            if (ring_cur - ttref > (uint64_t)t.ring) { if (lane == 0) atomicOr(t.err, ERR_RING); return; }
            const float* rbuf = t.ring_buf + (size_t)g * t.ring;
            const uint32_t r0 = (uint32_t)(ttref % (uint64_t)t.ring);
            for (int i = lane; i < n; i += 64) lp[i] = rbuf[ring_wrap(r0 + i, t.ring)];
        }
        __syncthreads();
        // TT store (new entry) + prior ring
        if (status == ST_EVAL && ttstore) {
            float* rbuf = t.ring_buf + (size_t)g * t.ring;
            const int len = go ? NA : n;            // Go keeps the policy, Gomoku the children priors
            const float* src = go ? pol : lp;
            const uint32_t r0 = (uint32_t)(ring_cur % (uint64_t)t.ring);
            for (int i = lane; i < len; i += 64) rbuf[ring_wrap(r0 + i, t.ring)] = src[i];
            if (lane == 0) {
                const size_t tb = (size_t)g * t.tt_slots + tthslot;
                t.tt_hash[tb] = hash; t.tt_visits[tb] = 1; t.tt_value[tb] = value; t.tt_ref[tb] = ring_cur;
                t.ring_cur[g] = ring_cur + (uint64_t)len;
            }
        }
        // create children (include/alphazero/mcts/mcts_node.h: N=W=VL=0, prior, action)
        if (atop + n > t.ncap) { if (lane == 0) atomicOr(t.err, ERR_NODES); return; }
        const int first = atop;
#pragma unroll
        for (int k = 0; k < PK; ++k) {                 // unrolled: the LDS reads of every chunk before the stores
            const int i = lane + 64 * k;
            if (i < n) {
                const int c = first + i;
                nd.N[c] = 0; nd.W[c] = 0.0f; nd.VL[c] = 0; nd.P[c] = lp[i];
                nd.first[c] = -1; nd.act[c] = (int16_t)legal[i]; nd.cnt[c] = 0; nd.flag[c] = 0;
            }
        }
        // the leaf's flag: k_select left it in the path record (a simulation step), else from the node
        const int lfw = WAVE ? wflag : lane_bcast(depth < 64 ? ps0.w : ps1.w, depth & 63);
        if (lane == 0) {
            t.atop[g] = first + n;
            const uint8_t fl = (uint8_t)((sim ? (uint8_t)lfw : nd.flag[leaf]) | FL_EXPANDED);
            nd.first[leaf] = first; nd.cnt[leaf] = (int16_t)n; nd.flag[leaf] = fl;
            cnt[CNT_NODES] = first + n;
            if (depth == 0) { rfirst = first; rcnt = n; rflag = fl; }   // the root was the leaf
        }
        kb += 25LL * n + 7 + 4LL * n + (status == ST_EVAL ? 4LL * NA + 4 + 24 : 0);
        tstamp(t, g, 1, 6);
    } else if (status == ST_EXPANDED) {
        value = nd.N[leaf] == 0 ? 0.0f : nd.W[leaf] / (float)nd.N[leaf];
    }   // ST_EXPVAL: the TT value k_select cached in lvalue

    if (sim) {
        // backpropagate(node, value, searchPath) (parallel_mcts.cpp:782-833): the reference walks the
        // path leaf -> root negating v at every step, so node i gets (-1)^(depth-i) * value.  Path
        // nodes are distinct and each gets its own unchanged sequence of fp32 operations, so the
        // update runs one lane per node (bit-identical to the sequential walk) on the statistics
        // loaded in round trip 2 (nothing in this kernel writes a path node's N / VL / W before).
        float v0 = ((depth - lane) & 1) ? -value : value;
        float v1 = ((depth - lane - 64) & 1) ? -value : value;
        if (OPT && t.use_td) {
            // TD(lambda) (:825-831): after node i's update the value is negated and, unless node i is
            // the root, becomes (1 - lambda) * (-parent.getValue()) + lambda * value -- two products and
            // a sum -- with the parent (node i - 1) not yet updated and its virtual loss still on: the
            // pstat statistics.  The parents' terms are lane-parallel; the recurrence over the path is
            // sequential (wave-uniform, the terms read lane by lane).
            const float om = 1.0f - t.td_lambda;
            const float a0 = om * -(bN0 == 0 ? 0.0f : bW0 / (float)bN0);
            const float a1 = om * -(bN1 == 0 ? 0.0f : bW1 / (float)bN1);
            float cv = value;
            if (lane == (depth & 63)) { if (depth < 64) v0 = cv; else v1 = cv; }
            for (int i = depth; i >= 1; --i) {
                const int j = i - 1;
                const float a = lane_bcast(j < 64 ? a0 : a1, j & 63);
                cv = a + t.td_lambda * -cv;
                if (lane == (j & 63)) { if (j < 64) v0 = cv; else v1 = cv; }
            }
        }
        if (lane <= depth) {
            const float v = v0;
            int N = bN0 - t.vl, VL = bVL0 - t.vl;
            float W = bW0 + (float)t.vl;                   // removeVirtualLoss
            N += 1;
            W = W + v;
            nd.N[pth0] = N; nd.VL[pth0] = VL; nd.W[pth0] = W;
            if (hint && lane == 0) {                    // path[0]: the root
                hint->valid = 1; hint->N = N; hint->VL = VL; hint->W = W;
                hint->first = rfirst; hint->cnt = rcnt; hint->flag = rflag;
            }
        }
        if (lane + 64 <= depth) {
            const float v = v1;
            int N = bN1 - t.vl, VL = bVL1 - t.vl;
            float W = bW1 + (float)t.vl;
            N += 1;
            W = W + v;
            nd.N[pth1] = N; nd.VL[pth1] = VL; nd.W[pth1] = W;
        }
        kb += 24LL * plen;
    }
    if (lane == 0) {
        if (ev_add) { cnt[CNT_EVALS] = c_ev + 1; cnt[CNT_EVALS_TOTAL] = c_evt + 1; }
        if (sim) { cnt[CNT_SIMS] = c_sims + 1; cnt[CNT_BYTES_EXP] = c_bytes + kb; }
        if (WAVE) { cnt[CNT_LOOKUPS] += w_look; cnt[CNT_HITS] += w_hits; }
    }
    tstamp(t, g, 1, 7);
}

template <bool OPT, bool RULES>
__global__ __launch_bounds__(64) void k_expand_backup(const TreeDev* __restrict__ tp, int mode) {
    const TreeDev& t = *tp;
    __shared__ ExpLds EL;
    __shared__ GoLds gl;
    expand_game<OPT, RULES>(t, mode, EL, gl);
}
void az_launch_expand_backup(const TreeDev* t, int G, int mode, bool opt, bool rules, hipStream_t st) {
    if (rules) {
        if (opt) hipLaunchKernelGGL((k_expand_backup<true, true>), dim3(G), dim3(64), 0, st, t, mode);
        else hipLaunchKernelGGL((k_expand_backup<false, true>), dim3(G), dim3(64), 0, st, t, mode);
    } else if (opt) hipLaunchKernelGGL((k_expand_backup<true, false>), dim3(G), dim3(64), 0, st, t, mode);
    else hipLaunchKernelGGL((k_expand_backup<false, false>), dim3(G), dim3(64), 0, st, t, mode);
}

// K3 of simulation step i and K1 of step i+1 in one launch: a game's expansion / backup and its
// next selection are the same wave's consecutive work (no other game is involved), so one
// kernel boundary per step goes (the wave's own global stores are visible to its later loads
// after the block barrier's release / acquire).  te: step i's batch maps, ts: the search's.
// One TreeDev argument (the kernel's scalar registers are the tight resource): the expansion's
// batch map differs from the search's only in eval_slot / eval_identity.
template <int IT, bool OPT, bool RULES>
__global__ __launch_bounds__(64) void k_expand_select(const TreeDev* __restrict__ tsp, const int* eval_slot, int eval_identity) {
    const TreeDev& ts = *tsp;
    __shared__ RootHint hint;
    __shared__ union PhaseLds { SelLds s; ExpLds e; } U;
    __shared__ GoLds gl;
    TreeDev te = ts;
    te.eval_slot = const_cast<int*>(eval_slot);
    te.eval_identity = eval_identity;
    expand_game<OPT, RULES>(te, MODE_SIM, U.e, gl, &hint);
    __syncthreads();                                      // the expansion's LDS is the selection's from here
    select_game<IT, OPT, RULES>(ts, MODE_SIM, &hint, U.s, gl);
}

namespace {
template <bool OPT, bool RULES>
void launch_expand_select(const TreeDev* ts, const int* eval_slot, int eval_identity, int NA, int G, hipStream_t st) {
    if (NA <= 128) hipLaunchKernelGGL((k_expand_select<2, OPT, RULES>), dim3(G), dim3(64), 0, st, ts, eval_slot, eval_identity);
    else if (NA <= 256) hipLaunchKernelGGL((k_expand_select<4, OPT, RULES>), dim3(G), dim3(64), 0, st, ts, eval_slot, eval_identity);
    else hipLaunchKernelGGL((k_expand_select<(AZ_MAXNA + 63) / 64, OPT, RULES>), dim3(G), dim3(64), 0, st, ts, eval_slot, eval_identity);
}
}  // namespace
void az_launch_expand_select(const TreeDev* ts, const int* eval_slot, int eval_identity, int NA, int G, bool opt, bool rules,
                             hipStream_t st) {
    if (rules) {
        if (opt) launch_expand_select<true, true>(ts, eval_slot, eval_identity, NA, G, st);
        else launch_expand_select<false, true>(ts, eval_slot, eval_identity, NA, G, st);
    } else if (opt) launch_expand_select<true, false>(ts, eval_slot, eval_identity, NA, G, st);
    else launch_expand_select<false, false>(ts, eval_slot, eval_identity, NA, G, st);
}

// Leaf parallelism (handle setting leaves = K > 1, az_search_set_leaves): a simulation step is a wave of k <= K
// descents per game, all made before any of their leaves is completed -- ParallelMCTS with numThreads = k in the
// interleaving where every worker has put its virtual loss on its path (parallel_mcts.cpp:295) before any of them
// looks at its leaf (:297), the workers then finishing in order.  The game's one wavefront loops the shared
// selection / expansion over the k leaf slots q = g * K + j; between two iterations a block barrier (with its
// work-group release / acquire) makes the wave's own stores to the tree, the table and the cursors visible to its
// next loads, as between the two halves of k_expand_select.  K = 1 handles never launch these kernels.
template <int IT>
__global__ __launch_bounds__(64) void k_wave_select(const TreeDev* __restrict__ tp, int K, int k) {
    const TreeDev& t = *tp;
    __shared__ SelLds SL;
    __shared__ GoLds gl;
    for (int j = 0; j < k; ++j) {
        select_game<IT, false, false, true>(t, MODE_SIM, nullptr, SL, gl, j, K);
        __syncthreads();
    }
    // a short wave (the last of a search whose simulations K does not divide): the other slots hold no leaf
    const int g = blockIdx.x, j = k + (int)threadIdx.x;
    if (g < t.G && j < K) { t.lstatus[g * K + j] = ST_NONE; t.need_eval[g * K + j] = 0; }
}
__global__ __launch_bounds__(64) void k_wave_expand(const TreeDev* __restrict__ tp, int K, int k) {
    const TreeDev& t = *tp;
    __shared__ ExpLds EL;
    __shared__ GoLds gl;
    for (int j = 0; j < k; ++j) {
        expand_game<false, false, true>(t, MODE_SIM, EL, gl, nullptr, j, K);
        __syncthreads();
    }
}
void az_launch_wave_select(const TreeDev* t, int NA, int G, int K, int k, hipStream_t st) {
    if (NA <= 128) hipLaunchKernelGGL((k_wave_select<2>), dim3(G), dim3(64), 0, st, t, K, k);
    else if (NA <= 256) hipLaunchKernelGGL((k_wave_select<4>), dim3(G), dim3(64), 0, st, t, K, k);
    else hipLaunchKernelGGL((k_wave_select<(AZ_MAXNA + 63) / 64>), dim3(G), dim3(64), 0, st, t, K, k);
}
void az_launch_wave_expand(const TreeDev* t, int G, int K, int k, hipStream_t st) {
    hipLaunchKernelGGL(k_wave_expand, dim3(G), dim3(64), 0, st, t, K, k);
}

// K4: visit distribution, action choice and root value per game.
__global__ __launch_bounds__(64) void k_select_action(const TreeDev* __restrict__ tp, int training, float temperature,
                                                      const float* temps, int* actions, float* values, float* probs,
                                                      int* child_actions, int* nchild) {
    const TreeDev& t = *tp;
    const int g = blockIdx.x;
    if (temps && g < t.G) temperature = temps[g];         // per-game schedule (self-play driver)
    const int lane = threadIdx.x;
    __shared__ float c[AZ_MAXNA];
    if (g >= t.G) return;
    const int A = t.A, NA = t.NA;
    const bool go = t.game == GAME_GO;
    if (!t.active[g]) {
        if (lane == 0) { actions[g] = go ? -2 : -1; values[g] = 0.0f; nchild[g] = 0; }
        return;
    }
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    const int root = t.rnode[g];
    const int fc = nd.first[root], nc = nd.cnt[root];
    const uint8_t f = nd.flag[root];
    if ((f & FL_TERMINAL) || nc == 0) {
        if (lane == 0) {
            // first legal move of the root state (parallel_mcts.cpp:994-1004)
            int a = -1;                                         // Go: the pass leads getLegalMoves
            const uint8_t* rb = t.rboard + (size_t)g * A;
            if (go) a = -1;
            else if (t.rfresh[g]) a = t.fresh_order[0];
            else for (int x = A - 1; x >= 0; --x) if (rb[x] == 0) { a = x; break; }
            actions[g] = a; values[g] = 0.0f; nchild[g] = 0;
        }
        return;
    }
    const float ex = 1.0f / fmaxf(0.01f, temperature);
    for (int i = lane; i < nc; i += 64) {
        const float Nf = (float)nd.N[fc + i];
        float v;
        if (ex == 1.0f) v = Nf;                                // pow(x, 1) == x exactly
        else v = (float)pow((double)Nf, (double)ex);
        c[i] = v;
        child_actions[(size_t)g * NA + i] = nd.act[fc + i];
    }
    __syncthreads();
    if (lane == 0) {
        float total = 0.0f;
        for (int i = 0; i < nc; ++i) total += c[i];
        float* pr = probs + (size_t)g * NA;
        if (total > 0.0f) for (int i = 0; i < nc; ++i) pr[i] = c[i] / total;
        else { const float u = 1.0f / (float)nc; for (int i = 0; i < nc; ++i) pr[i] = u; }
        int bi = 0;
        if (training && temperature > 0.0f) {
            for (int i = 1; i < nc; ++i) if (pr[bi] < pr[i]) bi = i;      // std::max_element
        } else {
            int mx = 0;
            for (int i = 0; i < nc; ++i) mx = max(mx, nd.N[fc + i]);
            for (int i = 0; i < nc; ++i) if (nd.N[fc + i] == mx) { bi = i; break; }
        }
        actions[g] = nd.act[fc + bi];
        const int rN = nd.N[root];
        values[g] = rN == 0 ? 0.0f : nd.W[root] / (float)rN;
        nchild[g] = nc;
    }
}

// K6: copy the subtree of the (new) root into the other arena, breadth first.
// Subtree reuse: BFS copy of the new root's subtree into the other arena (children of a node stay
// contiguous and in order; node k of the copy came from src_of[k]).  One 256-thread block per game
// takes 256 queued nodes per round: a block prefix sum of their child counts places every child,
// and all the round's children are copied in parallel, each thread finding its parent by binary
// search over the prefix (one dependent round of loads per round instead of one per parent).
__global__ __launch_bounds__(256) void k_compact(TreeDev t, Nodes dst, int* src_of) {
    constexpr int NT = 256;
    __shared__ int s_inc[NT];     // inclusive prefix of this round's child counts
    __shared__ int s_fs[NT];      // first child (source arena) of each queued node
    __shared__ int s_wsum[NT / 64];
    const int g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (g >= t.G) return;
    const size_t base = (size_t)g * t.ncap;
    GamePtrs s = game_nodes(t.nd, base);
    GamePtrs d = game_nodes(dst, base);
    int* so = src_of + base;
    const int root = t.rnode[g];
    if (tid == 0) {
        d.N[0] = s.N[root]; d.W[0] = s.W[root]; d.VL[0] = s.VL[root]; d.P[0] = s.P[root];
        d.act[0] = s.act[root]; d.cnt[0] = s.cnt[root]; d.flag[0] = s.flag[root]; d.first[0] = -1;
        so[0] = root;
    }
    __syncthreads();
    int j = 0, top = 1;
    while (j < top) {
        const int m = min(NT, top - j);
        const int k = j + tid;
        const bool valid = tid < m;
        const int sn = valid ? so[k] : 0;
        const int nc = valid ? (int)s.cnt[sn] : 0;
        const int fs = valid && nc ? s.first[sn] : 0;
        // block inclusive scan of nc
        const int wincl = wave_incl_scan(nc, lane);
        if (lane == 63) s_wsum[wave] = wincl;
        __syncthreads();
        int off = 0;
#pragma unroll
        for (int w = 0; w < NT / 64; ++w) off += w < wave ? s_wsum[w] : 0;
        const int incl = off + wincl;
        s_inc[tid] = incl;
        s_fs[tid] = fs;
        const int tot = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
        if (valid) d.first[k] = nc ? top + incl - nc : -1;
        __syncthreads();
        if (top + tot > t.ncap) { if (tid == 0) atomicOr(t.err, ERR_NODES); return; }
        for (int c = tid; c < tot; c += NT) {
            int lo = 0, hi = m - 1;                // smallest p with s_inc[p] > c
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_inc[mid] > c) hi = mid; else lo = mid + 1;
            }
            const int ex = lo ? s_inc[lo - 1] : 0;
            const int a = s_fs[lo] + (c - ex), b = top + c;
            d.N[b] = s.N[a]; d.W[b] = s.W[a]; d.VL[b] = s.VL[a]; d.P[b] = s.P[a];
            d.act[b] = s.act[a]; d.cnt[b] = s.cnt[a]; d.flag[b] = s.flag[a]; d.first[b] = -1;
            so[b] = a;
        }
        __syncthreads();                           // so[] of this round visible to the next (same CU)
        j += m;
        top += tot;
    }
    if (tid == 0) { t.rnode[g] = 0; t.atop[g] = top; }
}

// releaseMemory(visitThreshold) (parallel_mcts.cpp:1481-1496; MCTSNode::pruneTree mcts_node.cpp:451-477):
// BFS copy of the tree into the other arena keeping, below every node, only the children with
// visitCount >= threshold (in child order; the root itself stays).  A node whose children all go
// stays expanded with none.  pruned[g] = nodes before - nodes after (getTreeSize of every removed
// subtree: the arena holds exactly the tree).
__global__ __launch_bounds__(64) void k_prune(TreeDev t, Nodes dst, int* src_of, int thr_all, const int* thr_g,
                                              long long* pruned) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    if (g >= t.G) return;
    const int thr = thr_g ? thr_g[g] : thr_all;     // per game (0: keep every child, the whole tree)
    const size_t base = (size_t)g * t.ncap;
    GamePtrs s = game_nodes(t.nd, base);
    GamePtrs d = game_nodes(dst, base);
    int* so = src_of + base;
    const int root = t.rnode[g];
    const int before = t.atop[g];
    if (lane == 0) {
        d.N[0] = s.N[root]; d.W[0] = s.W[root]; d.VL[0] = s.VL[root]; d.P[0] = s.P[root];
        d.act[0] = s.act[root]; d.cnt[0] = s.cnt[root]; d.flag[0] = s.flag[root]; d.first[0] = -1;
        so[0] = root;
    }
    __syncthreads();
    int j = 0, top = 1;
    while (j < top) {
        const int k = j + lane;
        const bool valid = k < top;
        const int sn = valid ? so[k] : 0;
        const int fsrc = valid ? s.first[sn] : 0;
        const int ncs = valid ? (int)s.cnt[sn] : 0;
        int nc = 0;                                  // children this node keeps
        for (int i = 0; i < ncs; ++i) nc += s.N[fsrc + i] >= thr ? 1 : 0;
        const int incl = wave_incl_scan(nc, lane);
        const int tot = __shfl(incl, 63);
        const int nf = top + incl - nc;
        if (valid) { d.first[k] = nc ? nf : -1; d.cnt[k] = (int16_t)nc; }
        const int m = min(64, top - j);
        for (int e = 0; e < m; ++e) {
            const int ce = __shfl(ncs, e);
            if (__shfl(nc, e) == 0) continue;
            const int fs = __shfl(fsrc, e);
            int fd = __shfl(nf, e);
            if (fd + __shfl(nc, e) > t.ncap) { if (lane == 0) atomicOr(t.err, ERR_NODES); return; }
            for (int i0 = 0; i0 < ce; i0 += 64) {
                const int i = i0 + lane;
                const int a = fs + i;
                const bool keep = i < ce && s.N[a] >= thr;
                const unsigned long long bm = __ballot(keep);
                if (keep) {
                    const int b = fd + __popcll(bm & ((1ULL << lane) - 1ULL));
                    d.N[b] = s.N[a]; d.W[b] = s.W[a]; d.VL[b] = s.VL[a]; d.P[b] = s.P[a];
                    d.act[b] = s.act[a]; d.cnt[b] = s.cnt[a]; d.flag[b] = s.flag[a]; d.first[b] = -1;
                    so[b] = a;
                }
                fd += __popcll(bm);
            }
        }
        __syncthreads();
        j += m;
        top += tot;
    }
    if (lane == 0) {
        t.rnode[g] = 0; t.atop[g] = top;
        t.cnt[(size_t)g * AZ_NCNT + CNT_NODES] = top;
        pruned[g] = before - top;
    }
}

// K7: Dirichlet mix on the root children (noise already normalised on the host).
__global__ __launch_bounds__(64) void k_noise(TreeDev t, const float* noise, const uint8_t* mask, float eps) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    if (g >= t.G || !mask[g]) return;
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    const int root = t.rnode[g];
    const int fc = nd.first[root], nc = nd.cnt[root];
    const float* nz = noise + (size_t)g * t.NA;
    for (int i = lane; i < nc; i += 64) {
        const float old = nd.P[fc + i];
        nd.P[fc + i] = (1.0f - eps) * old + eps * nz[i];
    }
}

// ---------------------------------------------------------------------------
// Slot lifecycle: a slot's root position, the rules' verdict on a move, the move itself and the start of a
// game, each written once.  k_new_games is "empty position, slot start", k_apply is "load, move, store, reuse
// the child", k_open_games is "empty position, (judge, move) per ply, slot start" and k_illegal_moves is
// "load, judge": whichever entry point reaches a position, the same code made it.
namespace {
// The root position of one slot -- what the r* arrays (tree.h) hold for it -- in wave-uniform registers.
struct RootPos {
    int player, stones, ply, res;    // side to move; stones placed; plies played (Go: passes too); GameResult
    int h6[6];                       // last moves, [0] most recent, -1 none
    uint64_t hash;                   // Gomoku: the position's Zobrist hash; Go: the stones-only hash
    int ko, passes, cap[2], nh;      // Go: ko point, consecutive passes, captures by black / white, rposh entries
};

// The start position.  Go: the stones-only hash of the empty board; Gomoku: Black to move, under Renju / Omok
// with the rules' feature keys.
__device__ __forceinline__ RootPos root_empty(const TreeDev& t) {
    RootPos s;
    s.player = 1; s.stones = 0; s.ply = 0; s.res = R_ONGOING;
    for (int i = 0; i < 6; ++i) s.h6[i] = -1;
    s.hash = t.game == GAME_GO ? 0ULL : (t.renju || t.omok) ? t.zplayer[0] ^ t.zconst : t.zplayer[0];
    s.ko = -1; s.passes = 0; s.cap[0] = 0; s.cap[1] = 0; s.nh = 0;
    return s;
}

__device__ __forceinline__ RootPos root_load(const TreeDev& t, int g) {
    RootPos s;
    s.player = t.rplayer[g]; s.stones = t.rstones[g]; s.ply = t.rply[g]; s.res = t.gresult[g];
    for (int i = 0; i < 6; ++i) s.h6[i] = t.rhist[g * 6 + i];
    s.hash = t.rhash[g];
    s.ko = -1; s.passes = 0; s.cap[0] = 0; s.cap[1] = 0; s.nh = 0;
    if (t.game == GAME_GO) {
        s.ko = t.rko[g]; s.passes = t.rpass[g]; s.cap[0] = t.rcap[2 * g]; s.cap[1] = t.rcap[2 * g + 1];
        s.nh = t.rnposh[g];
    }
    return s;
}

// The position and its board (LDS, complete) into slot g: a finished game stops searching, and only a game
// without a ply is fresh.  Every lane of the wave calls it.
__device__ __forceinline__ void root_store(const TreeDev& t, int g, int lane, const RootPos& s, const uint8_t* board) {
    uint8_t* rb = t.rboard + (size_t)g * t.A;
    for (int i = lane; i < t.A; i += 64) rb[i] = board[i];
    if (lane != 0) return;
    t.rplayer[g] = s.player; t.rstones[g] = s.stones; t.rply[g] = s.ply; t.rfresh[g] = s.ply == 0;
    for (int i = 0; i < 6; ++i) t.rhist[g * 6 + i] = s.h6[i];
    t.rhash[g] = s.hash;
    if (t.game == GAME_GO) {
        t.rko[g] = s.ko; t.rpass[g] = s.passes; t.rcap[2 * g] = s.cap[0]; t.rcap[2 * g + 1] = s.cap[1];
        t.rnposh[g] = s.nh;
    }
    t.gresult[g] = s.res; t.active[g] = s.res == R_ONGOING;
}

// One Go stone move against the rules, as getLegalMoves judges its candidates (go_legal above: the same
// suicide test and the same resulting-position hash -- the mover to move, the old ko point -- against the
// position history hist[0, nh)).  go_groups(.., &keys) must have run on the board; every lane of the wave
// calls it with the same arguments and gets the same answer: an AZ_OPEN_* reason, 0 when the move is legal.
__device__ __forceinline__ int go_move_reason(const TreeDev& t, const uint8_t* b, const GoLds& L, int lane, int a, int player,
                                              int ko, uint64_t bh, const uint64_t* hist, int nh) {
    const int A = t.A;
    if (b[a] != 0) return AZ_OPEN_OCCUPIED;
    if (a == ko) return AZ_OPEN_KO;
    int nb[4], capg[4], nc = 0;
    const int k = go_adj(a, t.bs, A, nb);
    bool alive = false;
    uint64_t h = bh ^ t.zpiece[(size_t)(player - 1) * A + a];
    for (int q = 0; q < k; ++q) {
        const int e = nb[q], v = b[e];
        if (v == 0) { alive = true; continue; }
        const int gi = L.gid[e];
        if (v == player) { if (L.glib[gi] >= 2) alive = true; continue; }
        if (L.glib[gi] == 1) {                    // its only liberty is a: captured
            bool dup = false;
            for (int r = 0; r < nc; ++r) dup |= capg[r] == gi;
            if (!dup) { capg[nc++] = gi; h ^= L.gxor[gi]; }
        }
    }
    if (!alive && nc == 0) return AZ_OPEN_SUICIDE;
    if (!t.superko) return 0;
    const uint64_t hc = h ^ t.zplayer[player - 1] ^ (ko >= 0 ? t.zko[ko] : 0ULL) ^ t.zconst;
    bool hit = false;
    for (int r = lane; r < nh; r += 64) hit |= hist[r] == hc;
    return __ballot(hit) != 0ULL ? AZ_OPEN_SUPERKO : 0;
}

// The judge: action a on position s (its board in LDS, complete; Go's position history in ph[0, s.nh))
// against the rules, where make_move / makeMove of the reference throw (gomoku_state.cpp:697-703,
// go_state.cpp:192-200) -- the AZ_OPEN_* reason, 0 when the move is legal (Go: the pass always is).  Every
// lane of the wave calls it with the same arguments and gets the same answer.
__device__ __forceinline__ int move_reason(const TreeDev& t, const RootPos& s, const uint8_t* board, GoLds& gl, int lane,
                                           int a, const uint64_t* ph) {
    const bool go = t.game == GAME_GO;
    if (s.res != R_ONGOING) return AZ_OPEN_ENDED;
    if (a < (go ? -1 : 0) || a >= t.A) return AZ_OPEN_RANGE;
    if (go) {
        if (a < 0) return 0;
        GoKeys gk;
        go_keys(t, board, s.player, lane, gk);
        go_groups(t, board, gl, lane, 64, &gk);
        return go_move_reason(t, board, gl, lane, a, s.player, s.ko, s.hash, ph, s.nh);
    }
    if (board[a] != 0) return AZ_OPEN_OCCUPIED;
    if ((t.renju || t.omok) && s.player == 1) {
        const bool base = __ballot(gomoku_base_shapes(board, t.bs, t.renju, t.omok, lane, 64)) != 0ULL;
        if (gomoku_forbidden(board, t.bs, t.renju, t.omok, a, base)) return AZ_OPEN_FORBIDDEN;
    }
    return 0;
}

// lane 0's value on every lane, after a branch only lane 0 took
__device__ __forceinline__ int lane0(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The move: legal action a turns s and its board (LDS) into the position after it, GomokuState::make_move
// (gomoku_state.cpp:681-722) / GoState::makeMove (go_state.cpp:192-257) with the result of the new position.
// Go: captures stay on lane 0 (go_play_seq); a stone move under superko pushes the new position onto the
// history ph[0, s.nh) of capacity hcap (simple ko keeps none); two passes end the game (go_result_seq).
// Gomoku: a five, the full board, or -- Renju / Omok -- Black left without a legal cell (is_stalemate,
// gomoku_state.cpp:506-521; forb: LDS room for that mask, which nothing reads afterwards: the selection
// builds the mask of the leaf it expands).  Every lane of the wave calls it with the same arguments; the
// board is complete again on return.
__device__ __forceinline__ void root_move(const TreeDev& t, RootPos& s, uint8_t* board, GoLds& gl, uint64_t* forb, int lane,
                                          int a, uint64_t* ph, int hcap) {
    const int A = t.A, p = s.player;
    if (t.game == GAME_GO) {
        go_clear_marks(gl, A, lane);
        int k = s.ko, ps = s.passes, cap[2] = {s.cap[0], s.cap[1]}, nh = s.nh, res = R_ONGOING;
        uint64_t bh = s.hash;
        if (lane == 0) {
            if (go_play_seq(t, board, gl, a, p, k, ps, bh, nullptr, cap) && t.superko) {
                if (nh >= hcap) atomicOr(t.err, ERR_HIST);
                else ph[nh++] = go_hash(t, bh, p, k);
            }
            if (ps >= 2) res = go_result_seq(t, board, gl, cap);
        }
        s.ko = lane0(k); s.passes = lane0(ps); s.cap[0] = lane0(cap[0]); s.cap[1] = lane0(cap[1]); s.nh = lane0(nh);
        s.res = lane0(res); s.hash = lane_read64(bh, 0);
        s.stones += a >= 0 ? 1 : 0;
        __syncthreads();                          // lane 0's board for every lane
    } else {
        __syncthreads();                          // the judging reads of the board are over
        if (lane == 0) board[a] = (uint8_t)p;
        __syncthreads();
        s.stones += 1;
        if (five_at_wave(board, t.bs, a, p, lane)) s.res = p == 1 ? R_WIN1 : R_WIN2;
        else if (s.stones >= A) s.res = R_DRAW;
        else if ((t.renju || t.omok) && p == 2 && forbidden_mask_wave(t, board, lane, forb) == 0) s.res = R_DRAW;
        s.hash ^= t.zpiece[(size_t)(p - 1) * A + a] ^ t.zplayer[p - 1] ^ t.zplayer[2 - p];
    }
    for (int j = 5; j > 0; --j) s.h6[j] = s.h6[j - 1];
    s.h6[0] = a;
    s.player = 3 - p;
    s.ply += 1;
}

// A game starts in slot g at position s: a new tree (one root node), the game's counters at zero, the
// RANDOM evaluator's generator seeded for the game's stream id (std::mt19937(eval_seed + id)), then the
// position.  TT visits are cleared by the caller (k_tt_clear).  Every lane of the wave calls it.
__device__ __forceinline__ void slot_start(const TreeDev& t, int g, int lane, const RootPos& s, const uint8_t* board,
                                           uint32_t seed) {
    long long* cnt = t.cnt + (size_t)g * AZ_NCNT;
    if (lane < CNT_EVALS_TOTAL) cnt[lane] = 0;
    if (lane == 0) {
        t.rnode[g] = 0; t.atop[g] = 1; t.ring_cur[g] = 0;
        node_clear(game_nodes(t.nd, (size_t)g * t.ncap), 0);
        if (t.mt) mt_seed(t.mt + (size_t)g * 625, seed);
    }
    root_store(t, g, lane, s, board);
}

// updateWithMove's subtree reuse (parallel_mcts.cpp:1065-1108): the child that played `a`
// becomes the root, else a fresh root node.  Lane 0.
// returns the flag of the new root (0 for a fresh node)
__device__ uint8_t reuse_child(const TreeDev& t, int g, const GamePtrs& nd, int a) {
    const int root = t.rnode[g];
    const int fc = nd.first[root], nc = nd.cnt[root];
    int child = -1;
    for (int i = 0; i < nc; ++i) if (nd.act[fc + i] == a) { child = fc + i; break; }
    if (child < 0) {
        child = t.atop[g];
        if (child + 1 > t.ncap) { atomicOr(t.err, ERR_NODES); child = 0; }
        else t.atop[g] = child + 1;
        node_clear(nd, child);
        t.rnode[g] = child;
        return 0;
    }
    t.rnode[g] = child;
    return nd.flag[child];
}
}  // namespace

// K5: makeMove + updateWithMove; terminal test of the new root (game loop condition).
// rexp[g] (optional): 1 when the game's root after the move needs no root expansion (expanded or
// terminal, or the game is not playing) -- the host then skips the no-op root steps
__global__ __launch_bounds__(64) void k_apply(TreeDev t, const int* actions, int* terminal, int* result, int* rexp) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ uint8_t board[AZ_MAXA];
    __shared__ GoLds gl;
    __shared__ uint64_t forb[AZ_FORB_WORDS];
    if (g >= t.G) return;
    const int a = actions[g];
    const int A = t.A;
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    if (!t.active[g] || a < (t.game == GAME_GO ? -1 : 0) || a >= A) {          // Go: -1 is the pass
        if (lane == 0) {
            terminal[g] = t.active[g] ? 0 : 1; result[g] = t.gresult[g];
            if (rexp) rexp[g] = t.active[g] ? ((nd.flag[t.rnode[g]] & (FL_EXPANDED | FL_TERMINAL)) != 0) : 1;
        }
        return;
    }
    RootPos s = root_load(t, g);
    const uint8_t* rb = t.rboard + (size_t)g * A;
    for (int i = lane; i < A; i += 64) board[i] = rb[i];
    __syncthreads();
    root_move(t, s, board, gl, forb, lane, a, t.rposh + (size_t)g * t.hmax, t.hmax);
    root_store(t, g, lane, s, board);
    if (lane == 0) {
        terminal[g] = s.res != R_ONGOING;
        result[g] = s.res;
        const uint8_t fl = reuse_child(t, g, nd, a);
        if (rexp) rexp[g] = s.res != R_ONGOING || (fl & (FL_EXPANDED | FL_TERMINAL)) != 0;
    }
}

// The moves az_search_apply is about to commit, against the rules: bad[g] = the judge's AZ_OPEN_* reason
// for actions[g] on game g's root position, 0 for a legal move, a pass, no move or a game that is not
// playing.  One wave per game; launched on a Go handle and on a Gomoku handle with rules.
__global__ __launch_bounds__(64) void k_illegal_moves(TreeDev t, const int* actions, int* bad) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ uint8_t board[AZ_MAXA];
    __shared__ GoLds gl;
    if (g >= t.G) return;
    const int a = actions[g], A = t.A;
    if (!t.active[g] || a < 0 || a >= A) { if (lane == 0) bad[g] = 0; return; }
    const RootPos s = root_load(t, g);
    const uint8_t* rb = t.rboard + (size_t)g * A;
    for (int i = lane; i < A; i += 64) board[i] = rb[i];
    __syncthreads();
    const int why = move_reason(t, s, board, gl, lane, a, t.rposh + (size_t)g * t.hmax);
    if (lane == 0) bad[g] = why;
}

// K8: fresh games (empty board, new tree; TT visits cleared by the caller).
__global__ __launch_bounds__(64) void k_new_games(TreeDev t, const int* games, const int* seed_ids, int n,
                                                  uint32_t eval_seed) {
    const int idx = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ uint8_t board[AZ_MAXA];
    if (idx >= n) return;
    const int g = games[idx];
    for (int i = lane; i < t.A; i += 64) board[i] = 0;
    __syncthreads();
    slot_start(t, g, lane, root_empty(t), board, eval_seed + (uint32_t)(seed_ids ? seed_ids[idx] : g));
}

// Openings: fresh games in the listed slots, each advanced by its own move sequence in one launch -- what
// k_new_games and one k_apply (+ k_compact) per move leave behind, field for field (the same routines make
// it), with every move judged against the rules first.  One wave per listed slot; the board lives in LDS.
// o.rep[AZ_OPEN_REP idx ..]: {first bad ply or -1, its AZ_OPEN_* reason, the game still playing after the
// opening, its GameResult, the random plies played}.  dry: the same pass without a
// single store to the slot (Go's position history then grows in o.hist, o.hstride per entry, instead of the
// slot's own); the host validates with it, so the storing pass never meets a bad move.
// Random plies: after the sequence up to o.rplies further plies are drawn here.  Ply j (the game's real ply
// number) of the game with stream id `id` draws Philox4x32-10 with key (o.key_lo, o.key_hi) and counter
// (id, j, 0, 0) and plays legal[(out0 * n_legal) >> 32] of the side to move's legal moves in ascending order
// (Gomoku: the empty cells less the forbidden ones; Go: go_legal's set without the pass).  A pick that would
// end the game is not played and the opening stops there, as it does at an empty list: random plies never end
// a game.  o.picks[o.rplies idx ..] are the plies played.
__global__ __launch_bounds__(64) void k_open_games(TreeDev t, OpenDev o) {
    const int idx = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ uint8_t board[AZ_MAXA];
    __shared__ GoLds gl;
    __shared__ uint64_t forb[AZ_FORB_WORDS];
    __shared__ int legal[AZ_MAXNA];
    const int n = o.n, dry = o.dry;
    if (idx >= n) return;
    const int g = o.games ? o.games[idx] : 0;
    const int A = t.A;
    const bool go = t.game == GAME_GO;
    const int seq = o.seq_of ? o.seq_of[idx] : idx;
    const int nm = o.n_moves ? o.n_moves[seq] : 0;
    const int* mv = o.moves + (size_t)seq * o.stride;
    const int sid = o.seed_ids ? o.seed_ids[idx] : g;
    const uint32_t rid = (uint32_t)(o.rand_ids ? o.rand_ids[idx] : sid);
    uint64_t* ph = dry ? o.hist + (size_t)idx * o.hstride : t.rposh + (size_t)g * t.hmax;
    const int hcap = dry ? o.hstride : t.hmax;
    for (int i = lane; i < A; i += 64) board[i] = 0;
    RootPos s = root_empty(t);                    // the game's position, the same on every lane
    int bad = -1, why = 0, nrand = 0;
    if (lane == 0) gl.nph = 0;                    // go_legal_hist: no path pushes, the history is ph[0, s.nh)
    __syncthreads();
    for (int i = 0; i < nm + o.rplies; ++i) {
        int a;
        if (i >= nm) {
            // a random ply: the side to move's legal moves in ascending order, one picked by the game's stream
            if (s.res != R_ONGOING) break;
            uint32_t c[4] = {rid, (uint32_t)i, 0u, 0u};
            philox4x32_10(c, o.key_lo, o.key_hi);
            int nl;
            if (go) {
                GoKeys gk;
                go_keys(t, board, s.player, lane, gk);
                go_groups(t, board, gl, lane, 64, &gk);
                nl = go_legal_hist(t, ph, t.superko ? s.nh : 0, lane, board, gl, s.player, s.ko, s.hash, legal, gk) - 1;   // [0]: the pass
                if (nl <= 0) break;
                a = legal[1 + (int)(((uint64_t)c[0] * (uint64_t)nl) >> 32)];
            } else {
                const bool masked = (t.renju || t.omok) && s.player == 1;
                if (masked) forbidden_mask_wave(t, board, lane, forb);
                __syncthreads();
                nl = 0;
                for (int c0 = 0; c0 < A; c0 += 64) {
                    const int q = c0 + lane;
                    const bool ok = q < A && board[q] == 0 && !(masked && (forb[c0 >> 6] >> lane & 1ULL));
                    const unsigned long long m = __ballot(ok);
                    if (ok) legal[nl + __popcll(m & ((1ULL << lane) - 1ULL))] = q;
                    nl += __popcll(m);
                }
                __syncthreads();
                if (nl <= 0) break;
                a = legal[(int)(((uint64_t)c[0] * (uint64_t)nl) >> 32)];
            }
        } else {
            a = mv[i];
            why = move_reason(t, s, board, gl, lane, a, ph);   // a random ply is legal by construction
            if (why) { bad = i; break; }
        }
        const RootPos before = s;
        root_move(t, s, board, gl, forb, lane, a, ph, hcap);
        if (i >= nm) {
            if (s.res != R_ONGOING) {
                // a random ply never ends the game: the stone comes off again (Gomoku; Go's picks leave out
                // the pass, the one move that ends a game)
                __syncthreads();
                if (lane == 0) board[a] = 0;
                __syncthreads();
                s = before;
                break;
            }
            if (lane == 0 && o.picks) o.picks[(size_t)idx * o.rplies + nrand] = a;
            ++nrand;
        }
    }
    if (lane == 0) {
        int* rep = o.rep + AZ_OPEN_REP * idx;
        rep[0] = bad; rep[1] = why; rep[2] = bad < 0 && s.res == R_ONGOING; rep[3] = s.res; rep[4] = nrand;
    }
    if (dry || bad >= 0) return;
    __syncthreads();
    slot_start(t, g, lane, s, board, o.eval_seed + (uint32_t)sid);
}

// Every slot of a new handle as an idle game: a valid root (node 0 of both arenas, no children),
// inactive.  Kernels that run over every slot (k_apply, k_compact, k_prune copy every game's tree
// when the arenas flip) then never read an uninitialised root index; k_new_games starts a game.
__global__ void k_init_slots(TreeDev t, Nodes other) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    t.rnode[g] = 0; t.atop[g] = 1; t.active[g] = 0; t.gresult[g] = R_ONGOING; t.ring_cur[g] = 0;
    t.rplayer[g] = 1; t.rstones[g] = 0; t.rply[g] = 0; t.rfresh[g] = 1; t.rhash[g] = 0;
    node_clear(game_nodes(t.nd, (size_t)g * t.ncap), 0);
    node_clear(game_nodes(other, (size_t)g * t.ncap), 0);
}

// TT clear for the listed games (visits == 0 marks an empty slot).
__global__ void k_tt_clear(TreeDev t, const int* games, int n) {
    const int idx = blockIdx.y;
    if (idx >= n) return;
    int* v = t.tt_visits + (size_t)games[idx] * t.tt_slots;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.tt_slots; i += gridDim.x * blockDim.x) v[i] = 0;
}

// Root children readback helper (tests / records).
__global__ void k_root_children(TreeDev t, int g, int* act, int* N, int* VL, float* W, float* P, int* n, int* rootinfo,
                                float* rootW) {
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    const int root = t.rnode[g];
    const int fc = nd.first[root], nc = nd.cnt[root];
    for (int i = threadIdx.x; i < nc; i += blockDim.x) {
        act[i] = nd.act[fc + i]; N[i] = nd.N[fc + i]; VL[i] = nd.VL[fc + i]; W[i] = nd.W[fc + i]; P[i] = nd.P[fc + i];
    }
    if (threadIdx.x == 0) { *n = nc; rootinfo[0] = nd.N[root]; rootinfo[1] = nd.VL[root]; *rootW = nd.W[root]; }
}

// Root child counts (host-side Dirichlet draws need |children| per game).
__global__ void k_root_nchild(TreeDev t, int* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= t.G) return;
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    const int root = t.rnode[g];
    out[g] = (nd.flag[root] & FL_EXPANDED) ? (int)nd.cnt[root] : 0;
}

// ---------------------------------------------------------------------------
// K-D: training examples (Dataset::extractExamples, src/selfplay/dataset.cpp:60-114, with
// augmentExample :245-436).  One wave per game replays the record (GomokuState / GoState
// makeMove on the LDS board), builds the position's planes in LDS (getEnhancedTensorRepresentation)
// and writes the K = 8 (or 1) examples of every position straight to their shuffled slots:
// no intermediate copy, HBM-bound on the example writes.
//
// Symmetry s maps a state pixel (row, col) to a destination; the kernel runs it backwards
// (src[s][dest]) so the writes are contiguous.  The reference's order: 0 original, 1 rot90
// (i,j)->(j,bs-1-i), 2 rot180, 3 rot270 (i,j)->(bs-1-j,i), 4 flipH (i,j)->(i,bs-1-j),
// 5..7 flipH applied to rot90 / rot180 / rot270 (:372-433).
namespace {
__device__ __forceinline__ int sym_src(int s, int a, int bs) {
    const int r = a / bs, c = a % bs, m = bs - 1;
    switch (s) {
        case 1: return (m - c) * bs + r;
        case 2: return (m - r) * bs + (m - c);
        case 3: return c * bs + (m - r);
        case 4: return r * bs + (m - c);
        case 5: return c * bs + r;
        case 6: return (m - r) * bs + c;
        case 7: return (m - c) * bs + (m - r);
        default: return a;
    }
}
}  // namespace

__global__ __launch_bounds__(AZ_DS_THREADS) void k_dataset_extract(DatasetDev d, TreeDev t) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;                 // AZ_DS_THREADS threads (4 waves) per game
    if (g >= d.n_games) return;
    const int bs = d.bs, A = d.A, C = d.C, K = d.K, NA = d.NA;
    __shared__ uint8_t board[AZ_MAXA];
    __shared__ float pl[11 * AZ_MAXA];          // planes of the current position, [C][A]
    __shared__ float pin[AZ_MAXNA];             // the move's child-order policy
    __shared__ int16_t src[8][AZ_MAXA];         // sym_src tables
    __shared__ GoLds L;
    __shared__ int hist6[6];
    __shared__ int s_ko;
    for (int a = lane; a < A; a += AZ_DS_THREADS) {
        board[a] = 0;
        for (int s = 0; s < K; ++s) src[s][a] = (int16_t)sym_src(s, a, bs);
    }
    if (lane < 6) hist6[lane] = -1;
    int player = 1, ko = -1, passes = 0;
    uint64_t bh = 0;
    // GameResult -> value of player 1 (:83-89); flipped for player 2 as -gameValue (-0.0f for draws)
    const int res = d.results[g];
    const float gv = res == R_WIN1 ? 1.0f : res == R_WIN2 ? -1.0f : 0.0f;
    const int m0 = d.move_off[g], m1 = d.move_off[g + 1];
    __syncthreads();
    for (int m = m0; m < m1; ++m) {
        // ---- planes of the position before move m
        if (d.game == GAME_GO) {
            go_clear_marks(L, A, lane);
            go_groups(t, board, L, lane, AZ_DS_THREADS);
            const float half = (float)(bs / 2);
            for (int a = lane; a < A; a += AZ_DS_THREADS) {
                const int v = board[a];
                const int x = a % bs, y = a / bs;
                pl[a] = v == 1 ? 1.0f : 0.0f;
                pl[A + a] = v == 2 ? 1.0f : 0.0f;
                pl[2 * A + a] = player == 1 ? 1.0f : 0.0f;
                const float lib = v ? fminf(1.0f, (float)L.glib[L.gid[a]] / 10.0f) : 0.0f;
                pl[3 * A + a] = v == 1 ? lib : 0.0f;
                pl[4 * A + a] = v == 2 ? lib : 0.0f;
                pl[5 * A + a] = a == ko ? 1.0f : 0.0f;
                pl[6 * A + a] = (float)min(x, bs - 1 - x) / half;
                pl[7 * A + a] = (float)min(y, bs - 1 - y) / half;
            }
        } else {
            int hp[6];
            for (int i = 0; i < 6; ++i) hp[i] = (((player == 1) == ((i % 2) == 0)) ? 3 : 6) + i / 2;
            for (int a = lane; a < A; a += AZ_DS_THREADS) {
                float c[11];
                for (int k = 0; k < 11; ++k) c[k] = 0.0f;
                const int v = board[a];
                if (v == player) c[0] = 1.0f;
                else if (v == 3 - player) c[1] = 1.0f;
                if (player == 1) c[2] = 1.0f;
                for (int i = 0; i < 6; ++i)
                    if (hist6[i] == a) c[hp[i]] = 1.0f;
                c[9] = (float)(a / bs) / (float)(bs - 1);
                c[10] = (float)(a % bs) / (float)(bs - 1);
                for (int k = 0; k < 11; ++k) pl[k * A + a] = c[k];
            }
        }
        const int n = d.n_children[m];
        const float* pg = d.policies + d.pol_off[m];
        for (int k = lane; k < n; k += AZ_DS_THREADS) pin[k] = pg[k];
        __syncthreads();
        const float val = player == 2 ? -gv : gv;
        for (int s = 0; s < K; ++s) {
            const long long e = (long long)m * K + s;
            const long long slot = d.dst ? d.dst[e] : e;
            float* o = d.states + slot * (long long)(C * A);
            for (int ca = lane; ca < C * A; ca += AZ_DS_THREADS) {
                const int c = ca / A, a = ca - c * A;
                o[ca] = pl[c * A + src[s][a]];
            }
            // policy: the reference permutes the child-order vector by board index, guarded by
            // oldIdx/newIdx < size; entries it does not overwrite keep the copied value
            float* op = d.policy + slot * (long long)NA;
            for (int k = lane; k < NA; k += AZ_DS_THREADS) {
                float v = 0.0f;
                if (k < n) {
                    if (s == 0) {
                        v = pin[k];
                    } else if (s <= 4) {
                        const int j = k < A ? src[s][k] : n;
                        v = (k < A && j < n) ? pin[j] : pin[k];
                    } else {
                        const int f = k < A ? src[4][k] : n;       // flip source, then the rotation
                        const int q = (k < A && f < n) ? f : k;
                        const int r = q < A ? src[s - 4][q] : n;
                        v = (q < A && r < n) ? pin[r] : pin[q];
                    }
                }
                op[k] = v;
            }
            if (lane == 0) { d.plen[slot] = n; d.value[slot] = val; }
        }
        __syncthreads();
        // ---- makeMove
        const int a = d.actions[m];
        if (d.game == GAME_GO) {
            go_clear_marks(L, A, lane);
            if (lane == 0) go_play_seq(t, board, L, a, player, ko, passes, bh);
        } else if (lane == 0) {
            board[a] = (uint8_t)player;
            for (int i = 5; i > 0; --i) hist6[i] = hist6[i - 1];
            hist6[0] = a;
        }
        player = 3 - player;
        if (lane == 0) s_ko = ko;
        __syncthreads();
        ko = s_ko;
    }
}

// Example gather (getBatch / getRandomSubset / shuffle): destination row i <- source row idx[i];
// one block per row, 16-byte copies when the row length allows.
__global__ __launch_bounds__(256) void k_dataset_gather(const float* states, const float* policy, const int* plen,
                                                        const float* value, int row, int NA, const long long* idx,
                                                        int n, float* ostates, float* opolicy, int* oplen,
                                                        float* ovalue) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const long long j = idx[i];
    const float* s = states + j * row;
    float* o = ostates + (long long)i * row;
    if ((row & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(s);
        float4* o4 = reinterpret_cast<float4*>(o);
        for (int k = threadIdx.x; k < row / 4; k += 256) o4[k] = s4[k];
    } else {
        for (int k = threadIdx.x; k < row; k += 256) o[k] = s[k];
    }
    for (int k = threadIdx.x; k < NA; k += 256) opolicy[(long long)i * NA + k] = policy[j * NA + k];
    if (threadIdx.x == 0) { oplen[i] = plen[j]; ovalue[i] = value[j]; }
}

// ---------------------------------------------------------------------------
// Replay buffer (az_replay_*, replay.hip; layout: ReplayDev in tree.h).
//
// K-R1: one wave per game slot, between k_select_action and k_apply: the root children's visit counts scattered to
// action index (clamped at 0: progressive widening leaves negative N) and the root's position record -- what
// write_leafrec / go_write_leafrec store for a leaf, here for the root -- into the slot's next staging row.
__global__ __launch_bounds__(64) void k_replay_stage(TreeDev t, ReplayDev r, const int* actions, const float* values) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    __shared__ uint8_t board[AZ_MAXA];
    __shared__ int cnt[AZ_MAXNA];
    __shared__ GoLds gl;
    if (g >= t.G) return;
    const bool go = t.game == GAME_GO;
    if (!t.active[g] || actions[g] == (go ? -2 : -1)) return;     // no move: nothing staged
    const int A = t.A, NA = t.NA;
    GamePtrs nd = game_nodes(t.nd, (size_t)g * t.ncap);
    const int root = t.rnode[g];
    const int fc = nd.first[root], nc = min((int)nd.cnt[root], NA);
    for (int k = lane; k < NA; k += 64) cnt[k] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nc; i += 64) {
        const int a = nd.act[fc + i];
        const int v = max(0, nd.N[fc + i]);
        const int k = a < 0 ? A : a;                               // Go's pass (-1) sits at A
        if (k < NA) { cnt[k] = v; sum += v; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (sum <= 0) {
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(r.ctr + RP_SKIPPED), 1ULL);
        return;
    }
    const int n = r.st_n[g];
    if (n >= r.max_plies) {
        if (lane == 0) atomicAdd(reinterpret_cast<unsigned long long*>(r.ctr + RP_DROPPED), 1ULL);
        return;
    }
    const uint8_t* rb = t.rboard + (size_t)g * A;
    for (int a = lane; a < A; a += 64) board[a] = rb[a];
    __syncthreads();
    const size_t row = (size_t)g * r.max_plies + n;
    uint8_t* rec = r.st.rec + row * r.rec;
    if (go) {
        go_groups(t, board, gl, lane, 64);
        for (int a = lane; a < A; a += 64) {
            rec[a] = board[a];
            rec[A + a] = board[a] ? (uint8_t)min(10, (int)gl.glib[gl.gid[a]]) : 0;
        }
    } else {
        for (int a = lane; a < A; a += 64) rec[a] = board[a];
    }
    int* meta = reinterpret_cast<int*>(rec + r.moff);
    const int player = t.rplayer[g];
    if (lane == 0) meta[0] = player;
    if (lane == 1) meta[1] = go ? t.rko[g] : -1;
    if (lane < 6) meta[2 + lane] = go ? -1 : t.rhist[g * 6 + lane];
    int* crow = r.st.cnt + row * NA;
    for (int k = lane; k < NA; k += 64) crow[k] = cnt[k];
    if (lane == 0) {
        r.st.sum[row] = sum; r.st.q[row] = values[g]; r.st.gid[row] = r.slot_gid[g]; r.st.ply[row] = t.rply[g];
        r.st.player[row] = player;
        r.st_n[g] = n + 1;
    }
}

// K-R2: one block per finished slot (slots ascending): its staged rows go to the ring behind those of the slots before
// it, position k of the commit order at ring row k % capacity, with z for the side to move.  Rows that the same
// commit would overwrite again (more than `capacity` positions at once) are not written.  The last block to finish
// moves the head and empties the slots' staging.
__global__ __launch_bounds__(256) void k_replay_commit(ReplayDev r, const int* slots, const int* results, int n) {
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ unsigned long long s_before, s_total;
    if (i >= n) return;
    if (tid == 0) { s_before = 0; s_total = 0; }
    __syncthreads();
    unsigned long long before = 0, total = 0;
    for (int j = tid; j < n; j += 256) {
        const unsigned long long c = (unsigned long long)r.st_n[slots[j]];
        if (j < i) before += c;
        total += c;
    }
    if (before) atomicAdd(&s_before, before);
    if (total) atomicAdd(&s_total, total);
    __syncthreads();
    const long long head = r.ctr[RP_HEAD];
    const long long base = head + (long long)s_before, end = head + (long long)s_total;
    const int g = slots[i];
    const int cnt = r.st_n[g];
    const int res = results[i];
    const int NA = r.NA, rec16 = r.rec / 16;
    for (int p = 0; p < cnt; ++p) {
        const long long k = base + p;
        if (k < end - r.capacity) continue;
        const size_t src = (size_t)g * r.max_plies + p, dst = (size_t)(k % r.capacity);
        const uint4* s4 = reinterpret_cast<const uint4*>(r.st.rec + src * r.rec);
        uint4* d4 = reinterpret_cast<uint4*>(r.ring.rec + dst * r.rec);
        for (int x = tid; x < rec16; x += 256) d4[x] = s4[x];
        for (int x = tid; x < NA; x += 256) r.ring.cnt[dst * NA + x] = r.st.cnt[src * NA + x];
        if (tid == 0) {
            const int player = r.st.player[src];
            const float gv = res == R_WIN1 ? 1.0f : res == R_WIN2 ? -1.0f : 0.0f;
            r.ring.z[dst] = gv == 0.0f ? 0.0f : (player == 2 ? -gv : gv);
            r.ring.sum[dst] = r.st.sum[src]; r.ring.q[dst] = r.st.q[src]; r.ring.gid[dst] = r.st.gid[src];
            r.ring.ply[dst] = r.st.ply[src]; r.ring.player[dst] = player;
        }
    }
    __syncthreads();
    if (tid == 0) {
        __threadfence();
        const unsigned long long done = atomicAdd(reinterpret_cast<unsigned long long*>(r.ctr + RP_DONE), 1ULL);
        if (done == (unsigned long long)(n - 1)) {     // every block has read the staged counts and the head
            for (int j = 0; j < n; ++j) r.st_n[slots[j]] = 0;
            r.ctr[RP_HEAD] = end;
            r.ctr[RP_GAMES] += n;
            r.ctr[RP_DONE] = 0;
        }
    }
}

// K-R3: one block per sample.  The record of ring row idx[i] is mapped by symmetry sym[i] into LDS -- every cell with
// its liberties, the last moves and the ko point -- and az_leaf_planes_v builds the planes of the MAPPED position, so
// the coordinate planes are what the net sees in play; the policy count / sum is permuted by the same cell map (the
// pass stays).  Plane and policy stores are contiguous over the threads.
__global__ __launch_bounds__(256) void k_replay_gather(ReplayDev r, const long long* idx, const int* sym, int n,
                                                       float* states, float* policy, float* z, float* q, int* gid,
                                                       int* ply) {
#pragma clang fp contract(off)
    const int i = blockIdx.x;
    const int tid = threadIdx.x;
    __shared__ uint8_t mb[AZ_MAXA], ml[AZ_MAXA];
    __shared__ int meta[8];
    __shared__ float pol[AZ_MAXNA];
    if (i >= n) return;
    const long long j = idx[i];
    const int s = sym ? sym[i] : 0;
    const int A = r.A, NA = r.NA, bs = r.bs, C = r.C;
    const int go = r.game == GAME_GO;
    const uint8_t* rec = r.ring.rec + (size_t)j * r.rec;
    const int* cnt = r.ring.cnt + (size_t)j * NA;
    const float fsum = (float)r.ring.sum[j];
    for (int a = tid; a < A; a += 256) {
        const int d = replay_sym_cell(bs, s, a);
        mb[d] = rec[a];
        ml[d] = go ? rec[A + a] : (uint8_t)0;
        pol[d] = (float)cnt[a] / fsum;
    }
    if (tid == 0 && NA > A) pol[A] = (float)cnt[A] / fsum;
    if (tid < 8) {
        int v = reinterpret_cast<const int*>(rec + r.moff)[tid];
        if (tid >= 1 && v >= 0 && v < A) v = replay_sym_cell(bs, s, v);
        meta[tid] = v;
    }
    __syncthreads();
    float* o = states + (size_t)i * C * A;
    for (int a = tid; a < A; a += 256) {
        float c[16];
        az_leaf_planes_v(mb[a], ml[a], meta, go, bs, a, c);
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < C) o[(size_t)k * A + a] = c[k];
    }
    for (int k = tid; k < NA; k += 256) policy[(size_t)i * NA + k] = pol[k];
    if (tid == 0) {
        if (z) z[i] = r.ring.z[j];
        if (q) q[i] = r.ring.q[j];
        if (gid) gid[i] = r.ring.gid[j];
        if (ply) ply[i] = r.ring.ply[j];
    }
}

// The raw counts rows of ring rows idx[0..n) (tests, diagnostics).
__global__ __launch_bounds__(256) void k_replay_counts(ReplayDev r, const long long* idx, int n, int* counts, int* sum) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const long long j = idx[i];
    for (int k = threadIdx.x; k < r.NA; k += 256) counts[(size_t)i * r.NA + k] = r.ring.cnt[(size_t)j * r.NA + k];
    if (threadIdx.x == 0 && sum) sum[i] = r.ring.sum[j];
}

void az_launch_replay_stage(const TreeDev& t, const ReplayDev& r, const int* actions, const float* values, hipStream_t st) {
    hipLaunchKernelGGL(k_replay_stage, dim3(t.G), dim3(64), 0, st, t, r, actions, values);
}
void az_launch_replay_commit(const ReplayDev& r, const int* slots, const int* results, int n, hipStream_t st) {
    hipLaunchKernelGGL(k_replay_commit, dim3(n), dim3(256), 0, st, r, slots, results, n);
}
void az_launch_replay_gather(const ReplayDev& r, const long long* idx, const int* sym, int n, float* states, float* policy,
                             float* z, float* q, int* gid, int* ply, hipStream_t st) {
    hipLaunchKernelGGL(k_replay_gather, dim3(n), dim3(256), 0, st, r, idx, sym, n, states, policy, z, q, gid, ply);
}
void az_launch_replay_counts(const ReplayDev& r, const long long* idx, int n, int* counts, int* sum, hipStream_t st) {
    hipLaunchKernelGGL(k_replay_counts, dim3(n), dim3(256), 0, st, r, idx, n, counts, sum);
}
