// tree.h -- device-side data layout of the batched search (G independent games).
//
// Flat structure-of-arrays node pool per game (two arenas, compacted after every
// committed move), per-game root state, per-step scratch, a direct-mapped
// transposition-table emulation per game and a prior ring that keeps the children
// priors of every TT entry alive for later hits.  See DESIGN.md "Data layout in HBM".
#pragma once
#include <stddef.h>
#include <stdint.h>

#define AZ_MAXA 361          // largest board handled on device (19x19)
#define AZ_MAXNA 362         // largest action space (Go 19x19: 361 points + pass)
#define AZ_SCAN_NETS 4        // nets k_scan_nets partitions a leaf batch by (AZ_MAX_SLOT_NETS of az_engine.h)
#define AZ_DMAX 96          // longest selection path (root + 95 plies); overflow => AZ_ERR_CAPACITY
#define AZ_NCNT 8            // per-game counters
#define AZ_FORB_WORDS ((AZ_MAXA + 63) / 64)   // 64-cell words of a forbidden-cell mask
// Go leaf state (k_select -> k_expand_backup): [0, 384) board, [384, 416) int32 {player, ko, passes,
// nph} + u64 stones hash, [416, 416 + 8 * AZ_DMAX) u64 position pushes of the path
#define AZ_GOLEAF_BYTES (416 + 8 * AZ_DMAX)

// ST_EXPANDED: the leaf is already expanded (a childless node after releaseMemory, or the depth
// cap): TT lookup, value = getValue() on a miss; ST_EXPVAL: the same with a TT hit (value cached)
enum { ST_NONE = 0, ST_TERMINAL = 1, ST_TTHIT = 2, ST_EVAL = 3, ST_EXPANDED = 4, ST_EXPVAL = 5 };
enum { MODE_SIM = 0, MODE_ROOT_NOISE = 1, MODE_ROOT_SEARCH = 2 };
enum { FL_EXPANDED = 1, FL_TERMINAL = 2 };   // result (GameResult) in bits 2..3
enum { CNT_EVALS = 0, CNT_LOOKUPS = 1, CNT_HITS = 2, CNT_SIMS = 3, CNT_NODES = 4, CNT_EVALS_TOTAL = 5,
       CNT_BYTES_SEL = 6, CNT_BYTES_EXP = 7 };   // [5..7] survive new games; 6/7: algorithmic HBM bytes of K1 / K3
enum { ERR_NODES = 1, ERR_PATH = 2, ERR_RING = 4, ERR_BATCH = 8, ERR_HIST = 16, ERR_WIDEN = 32 };
// MCTSNodeSelection (include/alphazero/mcts/parallel_mcts.h:26-31); RAVE plays PUCT (selectChildRave)
enum { SEL_UCB = 0, SEL_PUCT = 1, SEL_PROGRESSIVE_BIAS = 2, SEL_RAVE = 3 };
enum { GAME_GOMOKU = 0, GAME_GO = 1 };
// why the move judge (move_reason: k_open_games, k_illegal_moves) refuses a move (0: legal)
enum { AZ_OPEN_RANGE = 1, AZ_OPEN_OCCUPIED = 2, AZ_OPEN_FORBIDDEN = 3, AZ_OPEN_SUICIDE = 4, AZ_OPEN_KO = 5,
       AZ_OPEN_SUPERKO = 6, AZ_OPEN_ENDED = 7 };

struct Nodes {          // one arena: [G][ncap]
    int* N; float* W; int* VL; float* P; int* first; int16_t* act; int16_t* cnt; uint8_t* flag;
};

struct TreeDev {
    int G, bs, A, ncap;
    int game;                    // GAME_GOMOKU / GAME_GO
    int NA;                      // action space = policy length = max children (A, Go: A + 1 with pass = -1)
    int vl; float cpuct, fpu;
    int eval_kind;
    uint64_t tt_mask; int tt_slots;
    int ring;
    Nodes nd;                    // current arena
    int* atop;                   // [G] next free node in the current arena
    uint8_t* rboard;             // [G][A]   root board, 0 empty 1 black 2 white
    int* rhist;                  // [G][6]   last moves, [0] most recent, -1 none
    int* rplayer; int* rstones; int* rply; uint64_t* rhash; int* rfresh; int* rnode;
    int* active;                 // [G] game searching (not finished)
    // Go root state (GoState): ko point, consecutive passes, position_history_ (hashes of the
    // positions after every stone move, go_state.cpp:250-252; kept under superko only); rhash holds
    // the stones-only hash; rcap [G][2]: stones captured BY black / white (captured_stones_[1], [2])
    int* rko; int* rpass; uint64_t* rposh; int* rnposh; int* rcap; int hmax;
    int pad0 = 0;                // explicit padding (zero): tree_dev() compares TreeDev variants bytewise
    const uint64_t* zko;         // [A + 1] "ko_point" feature keys
    uint64_t zconst;             // "rules"[chinese] ^ "komi"[int(komi*2) & 15] (updateHash, with its & 15 aliasing)
    // GoState(bs, komi, chinese_rules, enforce_superko), fixed for the handle's life: every branch
    // on them is uniform over the grid
    float komi; int chinese; int superko;
    // GomokuState(bs, use_renju, use_omok): fixed per game sequence and uniform over the grid, read only by the
    // kernels' RULES instantiations (launched when tree_has_rules()) and by the per-move kernels.  The hash
    // keys "renju"[1] / "omok"[1] are in zconst (Gomoku: XORed into the start position's hash, root_empty)
    int renju, omok;
    int pad3 = 0;
    int* gresult;                // [G] GameResult of the root state
    uint64_t* gforb;             // [G][AZ_FORB_WORDS] Renju / Omok: forbidden-cell mask of the selected leaf (Black to
                                 // move), from the selection to the expansion; null without rules
    // Per-step scratch, from `gforb` above to `goleaf` below (bar rhdr and n_eval): one row per LEAF SLOT.  A
    // handle with leaf parallelism K (az_search_set_leaves, search_host.h) holds G * K rows, slot q = g * K + j
    // for descent j of game g's wave; at K = 1 -- and in the root steps of any handle -- the slot is the game,
    // which is how the [G] below read
    int* path; int* plen;        // [G][AZ_DMAX], [G]
    int* pact;                   // [G][AZ_DMAX] action of every path node (pact[0] unused)
    int* lstatus; float* lvalue; uint64_t* lhash; int* ttstore; uint64_t* ttref; int* tthslot;
    int4* pstat;                 // [G][AZ_DMAX] path nodes' statistics after k_select's virtual loss {N, VL, W bits, leaf flag}
    int4* rhdr;                  // [G] the root's header {first, cnt, flag} as the last simulation's k_select ended
    int* need_eval; int* eval_slot; int* eval_games; int* n_eval;
    int eval_identity;           // 1: the batch maps are the identity (eval_slot[g] == g): no slot load
    int pad1 = 0;
    uint8_t* leafrec;            // [G][AZ_REC_BYTES] leaf records (leaf_planes.h): the planes' inputs (NET)
    uint8_t* goleaf;             // Go: [G][AZ_GOLEAF_BYTES] the selected leaf's position (board, side to move,
                                 // ko, passes, stones hash, the path's position pushes) for its expansion
    uint64_t* tt_hash; int* tt_visits; float* tt_value; uint64_t* tt_ref;   // [G][slots]
    float* ring_buf; uint64_t* ring_cur;                                     // [G][ring], [G]
    long long* cnt;              // [G][AZ_NCNT]
    const uint64_t* zpiece;      // [2][A]
    const uint64_t* zplayer;     // [2]
    const int* fresh_order;      // [A] first-query legal order of a fresh state
    uint32_t* mt;                // [G][625] mt19937 state + index (RANDOM evaluator)
    int* err;                    // [1] sticky error bits
    const float* net_logits;     // [B][A] (NET) raw policy logits, by eval slot
    const float* net_value;      // [B]
    int log_game, log_cap; float* log_pol; float* log_val; float* log_planes; int* log_n;
    // Search options (az_search_opts, az_search_set_options; MCTSConfig): read only by the kernels' OPT instantiations,
    // which the host launches when tree_has_opts(); the default instantiations never look at them.
    // wid_tab[N], N in [0, wid_len): getProgressiveWideningCount(N, NA) (az_search_widening_table);
    // wid_complete: its last entry reached NA, so every count past it is "all children"
    int sel, max_depth, use_td; float td_lambda;
    int use_wid, wid_min, wid_len, wid_complete;
    const int* wid_tab;
    int stamp_game;              // diagnostic: this game's k_select / k_expand_backup write phase stamps (-1 off)
    int pad2 = 0;
};
// the options that need the OPT kernels (RAVE and a cap the path capacity reaches first are the default search)
inline bool tree_has_opts(const TreeDev& t) {
    return t.sel == SEL_UCB || t.sel == SEL_PROGRESSIVE_BIAS || t.max_depth < AZ_DMAX || t.use_td || t.use_wid;
}
// Renju / Omok in force: the kernels' RULES instantiations
inline bool tree_has_rules(const TreeDev& t) { return t.game == GAME_GOMOKU && (t.renju || t.omok); }
// no implicit padding: every byte of a TreeDev is a member (tree_dev() finds a variant with memcmp)
static_assert(offsetof(TreeDev, zko) == offsetof(TreeDev, pad0) + sizeof(int), "TreeDev hole after pad0");
static_assert(offsetof(TreeDev, gresult) == offsetof(TreeDev, pad3) + sizeof(int), "TreeDev hole after pad3");
static_assert(offsetof(TreeDev, komi) == offsetof(TreeDev, zconst) + sizeof(uint64_t), "TreeDev hole before komi");
static_assert(offsetof(TreeDev, pad3) == offsetof(TreeDev, komi) + 5 * sizeof(int), "TreeDev hole before pad3");
static_assert(offsetof(TreeDev, path) == offsetof(TreeDev, gresult) + 2 * sizeof(int*), "TreeDev hole after gforb");
static_assert(offsetof(TreeDev, leafrec) == offsetof(TreeDev, pad1) + sizeof(int), "TreeDev hole after pad1");
static_assert(sizeof(TreeDev) == offsetof(TreeDev, pad2) + sizeof(int), "TreeDev tail padding");
static_assert(offsetof(TreeDev, wid_tab) == offsetof(TreeDev, sel) + 8 * sizeof(int), "TreeDev hole before wid_tab");
static_assert(offsetof(TreeDev, sel) == offsetof(TreeDev, log_n) + sizeof(int*), "TreeDev hole before sel");
static_assert(offsetof(TreeDev, stamp_game) == offsetof(TreeDev, wid_tab) + sizeof(int*), "TreeDev hole after wid_tab");
static_assert(offsetof(TreeDev, tt_mask) == 10 * sizeof(int), "TreeDev hole before tt_mask");

// k_open_games' arguments: entry i of n starts slot games[i] and plays sequence seq_of[i] (null: i) -- the
// n_moves[seq] moves at moves[seq * stride] -- then up to rplies random plies of the Philox stream
// (key_lo, key_hi) with id rand_ids[i] (null: the seed id).
#define AZ_OPEN_REP 5         // ints of rep per entry: first bad ply (-1 none), reason, playing, GameResult, random plies
struct OpenDev {
    const int* games;        // [n] slots (a dry pass reads none: may be null)
    const int* seed_ids;     // [n] evaluator / noise stream ids, null: the slot index
    const int* moves; const int* n_moves; const int* seq_of;
    const int* rand_ids;
    int* picks;              // [n][rplies] the random plies played (null: not reported)
    uint64_t* hist;          // dry: [n][hstride] Go position history of the pass
    int* rep;                // [n][AZ_OPEN_REP]
    int n, stride, dry, rplies, hstride;
    uint32_t key_lo, key_hi, eval_seed;
};

// Replay buffer (az_replay_*, replay.hip): action-space training targets kept on the device.  A position is
// a record of `rec` bytes -- board [A] u8, Go: min(10, liberties) [A] u8, then at `moff` (4-aligned) eight
// int32 {side to move, ko point, last six moves}: the inputs of az_leaf_planes_v -- a counts row int32 [NA]
// (visit counts by action, Go's pass at A) and one int32 / fp32 per column below.  Staged rows: slot g's
// position p at g * max_plies + p; ring rows: [capacity].
enum { RP_HEAD = 0, RP_GAMES = 1, RP_DROPPED = 2, RP_SKIPPED = 3, RP_DONE = 4, RP_NCTR = 8 };
struct ReplayRows {
    uint8_t* rec; int* cnt; int* sum; float* q; int* gid; int* ply; int* player;
    float* z;                    // ring only
};
struct ReplayDev {
    int game, bs, A, NA, C;
    int rec, moff;               // record bytes (a multiple of 16), offset of its meta ints
    int capacity, max_plies;
    int pad = 0;
    ReplayRows st, ring;
    int* st_n;                   // [G] positions staged for the slot's game (counts past max_plies: dropped)
    int* slot_gid;               // [G] the game id each slot plays
    long long* ctr;              // [RP_NCTR]: ring head = positions ever committed, games, dropped, skipped, RP_DONE:
                                 // the blocks of the running k_replay_commit that have finished
};
// sym = k + 4 f: if f the columns are mirrored, (r, c) -> (r, n - c); then k quarter turns (r, c) -> (c, n - r)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline int replay_sym_cell(int bs, int sym, int cell) {
    const int n = bs - 1;
    int r = cell / bs, c = cell % bs;
    if (sym & 4) c = n - c;
    for (int k = sym & 3; k > 0; --k) { const int t = r; r = c; c = n - t; }
    return r * bs + c;
}
// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the replay buffer's
// sample plan (host) and the openings' random plies (k_open_games) draw from it
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// Training-example extraction (Dataset::extractExamples + augmentExample).
// Records are flattened: game g owns moves [move_off[g], move_off[g+1]); move m owns policy
// floats [pol_off[m], pol_off[m] + n_children[m]).  Pre-shuffle example e = m * K + s (s = 0
// original, 1..7 the reference's augmentation order); dst[e] is its slot (null: e).
constexpr int AZ_DS_THREADS = 256;   // k_dataset_extract: one 4-wave block per game record (8 waves: no faster, Go slower)
struct DatasetDev {
    int game, bs, A, NA, C, K, n_games;
    const int* move_off;         // [n_games + 1]
    const int* actions;          // [M]
    const long long* pol_off;    // [M]
    const int* n_children;       // [M]
    const float* policies;       // [sum n_children]
    const int* results;          // [n_games] GameResult
    const long long* dst;        // [M * K] or null
    float* states;               // [E][C][A]   (state[plane][row][col], NCHW)
    float* policy;               // [E][NA]     child-order targets, zero past plen
    int* plen;                   // [E]
    float* value;                // [E]
};
