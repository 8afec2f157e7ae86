// search_host.h -- the batched search handle and the steps of a move that the self-play driver
// (selfplay.hip) strings together.  Internal to libaz_hip.so.
#pragma once
#include <future>
#include <mutex>
#include <random>
#include <vector>

#include "engine_internal.h"
#include "tree.h"

struct az_net;
struct az_replay;

struct az_search {
    az_engine* e = nullptr;
    DevPool pool;   // every device buffer of the handle: the pointers below and in `t` point into it
    az_net* net = nullptr;
    // az_search_set_slot_nets: slot g is evaluated by nets[slot_net[g]] (n_nets = 0: the one net above).
    // Net k's batch is region k of the batch buffers -- rows [k * G, (k + 1) * G) of t.eval_games,
    // d_logits, d_value and d_batch, counter t.n_eval[k] -- which hold `regions` regions (1 at creation).
    az_net* nets[AZ_MAX_SLOT_NETS] = {};
    int n_nets = 0, regions = 1;
    int net_slots[AZ_MAX_SLOT_NETS] = {};   // slots assigned to each net: its forward's capacity
    uint8_t* d_slot_net = nullptr;          // [G]
    az_search_cfg c{};
    // Leaf parallelism (az_search_set_leaves): a simulation step makes `leaves` descents per game before it
    // completes any of them, and their leaves share one evaluator batch.  The per-step scratch of `t` (path, pact,
    // pstat, plen, lstatus, lvalue, lhash, ttstore, ttref, tthslot, need_eval, eval_slot, eval_games, leafrec,
    // goleaf) and the batch buffers (d_batch, d_logits, d_value, d_id) hold G * leaves rows, indexed by leaf
    // slot g * leaves + j; the root steps run on rows 0 .. G-1 as they do at leaves = 1.
    int leaves = 1;
    TreeDev t{};
    Nodes arena[2]{};
    int cur = 0;
    int* d_src_of = nullptr;
    float* d_batch = nullptr;       // gathered NHWC16 planes [G][A][16]
    int* d_id = nullptr;            // AZ_EVAL_NET: [G + 1] = 0, 1, ..., G-1, G (identity batch map + its count)
    // AZ_EVAL_CALLBACK: host evaluator, leaf moves / lengths and host staging
    az_eval_fn eval_fn = nullptr; void* eval_user = nullptr;
    int* d_lmoves = nullptr; int* d_llen = nullptr;
    std::vector<float> h_planes, h_nchw, h_pol, h_val;
    std::vector<int> h_games, h_lmoves, h_llen, h_full;
    std::vector<std::vector<int>> hist;    // per slot: the moves committed since the game started
    float* d_logits = nullptr; float* d_value = nullptr;
    float* d_noise = nullptr; uint8_t* d_mask = nullptr;
    int* d_actions = nullptr; float* d_values = nullptr; float* d_probs = nullptr; int* d_cact = nullptr; int* d_nch = nullptr;
    int* d_term = nullptr; int* d_res = nullptr; int* d_games = nullptr; int* d_seed_ids = nullptr;
    int* d_rexp = nullptr;          // k_apply: per game, its new root needs no root expansion
    // every playing game's root is expanded (or terminal): the root steps (MODE_ROOT_SEARCH /
    // MODE_ROOT_NOISE) would select nothing, evaluate nothing and expand nothing -- skipped
    bool roots_ready = false;
    bool used = false;              // a search step or a move has run: az_search_set_gomoku_rules comes before
    // scratch allocated once: one game's root-children readback, per-game prune thresholds / counts
    int* d_rc = nullptr; float* d_rcf = nullptr; int* d_thr = nullptr; long long* d_pruned = nullptr;
    float* d_temps = nullptr;
    // host mirrors
    std::vector<int> stones, active, fresh, ply, expanded;
    // az_search_profile
    bool prof = false;
    ProfClock pc;                 // sampled tree-kernel timing (az_search_profile)
    int64_t prof_steps = 0, prof_sampled = 0;
    ProfClock pcf;                // sampled timing of the fused k_expand_select (the production tree step)
    int64_t prof_fused = 0, prof_fused_launches = 0;
    std::vector<long long> prof_cnt0;
    std::vector<std::mt19937> rng;
    Pinned<float> h_noise; std::vector<uint8_t> h_mask;   // [G][NA] Dirichlet noise (page-locked: its H2D per move)
    // az_selfplay_step's MoveData records of the last step (az_selfplay_step_moves)
    // page-locked (Pinned): the per-move D2H of every game's visit distribution and child actions
    Pinned<float> sp_probs, sp_values;
    Pinned<int> sp_cact, sp_nch;
    std::vector<int> sp_slots;
    std::vector<az_move_rec> sp_moves;
    int sp_next_id = 0;             // one past the highest game id started on the handle (az_selfplay_step restarts)
    std::vector<int> slot_id;       // the game id each slot plays (search_new_games' seed id; default the slot index)
    // az_search_attach_replay: the self-play driver stages every root it moves from and commits finished games
    // (replay.hip); null: the driver launches nothing more than it does without the feature
    az_replay* replay = nullptr;
    // device-resident copies of the TreeDev variants the per-step kernels take (tree_dev()): those
    // kernels get one 8-byte pointer instead of the ~550-byte struct by value, on ~38k dispatches per
    // C3 move.  Slot i's host shadow (pinned, the source of its async upload) is h_tree.p[i].
    TreeDev* d_tree = nullptr;
    Pinned<TreeDev> h_tree;
    int n_tree = 0, next_tree = 0;
    az_search_opts opts{};          // the search options in force (az_search_set_options; creation: the defaults)
    // the progressive-widening table t.wid_tab was built for (apply_search_opts)
    bool wid_valid = false; float wid_base = 0.0f, wid_exponent = 0.0f; int wid_cap = 0;
    int64_t tree_evictions = 0;     // slot reuses (each a stream synchronisation): az_diag_tree_evictions
    // Dirichlet draws of the NEXT move, made on a host thread while the device searches this one
    // (prefetch_noise; Gomoku self-play): per game the child count they were drawn for (-1: none)
    // and the generator state after them, taken over only when the next noise call asks for exactly
    // that count; otherwise discarded (the game's own rng was never touched) and drawn inline.
    struct NoisePrefetch {
        std::future<void> job;
        bool on = false;
        float alpha = 0.0f;
        std::vector<int> nc;
        std::vector<std::mt19937> rng;
        std::vector<float> noise;
    } pf;
    // az_search_set_openings: the games the drivers start (az_selfplay_step restarts, az_selfplay_run, the
    // arena) begin with an opening of the book and / or random plies; off: they start from the empty board and
    // nothing more is launched.  The book lives on the host (records, mirrors) and in the handle's pool.
    struct Openings {
        bool on = false;
        std::vector<int> moves, n_moves;   // [n][stride], [n]
        int n = 0, stride = 0, rplies = 0;
        uint64_t seed = 0;
        int* d_moves = nullptr; int* d_nm = nullptr;
    } op;
    std::mutex mu;
};

// az_search_create; net_batch: the batch capacity `net` must have (az_search_create: n_games).
int search_create(az_engine* e, az_net* net, const az_search_cfg* c, int net_batch, az_search** out);
// One search of every playing game: root step, optional noise, the simulations, the error check.
int search_run(az_search* s);
// The root noise of the games in mask (null: all): draws on the host, k_noise on the device.
int search_noise(az_search* s, float alpha, float eps, const uint8_t* mask);
// (Re)start the listed slots with fresh games.  seed_ids (optional) give each game its own
// stream id for the evaluator / noise seeds (default: the slot index), so a game's record
// does not depend on which slot plays it.
int search_new_games(az_search* s, const int* games, int n, const int* seed_ids = nullptr);
// search_new_games with slot games[i] advanced by moves[i * stride .. i * stride + n_moves[i]), every move
// judged against the rules first: an illegal one is AZ_ERR_ARG and nothing has changed.
int search_open_games(az_search* s, const int* games, int n, const int* seed_ids, const int* moves, const int* n_moves,
                      int stride);
// The games a driver starts: search_new_games on a handle without openings; else entry i begins with opening
// open_ids[i] % n_openings (open_ids null: its stream id) and the random plies of stream open_ids[i].
// played (optional): per entry the opening plies its game was started with.
int search_start_games(az_search* s, const int* games, int n, const int* seed_ids, const int* open_ids,
                       std::vector<std::vector<int>>* played);
int search_set_openings(az_search* s, const az_openings_cfg* cfg);
int search_select(az_search* s, int training, const float* temps_host, float T, int* actions, float* values, float* probs,
                  int* cact, int* nch);
// makeMove + updateWithMove (device), then subtree compaction into the other arena.
int search_apply_dev(az_search* s, int* terminal, int* result);
// Start drawing the next move's noise for the games in `want` on a host thread (Gomoku: a root
// after one more stone has A - stones - 1 legal children).  The draws use copies of the games'
// generators; search_noise adopts a game's copy only when it asks for that very draw.
void prefetch_noise(az_search* s, float alpha, const std::vector<uint8_t>& want);
// the prefetch job done (every accessor of s->rng / s->pf calls this first)
void pf_wait(az_search* s);
// The replay buffer's hooks (replay.hip), for a handle with s->replay set; the caller holds s->mu.
// stage: after search_select and before search_apply_dev, one position per playing game that moves.
int replay_stage(az_search* s);
// commit the staged positions of the finished slots (ascending) with their GameResults (0: cut), in one launch
int replay_commit(az_search* s, const std::vector<int>& slots, const std::vector<int>& results);
// empty the staging of the listed slots (null: every slot) and refresh the slots' game ids
int replay_discard(az_search* s, const int* games, int n);
void replay_detach(az_search* s);
