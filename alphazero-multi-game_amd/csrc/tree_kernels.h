// tree_kernels.h -- launch interface of the search kernels (tree_kernels.hip): the launchers and
// the kernels that the host launches directly.  The one declaration of each, included by
// tree_kernels.hip and by every file that calls them.  The data layout is tree.h.
#pragma once
#include <hip/hip_runtime.h>

#include "tree.h"

// opt: tree_has_opts() of the TreeDev behind the device pointer -- the kernels' instantiation with the
// search options (selection strategy, depth cap, TD backup, progressive widening); false: the plain search
// rules: tree_has_rules() of it -- the instantiation that builds and honours the Renju / Omok forbidden-cell mask
void az_launch_select(const TreeDev* t, int NA, int G, int mode, bool opt, bool rules, hipStream_t st);
void az_launch_expand_select(const TreeDev* ts, const int* eval_slot, int eval_identity, int NA, int G, bool opt, bool rules,
                             hipStream_t st);
void az_launch_expand_backup(const TreeDev* t, int G, int mode, bool opt, bool rules, hipStream_t st);
// leaf parallelism (TreeDev scratch indexed by leaf slot g * K + j): one wave of k <= K descents per game, then its
// k completions in descent order; k_scan_leaves compacts the n = G * K leaf slots
void az_launch_wave_select(const TreeDev* t, int NA, int G, int K, int k, hipStream_t st);
void az_launch_wave_expand(const TreeDev* t, int G, int K, int k, hipStream_t st);
__global__ void k_scan(const TreeDev* __restrict__ tp);
__global__ void k_scan_leaves(const TreeDev* __restrict__ tp, int n);
__global__ void k_scan_nets(const TreeDev* __restrict__ tp, const uint8_t* __restrict__ slot_net, int n_nets);
__global__ void k_select_action(const TreeDev* __restrict__ tp, int training, float temperature, const float* temps, int* actions, float* values, float* probs,
                                int* child_actions, int* nchild);
__global__ void k_apply(TreeDev t, const int* actions, int* terminal, int* result, int* rexp);
// bad[g] = the AZ_OPEN_* reason the rules refuse actions[g] on game g's root position for (0: legal, a pass, no
// move, a game not playing); for a Go handle or tree_has_rules()
__global__ void k_illegal_moves(TreeDev t, const int* actions, int* bad);
__global__ void k_compact(TreeDev t, Nodes dst, int* src_of);
__global__ void k_leaf_moves(TreeDev t, int* moves, int* len);
__global__ void k_prune(TreeDev t, Nodes dst, int* src_of, int thr_all, const int* thr_g, long long* pruned);
__global__ void k_noise(TreeDev t, const float* noise, const uint8_t* mask, float eps);
__global__ void k_new_games(TreeDev t, const int* games, const int* seed_ids, int n, uint32_t eval_seed);
// openings (OpenDev, tree.h): fresh games in the listed slots, each advanced by a move sequence with every move
// judged against the rules, then by random plies drawn on the device; dry: nothing of the slots is written
__global__ void k_open_games(TreeDev t, OpenDev o);
__global__ void k_init_slots(TreeDev t, Nodes other);
__global__ void k_tt_clear(TreeDev t, const int* games, int n);
__global__ void k_root_nchild(TreeDev t, int* out);
__global__ void k_root_children(TreeDev t, int g, int* act, int* N, int* VL, float* W, float* P, int* n, int* rootinfo,
                                float* rootW);
// replay buffer (replay.hip).  stage: one wave per game slot -- the root position and its children's visit counts of
// every playing game whose actions[g] is a move, into the slot's staging rows.  commit: one block per finished slot
// slots[i] (ascending), GameResult results[i]: its staged rows into the ring after those of the slots before it.
// gather: one block per sample -- ring row idx[i] under symmetry sym[i] (null: 0) as planes, policy, z, q, game id, ply
// (the last four optional).  counts: the raw counts rows.
void az_launch_replay_stage(const TreeDev& t, const ReplayDev& r, const int* actions, const float* values, hipStream_t st);
void az_launch_replay_commit(const ReplayDev& r, const int* slots, const int* results, int n, hipStream_t st);
void az_launch_replay_gather(const ReplayDev& r, const long long* idx, const int* sym, int n, float* states, float* policy,
                             float* z, float* q, int* gid, int* ply, hipStream_t st);
void az_launch_replay_counts(const ReplayDev& r, const long long* idx, int n, int* counts, int* sum, hipStream_t st);
// training-example dataset (dataset.hip)
__global__ void k_dataset_extract(DatasetDev d, TreeDev t);
__global__ void k_dataset_gather(const float* states, const float* policy, const int* plen, const float* value, int row,
                                 int NA, const long long* idx, int n, float* ostates, float* opolicy, int* oplen,
                                 float* ovalue);
