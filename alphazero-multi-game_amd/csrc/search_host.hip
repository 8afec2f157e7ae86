// search_host.hip -- host side of the batched search behind the az_search_* entry points of
// include/az_engine.h: the handle, one simulation step (selection, network, expansion), the root
// noise with its prefetch, action selection and the committed move.
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <sched.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/az_engine.h"
#include "engine_internal.h"
#include "leaf_planes.h"
#include "net.h"
#include "net_host.h"
#include "search_host.h"
#include "tree_kernels.h"

// diagnostic: the game whose k_select / k_expand_backup write phase stamps (tools/tree_stamps.py),
// read at search creation; -1 off
static int g_tree_stamp_game = -1;
// diagnostic: a host synchronisation after every n simulation steps (0: none, the product default) --
// bounds the dispatches queued on the engine stream (rocprofv3 --pmc probe)
static int g_sync_every = 0;

namespace {

constexpr int AZ_TREE_SLOTS = 16;
// The device copy of TreeDev t (a variant with another arena or batch map is another slot).  A new
// variant is uploaded on the engine stream, so kernels queued before it still read their slot's old
// contents; a slot is reused only after a stream synchronisation (no queued kernel reads it then).
// Variants repeat (2 arenas x {search, identity batch}), so uploads happen at the first moves only.
const TreeDev* tree_dev(az_search* s, const TreeDev& t) {
    for (int i = 0; i < s->n_tree; ++i)
        if (std::memcmp(&s->h_tree.p[i], &t, sizeof(TreeDev)) == 0) return s->d_tree + i;
    int k;
    if (s->n_tree < AZ_TREE_SLOTS) {
        k = s->n_tree++;
    } else {
        if (hipStreamSynchronize(s->e->stream) != hipSuccess) return nullptr;
        ++s->tree_evictions;
        k = s->next_tree;
        s->next_tree = (k + 1) % AZ_TREE_SLOTS;
    }
    std::memcpy(&s->h_tree.p[k], &t, sizeof(TreeDev));
    if (hipMemcpyAsync(s->d_tree + k, &s->h_tree.p[k], sizeof(TreeDev), hipMemcpyHostToDevice, s->e->stream) != hipSuccess)
        return nullptr;
    return s->d_tree + k;
}
#define TREE_DEV(var, s, t)                                                       \
    const TreeDev* var = tree_dev(s, t);                                          \
    if (!var) return az_fail(AZ_ERR_HIP, "TreeDev upload failed")

int check_err(az_search* s) {
    int err = 0, ovf = 0;
    HIPCHK(hipMemcpyAsync(&err, s->t.err, 4, hipMemcpyDeviceToHost, s->e->stream));
    if (s->net && s->c.eval_kind == AZ_EVAL_NET) HIPCHK(hipMemcpyAsync(&ovf, s->net->ovf, 4, hipMemcpyDeviceToHost, s->e->stream));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    if (err) return az_fail(AZ_ERR_CAPACITY, "device capacity exceeded (flags 0x%x: 1 node pool, 2 path, 4 prior ring, 8 leaf batch, 32 widening table)", err);
    if (int r = check_ovf(s->net, ovf)) return r;
    // per-slot nets: every other net's range guard (nets[0] is s->net, read above)
    for (int k = 1; k < s->n_nets; ++k) {
        int o = 0;
        HIPCHK(hipMemcpyAsync(&o, s->nets[k]->ovf, 4, hipMemcpyDeviceToHost, s->e->stream));
        HIPCHK(hipStreamSynchronize(s->e->stream));
        if (int r = check_ovf(s->nets[k], o)) return r;
    }
    return 0;
}

// One batched step over all games: select -> (network) -> expand/backup.
// tree-kernel timing (az_search_profile): events around K1 and K3 of simulation steps
// (clock stamps, ProfClock: four per sampled step -- before / after the selection and the expansion)

// AZ_EVAL_CALLBACK: the leaves that need an evaluation go to the host evaluator as (game, moves
// from the root, NCHW feature planes); its policies / values come back for k_expand_backup.
int host_evaluate(az_search* s) {
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games, A = s->t.A, NA = s->t.NA, C = s->t.game == GAME_GO ? 8 : 11;
    TREE_DEV(dt, s, s->t);
    hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, dt);
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, s->t.n_eval, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n == 0) return 0;
    if (!s->eval_fn) return az_fail(AZ_ERR_STATE, "AZ_EVAL_CALLBACK search without az_search_set_evaluator");
    az_launch_rec_planes(s->t.leafrec, s->d_batch, s->t.eval_games, s->t.n_eval, s->t.game == GAME_GO, s->t.bs, G, st);
    hipLaunchKernelGGL(k_leaf_moves, dim3(G), dim3(64), 0, st, s->t, s->d_lmoves, s->d_llen);
    s->h_planes.resize((size_t)n * A * 16); s->h_games.resize(n); s->h_lmoves.resize((size_t)n * AZ_DMAX); s->h_llen.resize(n);
    HIPCHK(hipMemcpyAsync(s->h_planes.data(), s->d_batch, (size_t)n * A * 16 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s->h_games.data(), s->t.eval_games, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s->h_lmoves.data(), s->d_lmoves, (size_t)n * AZ_DMAX * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(s->h_llen.data(), s->d_llen, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    s->h_nchw.resize((size_t)n * C * A);
    for (int i = 0; i < n; ++i)
        for (int c = 0; c < C; ++c)
            for (int a = 0; a < A; ++a) s->h_nchw[((size_t)i * C + c) * A + a] = s->h_planes[((size_t)i * A + a) * 16 + c];
    s->h_pol.assign((size_t)n * NA, 0.0f);
    s->h_val.assign(n, 0.0f);
    // moves from the game's initial state: the slot's committed moves, then the path
    size_t mx = 1;
    for (int i = 0; i < n; ++i) mx = std::max(mx, s->hist[s->h_games[i]].size() + (size_t)s->h_llen[i]);
    s->h_full.assign((size_t)n * mx, 0);
    std::vector<int> len(n);
    for (int i = 0; i < n; ++i) {
        const std::vector<int>& h = s->hist[s->h_games[i]];
        int* dst = s->h_full.data() + (size_t)i * mx;
        std::copy(h.begin(), h.end(), dst);
        std::copy(s->h_lmoves.begin() + (size_t)i * AZ_DMAX, s->h_lmoves.begin() + (size_t)i * AZ_DMAX + s->h_llen[i],
                  dst + h.size());
        len[i] = (int)h.size() + s->h_llen[i];
    }
    if (s->eval_fn(s->eval_user, n, s->h_games.data(), len.data(), s->h_full.data(), (int)mx, s->h_nchw.data(), C,
                   s->h_pol.data(), s->h_val.data()) != 0)
        return az_fail(AZ_ERR_STATE, "host evaluator failed");
    HIPCHK(hipMemcpyAsync(s->d_logits, s->h_pol.data(), (size_t)n * NA * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_value, s->h_val.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    return 0;
}

// The network part of a step on a handle with per-slot nets (az_search_set_slot_nets): k_scan_nets
// partitions the leaves by net, then every net that has slots runs one forward on its own region of
// the batch buffers (rows [k * G, (k + 1) * G)), its capacity the number of slots assigned to it and its
// batch size the device counter n_eval[k] -- the host never reads the counts.  The expansion finds a
// slot's outputs through eval_slot as on a compacted single-net batch.
int eval_slot_nets(az_search* s, int mode, const TreeDev* dts, hipStream_t st) {
    const TreeDev& t = s->t;
    const int G = t.G;
    const bool go = t.game == GAME_GO;
    hipLaunchKernelGGL(k_scan_nets, dim3(1), dim3(1024), 0, st, dts, s->d_slot_net, s->n_nets);
    for (int k = 0; k < s->n_nets; ++k) {
        const int B = s->net_slots[k];
        if (B == 0) continue;
        az_net* n = s->nets[k];
        const int* games = t.eval_games + (size_t)k * G;
        const int* nb = t.n_eval + k;
        float* logits = s->d_logits + (size_t)k * G * t.NA;
        float* value = s->d_value + (size_t)k * G;
        const bool in_place = net_input_path(n) != NET_IN_GEMM;
        const LeafRecs lr{t.leafrec, games, go, G, 0};
        float* x = s->d_batch + (size_t)k * G * t.A * 16;
        if (!in_place) az_launch_rec_planes(t.leafrec, x, games, nb, lr.go, t.bs, B, st);
        const bool prof = n->prof;
        if (mode != MODE_SIM) n->prof = false;   // time only the simulation batches
        const int r = in_place ? net_forward(n, nullptr, B, nb, logits, value, st, &lr)
                               : net_forward(n, x, B, nb, logits, value, st);
        n->prof = prof;
        if (r) return r;
    }
    return 0;
}

// pre: this step's selection was already issued (fused into the previous step's expansion);
// fuse_next: issue this step's expansion fused with the next simulation step's selection.
int search_step(az_search* s, int mode, bool pre = false, bool fuse_next = false) {
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games;
    if (mode != MODE_SIM && s->roots_ready) return 0;   // every playing root expanded: a no-op step
    // a root step that fails part-way (TreeDev upload, the host evaluator, the net forward) leaves
    // the roots unexpanded: roots_ready is set only once the step is fully issued (below)
    if (mode != MODE_SIM) s->roots_ready = false;
    s->t.nd = s->arena[s->cur];
    const int64_t sidx = s->prof_steps;   // this simulation step's index while profiling
    const bool prof = s->prof && mode == MODE_SIM && s->prof_steps++ % prof_every() == 0 && s->pc.room(4);
    if (prof) s->pc.stamp(st);
    TREE_DEV(dts, s, s->t);
    const bool opt = tree_has_opts(s->t), rules = tree_has_rules(s->t);
    s->used = true;
    if (!pre) az_launch_select(dts, s->t.NA, s->t.G, mode, opt, rules, st);
    if (prof) s->pc.stamp(st);
    if (s->c.eval_kind == AZ_EVAL_CALLBACK) {
        if (int r = host_evaluate(s)) return r;
    }
    TreeDev tt = s->t;
    if (s->c.eval_kind == AZ_EVAL_NET && s->n_nets > 0) {
        if (int r = eval_slot_nets(s, mode, dts, st)) return r;
    } else
    if (s->c.eval_kind == AZ_EVAL_NET) {
        // The batch: in a simulation step with every game active, every game has a leaf and nearly
        // all of them need the network (C3: 800 evaluations per 800-sim move), so the batch is the
        // identity (slot = game; the few terminal / TT-hit leaves are computed and ignored: the
        // net's outputs are batch-position independent) and k_scan's compaction is skipped.
        // Otherwise (root steps, finished slots) k_scan compacts the leaves that need it.
        bool identity = mode == MODE_SIM && s->d_id != nullptr;
        for (int g = 0; identity && g < G; ++g) identity = s->active[g] != 0;
        if (identity) {
            tt.eval_slot = s->d_id; tt.eval_games = s->d_id; tt.n_eval = s->d_id + G; tt.eval_identity = 1;
        } else {
            hipLaunchKernelGGL(k_scan, dim3(1), dim3(1024), 0, st, dts);
        }
        // the net's input stage builds the leaves' planes from their records (record eval_games[b])
        // where it can; otherwise a dense fp32 plane batch is built first
        const bool in_place = net_input_path(s->net) != NET_IN_GEMM;
        const LeafRecs lr{tt.leafrec, tt.eval_games, tt.game == GAME_GO, G, identity ? 1 : 0};
        if (!in_place) az_launch_rec_planes(tt.leafrec, s->d_batch, tt.eval_games, tt.n_eval, lr.go, tt.bs, G, st);
        const bool prof = s->net->prof;
        if (mode != MODE_SIM) s->net->prof = false;   // time only the simulation batches
        int r = in_place ? net_forward(s->net, nullptr, G, tt.n_eval, s->d_logits, s->d_value, st, &lr)
                         : net_forward(s->net, s->d_batch, G, tt.n_eval, s->d_logits, s->d_value, st);
        s->net->prof = prof;
        if (r) return r;
    }
    if (prof) s->pc.stamp(st);
    if (fuse_next) {
        // the fused launch is timed on its own cadence, half-way between the split sampled steps
        const bool fs = s->prof && mode == MODE_SIM && sidx % prof_every() == prof_every() / 2 && s->pcf.room(2);
        if (s->prof && mode == MODE_SIM) ++s->prof_fused_launches;
        if (fs) s->pcf.stamp(st);
        az_launch_expand_select(dts, tt.eval_slot, tt.eval_identity, s->t.NA, G, opt, rules, st);
        if (fs) { s->pcf.stamp(st); ++s->prof_fused; }
    } else {
        TREE_DEV(dte, s, tt);
        az_launch_expand_backup(dte, G, mode, opt, rules, st);
    }
    if (prof) { s->pc.stamp(st); s->prof_sampled += 1; }
    HIPCHK(hipGetLastError());
    if (mode != MODE_SIM) s->roots_ready = true;         // after it every playing root is (expanded or terminal)
    return 0;
}

// One wave of a handle with leaves = K > 1: k <= K descents per game (k_wave_select), one evaluator batch over
// the G * K leaf slots, the k completions per game in descent order (k_wave_expand).  The batch is the identity
// when every game plays and the wave is full; the net runs on every leaf that may need it, and a forward whose
// completion then finds a TT hit or an expanded leaf is dropped (not an evaluation: `evals` counts completions).
int wave_step(az_search* s, int k) {
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games, K = s->leaves, Q = G * K;
    s->t.nd = s->arena[s->cur];
    TREE_DEV(dts, s, s->t);
    s->used = true;
    az_launch_wave_select(dts, s->t.NA, G, K, k, st);
    TreeDev tt = s->t;
    if (s->c.eval_kind == AZ_EVAL_NET) {
        bool identity = k == K && s->d_id != nullptr;
        for (int g = 0; identity && g < G; ++g) identity = s->active[g] != 0;
        if (identity) {
            tt.eval_slot = s->d_id; tt.eval_games = s->d_id; tt.n_eval = s->d_id + Q; tt.eval_identity = 1;
        } else {
            hipLaunchKernelGGL(k_scan_leaves, dim3(1), dim3(1024), 0, st, dts, Q);
        }
        const bool in_place = net_input_path(s->net) != NET_IN_GEMM;
        const LeafRecs lr{tt.leafrec, tt.eval_games, tt.game == GAME_GO, Q, identity ? 1 : 0};
        if (!in_place) az_launch_rec_planes(tt.leafrec, s->d_batch, tt.eval_games, tt.n_eval, lr.go, tt.bs, Q, st);
        const int r = in_place ? net_forward(s->net, nullptr, Q, tt.n_eval, s->d_logits, s->d_value, st, &lr)
                               : net_forward(s->net, s->d_batch, Q, tt.n_eval, s->d_logits, s->d_value, st);
        if (r) return r;
    }
    TREE_DEV(dte, s, tt);
    az_launch_wave_expand(dte, G, K, k, st);
    HIPCHK(hipGetLastError());
    return 0;
}

// n simulation steps.  Step i's expansion and step i+1's selection share one launch
// (k_expand_select) except around the profiled steps (their kernels are timed separately) and
// with the host evaluator (which runs between the two).
// leaves = K > 1: ceil(n / K) waves, the last one short when K does not divide n.
int search_sims(az_search* s, int n) {
    if (s->leaves > 1) {
        for (int done = 0, w = 0; done < n; ++w) {
            const int k = std::min(s->leaves, n - done);
            if (int r = wave_step(s, k)) return r;
            done += k;
            if (g_sync_every > 0 && (w + 1) % g_sync_every == 0) HIPCHK(hipStreamSynchronize(s->e->stream));
        }
        return 0;
    }
    const bool can_fuse = s->c.eval_kind != AZ_EVAL_CALLBACK;
    bool pre = false;
    for (int i = 0; i < n; ++i) {
        const bool sampled = s->prof && s->prof_steps % prof_every() == 0;
        const bool next_sampled = s->prof && (s->prof_steps + 1) % prof_every() == 0;
        const bool fuse = can_fuse && i + 1 < n && !sampled && !next_sampled;
        if (int r = search_step(s, MODE_SIM, pre, fuse)) return r;
        pre = fuse;
        if ((i + 1) % 100 == 0) STEP_TRACE("%d sims issued", i + 1);
        if (g_sync_every > 0 && (i + 1) % g_sync_every == 0) HIPCHK(hipStreamSynchronize(s->e->stream));
    }
    return 0;
}

// Host worker threads for per-game host work: the process's CPU share -- its affinity mask (a
// multi-GPU bench rank runs on its own slice of the host, bench.py), capped by OMP_NUM_THREADS
// where set (the GPU boxes, where hardware_concurrency reports the whole machine) and by 16.
int host_threads() {
    static const int n = [] {
        int h = (int)std::thread::hardware_concurrency();
        cpu_set_t cs;
        if (sched_getaffinity(0, sizeof(cs), &cs) == 0 && CPU_COUNT(&cs) > 0) h = std::min(h, (int)CPU_COUNT(&cs));
        if (const char* e = getenv("OMP_NUM_THREADS")) if (atoi(e) > 0) h = std::min(h, atoi(e));
        return std::max(1, std::min(16, h));
    }();
    return n;
}

// addDirichletNoise's draws for one game (parallel_mcts.cpp:1136-1156): nc gammas of a fresh
// libstdc++ gamma_distribution<float>(alpha) on the game's mt19937, floored and normalised
void draw_dirichlet(std::mt19937& rng, float alpha, int nc, float* nz) {
    std::gamma_distribution<float> gamma(alpha, 1.0f);
    float sum = 0.0f;
    for (int i = 0; i < nc; ++i) { nz[i] = std::max(1e-10f, gamma(rng)); sum += nz[i]; }
    if (sum <= 0.0f) { sum = 1.0f; for (int i = 0; i < nc; ++i) nz[i] = 1.0f / (float)nc; }
    for (int i = 0; i < nc; ++i) nz[i] /= sum;
}

// game g's generator changes outside the noise path (reseed, set, stochastic selectAction): its
// prefetched draws no longer follow from it
void pf_drop(az_search* s, int g) {
    pf_wait(s);
    if (s->pf.on && g >= 0 && g < (int)s->pf.nc.size()) s->pf.nc[g] = -1;
}

}  // namespace

// the prefetch job done (every accessor of s->rng / s->pf calls this first)
void pf_wait(az_search* s) {
    if (s->pf.job.valid()) s->pf.job.get();
}

// Start drawing the next move's noise for the games in `want` on a host thread (Gomoku: a root
// after one more stone has A - stones - 1 legal children).  The draws use copies of the games'
// generators; search_noise adopts a game's copy only when it asks for that very draw.
void prefetch_noise(az_search* s, float alpha, const std::vector<uint8_t>& want) {
    pf_wait(s);
    auto& P = s->pf;
    const int G = s->c.n_games, A = s->t.A, NA = s->t.NA;
    P.on = false;
    if (s->t.game != GAME_GOMOKU || tree_has_rules(s->t)) return;   // Renju / Omok: the child count is the device's to tell
    P.nc.assign(G, -1);
    P.rng.resize(G);
    P.noise.resize((size_t)G * NA);
    bool any = false;
    for (int g = 0; g < G; ++g)
        if (want[g] && s->active[g] && A - s->stones[g] - 1 > 0) { P.nc[g] = A - s->stones[g] - 1; any = true; }
    if (!any) return;
    P.on = true;
    P.alpha = alpha;
    P.job = std::async(std::launch::async, [s, alpha, G, NA] {
        pthread_setname_np(pthread_self(), "az-noise-pf");   // named in crash reports (az_diag_crash_report)
        auto& Q = s->pf;
        for (int g = 0; g < G; ++g) {
            if (Q.nc[g] < 0) continue;
            Q.rng[g] = s->rng[g];
            draw_dirichlet(Q.rng[g], alpha, Q.nc[g], Q.noise.data() + (size_t)g * NA);
        }
    });
}

int search_noise(az_search* s, float alpha, float eps, const uint8_t* mask) {
    const int G = s->c.n_games, A = s->t.A, NA = s->t.NA;
    if (int r = search_step(s, MODE_ROOT_NOISE)) return r;
    pf_wait(s);
    STEP_TRACE("noise: root step issued");
    std::vector<int> nroot;
    if (s->t.game == GAME_GO || tree_has_rules(s->t)) {   // |children| of each root (Go: legal moves incl. pass and superko;
                                                          // Renju / Omok: the empty cells less the forbidden ones)
        nroot.resize(G);
        s->t.nd = s->arena[s->cur];
        hipLaunchKernelGGL(k_root_nchild, dim3((G + 255) / 256), dim3(256), 0, s->e->stream, s->t, s->d_nch);
        HIPCHK(hipMemcpyAsync(nroot.data(), s->d_nch, G * 4, hipMemcpyDeviceToHost, s->e->stream));
        HIPCHK(hipStreamSynchronize(s->e->stream));
    }
    // addDirichletNoise draws (parallel_mcts.cpp:1136-1156): libstdc++ gamma on the host,
    // one fresh gamma_distribution per call on the game's mt19937.
    // Every game draws from its own mt19937, so the games split over host threads without changing
    // a single draw (a C2 move's 128 x 225 draws take ~6 ms on one core).
    auto& P = s->pf;
    const bool pfo = P.on && P.alpha == alpha;
    int inline_games = 0;
    for (int g = 0; g < G; ++g) {
        if (!s->active[g] || (mask && !mask[g])) continue;
        const int nc = !nroot.empty() ? nroot[g] : s->fresh[g] ? A : A - s->stones[g];
        inline_games += !(pfo && nc > 0 && P.nc[g] == nc);
    }
    auto draw = [&](int g0, int g1) {
        if (g0 > 0) pthread_setname_np(pthread_self(), "az-gamma");   // the workers (g0 = 0: the caller)
        for (int g = g0; g < g1; ++g) {
            s->h_mask[g] = 0;
            if (!s->active[g] || (mask && !mask[g])) continue;
            const int nc = !nroot.empty() ? nroot[g] : s->fresh[g] ? A : A - s->stones[g];
            if (nc <= 0) continue;
            float* nz = s->h_noise.data() + (size_t)g * NA;
            if (pfo && P.nc[g] == nc) {               // drawn ahead from a copy of this very generator state
                std::copy(P.noise.begin() + (size_t)g * NA, P.noise.begin() + (size_t)g * NA + nc, nz);
                s->rng[g] = P.rng[g];
            } else {
                draw_dirichlet(s->rng[g], alpha, nc, nz);
            }
            s->h_mask[g] = 1;
        }
    };
    // host threads only for the draws still to be made (none when the prefetch covered the move)
    const int nt = std::max(1, std::min({host_threads(), inline_games / 16}));
    if (nt == 1) {
        draw(0, G);
    } else {
        std::vector<std::thread> th;
        for (int t = 1; t < nt; ++t) th.emplace_back(draw, (int)((long)G * t / nt), (int)((long)G * (t + 1) / nt));
        draw(0, (int)((long)G / nt));
        for (auto& x : th) x.join();
    }
    P.on = false;                                       // consumed (or superseded): each prefetch serves one call
    STEP_TRACE("noise: gamma draws done (%d inline)", inline_games);
    bool any = false;
    for (int g = 0; g < G && !any; ++g) any = s->h_mask[g] != 0;
    if (!any) return 0;
    hipStream_t st = s->e->stream;
    HIPCHK(hipMemcpyAsync(s->d_noise, s->h_noise.data(), (size_t)G * NA * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(s->d_mask, s->h_mask.data(), G, hipMemcpyHostToDevice, st));
    s->t.nd = s->arena[s->cur];
    hipLaunchKernelGGL(k_noise, dim3(G), dim3(64), 0, st, s->t, s->d_noise, s->d_mask, eps);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int search_run(az_search* s) {
    STEP_TRACE("search_run: root step");
    if (int r = search_step(s, MODE_ROOT_SEARCH)) return r;
    if (s->c.use_dirichlet_each_search)
        if (int r = search_noise(s, s->c.dirichlet_alpha, s->c.dirichlet_eps, nullptr)) return r;
    STEP_TRACE("search_run: sims");
    if (int r = search_sims(s, s->c.num_simulations)) return r;
    STEP_TRACE("search_run: check_err");
    const int r = check_err(s);
    STEP_TRACE("search_run: done");
    return r;
}

namespace {
// The host mirrors of slot g after a game with stream id `id` has started in it with `plies` plies played
// (s->hist[g] is the caller's): as a fresh game and `plies` search_apply_dev leave them -- stones counts a
// Go pass too.
void slot_started(az_search* s, int g, int id, int plies, int active) {
    s->stones[g] = plies; s->active[g] = active; s->fresh[g] = plies == 0; s->ply[g] = plies;
    if (plies) s->used = true;                           // moves have been made (az_search_set_gomoku_rules comes before)
    s->roots_ready = false;                              // a fresh root: unexpanded
    s->slot_id[g] = id;
    s->sp_next_id = std::max(s->sp_next_id, id + 1);
    pf_drop(s, g);
    s->rng[g].seed(s->c.noise_seed + (uint32_t)(s->c.noise_seed_stride * id));
}
}  // namespace

// (Re)start the listed slots with fresh games.  seed_ids (optional) give each game its own
// stream id for the evaluator / noise seeds (default: the slot index), so a game's record
// does not depend on which slot plays it.
int search_new_games(az_search* s, const int* games, int n, const int* seed_ids) {
    if (n <= 0) return 0;
    hipStream_t st = s->e->stream;
    for (int i = 0; i < n; ++i)
        if (games[i] < 0 || games[i] >= s->c.n_games) return az_fail(AZ_ERR_ARG, "game index %d out of range", games[i]);
    HIPCHK(hipMemcpyAsync(s->d_games, games, n * 4, hipMemcpyHostToDevice, st));
    if (seed_ids) HIPCHK(hipMemcpyAsync(s->d_seed_ids, seed_ids, n * 4, hipMemcpyHostToDevice, st));
    s->t.nd = s->arena[s->cur];
    hipLaunchKernelGGL(k_new_games, dim3(n), dim3(64), 0, st, s->t, s->d_games, seed_ids ? s->d_seed_ids : nullptr, n,
                       s->c.eval_seed);
    hipLaunchKernelGGL(k_tt_clear, dim3(64, n), dim3(256), 0, st, s->t, s->d_games, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        s->hist[games[i]].clear();
        slot_started(s, games[i], seed_ids ? seed_ids[i] : games[i], 0, 1);
    }
    if (s->replay) return replay_discard(s, games, n);   // a new game in the slot: its staged positions go
    return 0;
}

namespace {
const char* open_reason(const az_search* s, int why) {
    switch (why) {
    case AZ_OPEN_RANGE: return "is out of range";
    case AZ_OPEN_OCCUPIED: return "is an occupied cell";
    case AZ_OPEN_FORBIDDEN: return s->t.renju ? "is forbidden to Black under the Renju rules" : "is forbidden to Black under the Omok rules";
    case AZ_OPEN_SUICIDE: return "is suicide";
    case AZ_OPEN_KO: return "retakes the ko";
    case AZ_OPEN_SUPERKO: return "repeats a position (superko)";
    case AZ_OPEN_ENDED: return "comes after the game has ended";
    }
    return "is illegal";
}
}  // namespace

namespace {
// One start through k_open_games: entry i starts slot games[i] with sequence seq_of[i] (null: i) of the
// sequences (moves / n_moves / stride on the host, d_moves / d_nm the same on the device), then up to rplies
// random plies of the Philox stream (seed, rand_ids[i] -- null: the seed id).
struct OpenJob {
    const int* games; const int* seed_ids; int n;
    const int* moves; const int* n_moves; int stride;
    const int* d_moves; const int* d_nm;
    const int* seq_of; const int* rand_ids;
    int rplies; uint64_t seed;
};

// validate: a dry pass judges every sequence first, so a refused call has changed nothing.
// played (optional): per entry the plies its game was started with (the sequence, then the random picks).
int open_games_run(az_search* s, const OpenJob& j, bool validate, std::vector<std::vector<int>>* played) {
    hipStream_t st = s->e->stream;
    const int n = j.n;
    const bool keeps_hist = s->t.game == GAME_GO && s->t.superko;
    int longest = 0;
    for (int i = 0; i < n; ++i) longest = std::max(longest, j.n_moves ? j.n_moves[j.seq_of ? j.seq_of[i] : i] : 0);
    DevPool tmp;   // freed on every return
    int *d_seq = nullptr, *d_rid = nullptr, *d_picks = nullptr, *d_rep = nullptr;
    uint64_t* d_hist = nullptr;
    if (j.seq_of) if (int r = tmp.alloc(&d_seq, (size_t)n)) return r;
    if (j.rand_ids) if (int r = tmp.alloc(&d_rid, (size_t)n)) return r;
    if (j.rplies > 0) if (int r = tmp.alloc(&d_picks, (size_t)n * j.rplies)) return r;
    if (int r = tmp.alloc(&d_rep, AZ_OPEN_REP * (size_t)n)) return r;
    if (validate && keeps_hist) if (int r = tmp.alloc(&d_hist, (size_t)n * longest)) return r;
    HIPCHK(hipMemcpyAsync(s->d_games, j.games, n * 4, hipMemcpyHostToDevice, st));
    if (j.seed_ids) HIPCHK(hipMemcpyAsync(s->d_seed_ids, j.seed_ids, n * 4, hipMemcpyHostToDevice, st));
    if (j.seq_of) HIPCHK(hipMemcpyAsync(d_seq, j.seq_of, n * 4, hipMemcpyHostToDevice, st));
    if (j.rand_ids) HIPCHK(hipMemcpyAsync(d_rid, j.rand_ids, n * 4, hipMemcpyHostToDevice, st));
    s->t.nd = s->arena[s->cur];
    OpenDev o{};
    o.games = s->d_games; o.seed_ids = j.seed_ids ? s->d_seed_ids : nullptr;
    o.moves = j.d_moves; o.n_moves = j.d_nm; o.seq_of = d_seq; o.rand_ids = d_rid;
    o.picks = d_picks; o.hist = d_hist; o.rep = d_rep;
    o.n = n; o.stride = j.stride; o.hstride = longest;
    o.key_lo = (uint32_t)j.seed; o.key_hi = (uint32_t)(j.seed >> 32); o.eval_seed = s->c.eval_seed;
    std::vector<int> rep(AZ_OPEN_REP * (size_t)n), picks((size_t)n * std::max(j.rplies, 0));
    if (validate) {
        o.dry = 1; o.rplies = 0;                         // a random ply is legal by construction
        hipLaunchKernelGGL(k_open_games, dim3(n), dim3(64), 0, st, s->t, o);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rep.data(), d_rep, rep.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i)
            if (rep[AZ_OPEN_REP * i] >= 0) {
                const int ply = rep[AZ_OPEN_REP * i], seq = j.seq_of ? j.seq_of[i] : i;
                return az_fail(AZ_ERR_ARG, "entry %d (slot %d): ply %d, action %d %s", i, j.games[i], ply,
                               j.moves[(size_t)seq * j.stride + ply], open_reason(s, rep[AZ_OPEN_REP * i + 1]));
            }
    }
    o.dry = 0; o.rplies = j.rplies;
    hipLaunchKernelGGL(k_open_games, dim3(n), dim3(64), 0, st, s->t, o);
    hipLaunchKernelGGL(k_tt_clear, dim3(64, n), dim3(256), 0, st, s->t, s->d_games, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rep.data(), d_rep, rep.size() * 4, hipMemcpyDeviceToHost, st));
    if (j.rplies > 0) HIPCHK(hipMemcpyAsync(picks.data(), d_picks, picks.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (played) played->assign(n, {});
    for (int i = 0; i < n; ++i) {
        const int g = j.games[i], seq = j.seq_of ? j.seq_of[i] : i;
        const int nm = j.n_moves ? j.n_moves[seq] : 0, nr = rep[AZ_OPEN_REP * i + 4];
        std::vector<int>& h = s->hist[g];
        h.clear();
        if (nm) h.assign(j.moves + (size_t)seq * j.stride, j.moves + (size_t)seq * j.stride + nm);
        h.insert(h.end(), picks.begin() + (size_t)i * j.rplies, picks.begin() + (size_t)i * j.rplies + nr);
        slot_started(s, g, j.seed_ids ? j.seed_ids[i] : g, nm + nr, rep[AZ_OPEN_REP * i + 2]);
        if (played) (*played)[i] = h;
    }
    if (s->replay) return replay_discard(s, j.games, n);   // a new game in the slot: its staged positions go
    return 0;
}
}  // namespace

// search_new_games with every listed slot advanced by its own move sequence (k_open_games): the handle as
// after search_new_games and one az_search_apply per move.
int search_open_games(az_search* s, const int* games, int n, const int* seed_ids, const int* moves, const int* n_moves,
                      int stride) {
    if (n <= 0) return 0;
    const int G = s->c.n_games;
    if (n > G) return az_fail(AZ_ERR_ARG, "%d slots listed, the handle has %d", n, G);
    if (stride < 0) return az_fail(AZ_ERR_ARG, "stride %d", stride);
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        if (games[i] < 0 || games[i] >= G) return az_fail(AZ_ERR_ARG, "entry %d: game index %d out of range", i, games[i]);
        if (n_moves[i] < 0 || n_moves[i] > stride)
            return az_fail(AZ_ERR_ARG, "entry %d (slot %d): %d moves, the stride is %d", i, games[i], n_moves[i], stride);
        longest = std::max(longest, n_moves[i]);
    }
    if (longest == 0) return search_new_games(s, games, n, seed_ids);
    if (s->t.game == GAME_GO && s->t.superko)
        for (int i = 0; i < n; ++i) {
            int placed = 0;
            for (int k = 0; k < n_moves[i]; ++k) placed += moves[(size_t)i * stride + k] >= 0;
            if (placed > s->t.hmax)
                return az_fail(AZ_ERR_CAPACITY, "entry %d (slot %d): %d stone moves, the position history holds %d", i, games[i],
                               placed, s->t.hmax);
        }
    DevPool tmp;   // freed on every return
    int *d_moves = nullptr, *d_nm = nullptr;
    if (int r = tmp.alloc(&d_moves, (size_t)n * stride)) return r;
    if (int r = tmp.alloc(&d_nm, (size_t)n)) return r;
    HIPCHK(hipMemcpyAsync(d_moves, moves, (size_t)n * stride * 4, hipMemcpyHostToDevice, s->e->stream));
    HIPCHK(hipMemcpyAsync(d_nm, n_moves, (size_t)n * 4, hipMemcpyHostToDevice, s->e->stream));
    const OpenJob j{games, seed_ids, n, moves, n_moves, stride, d_moves, d_nm, nullptr, nullptr, 0, 0};
    return open_games_run(s, j, true, nullptr);
}

// The games a driver starts: empty boards on a handle without openings (search_new_games, nothing more is
// launched), else game i begins with opening open_ids[i] % n_openings of the book (null: its stream id) and
// the random plies of stream open_ids[i] after it.  played (optional): per entry the opening plies.
int search_start_games(az_search* s, const int* games, int n, const int* seed_ids, const int* open_ids,
                       std::vector<std::vector<int>>* played) {
    if (played) played->assign(std::max(n, 0), {});
    if (!s->op.on) return search_new_games(s, games, n, seed_ids);
    if (n <= 0) return 0;
    for (int i = 0; i < n; ++i)
        if (games[i] < 0 || games[i] >= s->c.n_games) return az_fail(AZ_ERR_ARG, "game index %d out of range", games[i]);
    std::vector<int> seq(n), rid(n);
    for (int i = 0; i < n; ++i) {
        rid[i] = open_ids ? open_ids[i] : seed_ids ? seed_ids[i] : games[i];
        seq[i] = s->op.n > 0 ? (int)((unsigned)rid[i] % (unsigned)s->op.n) : 0;
    }
    const OpenJob j{games, seed_ids, n, s->op.moves.data(), s->op.n > 0 ? s->op.n_moves.data() : nullptr, s->op.stride,
                    s->op.d_moves, s->op.n > 0 ? s->op.d_nm : nullptr, seq.data(), rid.data(), s->op.rplies, s->op.seed};
    return open_games_run(s, j, false, played);            // the book was judged when it was set
}

// The openings of the games the drivers start (az_search_set_openings); cfg null or empty: none.
int search_set_openings(az_search* s, const az_openings_cfg* cfg) {
    const bool go = s->t.game == GAME_GO;
    if (!cfg || (cfg->n_openings == 0 && cfg->random_plies == 0)) {
        s->pool.release(s->op.d_moves); s->pool.release(s->op.d_nm);
        s->op = az_search::Openings{};
        return 0;
    }
    const int n = cfg->n_openings, stride = cfg->stride;
    if (n < 0 || cfg->random_plies < 0 || (n > 0 && (!cfg->moves || !cfg->n_moves || stride < 0)))
        return az_fail(AZ_ERR_ARG, "openings: %d openings, stride %d, %d random plies", n, stride, cfg->random_plies);
    int longest = 0;
    for (int i = 0; i < n; ++i) {
        if (cfg->n_moves[i] < 0 || cfg->n_moves[i] > stride)
            return az_fail(AZ_ERR_ARG, "opening %d: %d moves, the stride is %d", i, cfg->n_moves[i], stride);
        longest = std::max(longest, cfg->n_moves[i]);
    }
    if (go && s->t.superko && longest + cfg->random_plies > s->t.hmax)
        return az_fail(AZ_ERR_CAPACITY, "openings of %d + %d plies, the position history holds %d", longest, cfg->random_plies,
                       s->t.hmax);
    hipStream_t st = s->e->stream;
    DevPool fresh;   // the new book; adopted by the handle's pool once it is judged
    int *d_moves = nullptr, *d_nm = nullptr;
    if (n > 0) {
        if (int r = fresh.alloc(&d_moves, (size_t)n * stride)) return r;
        if (int r = fresh.alloc(&d_nm, (size_t)n)) return r;
        HIPCHK(hipMemcpyAsync(d_moves, cfg->moves, (size_t)n * stride * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_nm, cfg->n_moves, (size_t)n * 4, hipMemcpyHostToDevice, st));
        // every opening through the dry kernel: legal, and the game still playing after it
        DevPool tmp;
        int* d_rep = nullptr;
        uint64_t* d_hist = nullptr;
        if (int r = tmp.alloc(&d_rep, AZ_OPEN_REP * (size_t)n)) return r;
        if (go && s->t.superko) if (int r = tmp.alloc(&d_hist, (size_t)n * longest)) return r;
        OpenDev o{};
        o.moves = d_moves; o.n_moves = d_nm; o.hist = d_hist; o.rep = d_rep;
        o.n = n; o.stride = stride; o.hstride = longest; o.dry = 1;
        std::vector<int> rep(AZ_OPEN_REP * (size_t)n);
        hipLaunchKernelGGL(k_open_games, dim3(n), dim3(64), 0, st, s->t, o);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(rep.data(), d_rep, rep.size() * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i) {
            const int* r = rep.data() + AZ_OPEN_REP * i;
            if (r[0] >= 0)
                return az_fail(AZ_ERR_ARG, "opening %d: ply %d, action %d %s", i, r[0], cfg->moves[(size_t)i * stride + r[0]],
                               open_reason(s, r[1]));
            if (!r[2]) return az_fail(AZ_ERR_ARG, "opening %d ends the game (result %d)", i, r[3]);
        }
    }
    s->pool.release(s->op.d_moves); s->pool.release(s->op.d_nm);
    s->pool.adopt(fresh);
    s->op = az_search::Openings{};
    s->op.on = true; s->op.n = n; s->op.stride = stride; s->op.rplies = cfg->random_plies; s->op.seed = cfg->seed;
    if (n > 0) {
        s->op.moves.assign(cfg->moves, cfg->moves + (size_t)n * stride);
        s->op.n_moves.assign(cfg->n_moves, cfg->n_moves + n);
    }
    s->op.d_moves = d_moves; s->op.d_nm = d_nm;
    return 0;
}

int search_select(az_search* s, int training, const float* temps_host, float T, int* actions, float* values, float* probs,
                  int* cact, int* nch) {
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games, A = s->t.NA;     // child-order arrays are [G][NA]
    s->t.nd = s->arena[s->cur];
    if (temps_host) HIPCHK(hipMemcpyAsync(s->d_temps, temps_host, G * 4, hipMemcpyHostToDevice, st));
    TREE_DEV(dt, s, s->t);
    hipLaunchKernelGGL(k_select_action, dim3(G), dim3(64), 0, st, dt, training, T, temps_host ? s->d_temps : nullptr,
                       s->d_actions, s->d_values, s->d_probs, s->d_cact, s->d_nch);
    HIPCHK(hipGetLastError());
    if (actions) HIPCHK(hipMemcpyAsync(actions, s->d_actions, G * 4, hipMemcpyDeviceToHost, st));
    if (values) HIPCHK(hipMemcpyAsync(values, s->d_values, G * 4, hipMemcpyDeviceToHost, st));
    if (probs) HIPCHK(hipMemcpyAsync(probs, s->d_probs, (size_t)G * A * 4, hipMemcpyDeviceToHost, st));
    if (cact) HIPCHK(hipMemcpyAsync(cact, s->d_cact, (size_t)G * A * 4, hipMemcpyDeviceToHost, st));
    if (nch) HIPCHK(hipMemcpyAsync(nch, s->d_nch, G * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

// makeMove + updateWithMove (device), then subtree compaction into the other arena.
int search_apply_dev(az_search* s, int* terminal, int* result) {
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games;
    s->t.nd = s->arena[s->cur];
    std::vector<int> acts(G);
    s->used = true;
    HIPCHK(hipMemcpyAsync(acts.data(), s->d_actions, G * 4, hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_apply, dim3(G), dim3(64), 0, st, s->t, s->d_actions, s->d_term, s->d_res, s->d_rexp);
    hipLaunchKernelGGL(k_compact, dim3(G), dim3(256), 0, st, s->t, s->arena[s->cur ^ 1], s->d_src_of);
    HIPCHK(hipGetLastError());
    s->cur ^= 1;
    s->t.nd = s->arena[s->cur];
    std::vector<int> term(G), res(G);
    HIPCHK(hipMemcpyAsync(term.data(), s->d_term, G * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(res.data(), s->d_res, G * 4, hipMemcpyDeviceToHost, st));
    std::vector<int> rexp(G);
    HIPCHK(hipMemcpyAsync(rexp.data(), s->d_rexp, G * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    bool ready = true;
    for (int g = 0; g < G; ++g) {
        if (s->active[g] && acts[g] >= (s->t.game == GAME_GO ? -1 : 0)) {
            s->hist[g].push_back(acts[g]);
            s->stones[g] += 1; s->ply[g] += 1; s->fresh[g] = 0;
            if (term[g]) s->active[g] = 0;
        }
        ready = ready && rexp[g] != 0;
    }
    s->roots_ready = ready;
    if (terminal) std::copy(term.begin(), term.end(), terminal);
    if (result) std::copy(res.begin(), res.end(), result);
    return check_err(s);
}

static int search_release(az_search* s, int threshold, int64_t* pruned, const uint8_t* mask) {
    HIPCHK(hipSetDevice(s->e->device));
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games;
    long long* d_pr = s->d_pruned;
    int* d_thr = nullptr;
    if (mask) {   // games outside the mask keep every child (the whole tree is copied as it is)
        std::vector<int> thr(G);
        for (int g = 0; g < G; ++g) thr[g] = mask[g] ? threshold : 0;
        d_thr = s->d_thr;
        HIPCHK(hipMemcpy(d_thr, thr.data(), (size_t)G * 4, hipMemcpyHostToDevice));
    }
    s->t.nd = s->arena[s->cur];
    hipLaunchKernelGGL(k_prune, dim3(G), dim3(64), 0, st, s->t, s->arena[s->cur ^ 1], s->d_src_of, threshold, d_thr, d_pr);
    s->cur ^= 1;
    s->t.nd = s->arena[s->cur];
    std::vector<long long> pr(G);
    hipError_t e1 = hipGetLastError();
    hipError_t e2 = hipMemcpyAsync(pr.data(), d_pr, (size_t)G * 8, hipMemcpyDeviceToHost, st);
    hipError_t e3 = hipStreamSynchronize(st);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess)
        return az_fail(AZ_ERR_HIP, "az_search_release: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2 != hipSuccess ? e2 : e3));
    if (pruned) for (int g = 0; g < G; ++g) pruned[g] = pr[g];
    return check_err(s);
}

// Park every game outside `mask` (inactive on the host and the device) around fn, then give the
// parked games their flags back: the masked entry points run the search of some games of a handle
// that several host objects share (mcts::SearchGroup), leaving the others' trees untouched.
static int with_masked(az_search* s, const uint8_t* mask, const std::function<int()>& fn) {
    const int G = s->c.n_games;
    const std::vector<int> saved = s->active;
    std::vector<int> now(G);
    bool parked = false;
    for (int g = 0; g < G; ++g) {
        now[g] = saved[g] && mask[g];
        parked |= now[g] != saved[g];
    }
    // roots_ready speaks for the games playing when it was set: parked games may have unexpanded roots
    s->roots_ready = false;
    if (parked) {
        s->active = now;
        HIPCHK(hipStreamSynchronize(s->e->stream));   // no queued kernel may still read the old flags
        HIPCHK(hipMemcpy(s->t.active, now.data(), (size_t)G * 4, hipMemcpyHostToDevice));
    }
    const int r = fn();
    if (parked) {
        HIPCHK(hipStreamSynchronize(s->e->stream));
        std::vector<int> back(G);
        for (int g = 0; g < G; ++g) back[g] = mask[g] ? s->active[g] : saved[g];
        s->active = back;
        HIPCHK(hipMemcpy(s->t.active, back.data(), (size_t)G * 4, hipMemcpyHostToDevice));
        s->roots_ready = false;
    }
    return r;
}

extern "C" {

int az_diag_set_tree_stamps(int game) {
    g_tree_stamp_game = game;
    return 0;
}
int az_diag_set_sync_every(int n) { g_sync_every = n; return 0; }

int az_search_create(az_engine* e, az_net* net, const az_search_cfg* c, az_search** out) {
    return search_create(e, net, c, c ? c->n_games : 0, out);
}

}  // extern "C"

// The Go rules a configuration names: go_rules 0 is GoState's defaults, whatever the other fields hold
namespace {
struct GoRules { float komi; int chinese, superko; };
GoRules go_rules_of(const az_search_cfg& c) {
    if (!c.go_rules) return {7.5f, 1, 1};
    return {c.go_komi, c.go_chinese_rules != 0, c.go_superko != 0};
}
bool same_rules(const GoRules& a, const GoRules& b) { return a.komi == b.komi && a.chinese == b.chinese && a.superko == b.superko; }

// MCTSConfig's defaults (include/alphazero/mcts/parallel_mcts.h:47-58): what a new handle plays
const az_search_opts kDefaultSearchOpts = {AZ_SEL_PUCT, 1000, 0, 0.8f, 0, 10, 2.0f, 0.5f};
int check_widening(float base, float exponent) {
    if (!std::isfinite(base) || base <= 0.0f) return az_fail(AZ_ERR_ARG, "widening_base must be finite and > 0");
    if (!(exponent > 0.0f && exponent <= 1.0f)) return az_fail(AZ_ERR_ARG, "widening_exponent must lie in (0, 1]");
    return 0;
}
int check_search_opts(const az_search_opts& o) {
    if (o.selection < AZ_SEL_UCB || o.selection > AZ_SEL_RAVE)
        return az_fail(AZ_ERR_ARG, "selection %d: 0 UCB, 1 PUCT, 2 PROGRESSIVE_BIAS, 3 RAVE", o.selection);
    if (!std::isfinite(o.td_lambda)) return az_fail(AZ_ERR_ARG, "td_lambda must be finite");
    return check_widening(o.widening_base, o.widening_exponent);
}
// largest widening table (entries); az_diag_set_widening_cap lowers it for the capacity test
int g_widening_cap = 1 << 22;

// getProgressiveWideningCount(N, n_actions) (parallel_mcts.cpp:1299-1313) for N = 0, 1, ... up to the first
// N whose count reaches n_actions, at most cap entries: the reference's expression -- a float base times
// std::pow(int, float), i.e. the double pow of the host libm -- with the x86-64 conversion of a NaN or
// out-of-range double (INT_MIN) spelled out
void widening_table(float base, float exponent, int n_actions, int cap, std::vector<int>& tab) {
    tab.clear();
    for (int N = 0; (int)tab.size() < cap; ++N) {
        const double x = base * std::pow(N, exponent);
        const int raw = (x > -2147483649.0 && x < 2147483648.0) ? static_cast<int>(x) : INT_MIN;
        const int count = std::max(1, std::min(raw, n_actions));
        tab.push_back(count);
        if (count >= n_actions) break;
    }
}

// The options into the TreeDev with their widening table (a new device buffer; the old one is
// released after the stream has drained: no queued kernel reads it then)
int apply_search_opts(az_search* s, const az_search_opts& o) {
    TreeDev& t = s->t;
    const bool retab = o.use_widening && (!t.wid_tab || !s->wid_valid || o.widening_base != s->wid_base ||
                                          o.widening_exponent != s->wid_exponent || g_widening_cap != s->wid_cap);
    if (retab) {
        std::vector<int> tab;
        widening_table(o.widening_base, o.widening_exponent, t.NA, g_widening_cap, tab);
        int* d = nullptr;
        if (int r = s->pool.alloc(&d, tab.size())) return r;
        if (hipMemcpy(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
            hipStreamSynchronize(s->e->stream) != hipSuccess) {
            s->pool.release(d);
            return az_fail(AZ_ERR_HIP, "widening table upload failed");
        }
        s->pool.release(t.wid_tab);
        t.wid_tab = d; t.wid_len = (int)tab.size(); t.wid_complete = tab.back() >= t.NA;
        s->wid_valid = true; s->wid_base = o.widening_base; s->wid_exponent = o.widening_exponent; s->wid_cap = g_widening_cap;
    }
    t.sel = o.selection; t.max_depth = o.max_search_depth; t.use_td = o.use_td; t.td_lambda = o.td_lambda;
    t.use_wid = o.use_widening; t.wid_min = o.widening_min_visits;
    s->opts = o;
    return 0;
}
}  // namespace

// az_search_create with the batch capacity asked of `net` given apart from the number of games: the
// arena's handle (arena.hip) gives each of its two nets half of its slots at once.
int search_create(az_engine* e, az_net* net, const az_search_cfg* c, int net_batch, az_search** out) {
    if (!e || !c || !out) return az_fail(AZ_ERR_ARG, "null argument");
    const int bs = c->board_size, A = bs * bs, G = c->n_games;
    const bool go = c->game == AZ_GAME_GO;
    const int NA = go ? A + 1 : A;
    if (bs < 3 || A > AZ_MAXA || G < 1 || c->num_simulations < 0 || c->virtual_loss < 0 || c->tt_log2 < 4 ||
        c->tt_log2 > 24 || c->eval_kind < 0 || c->eval_kind > 4 || (c->game != AZ_GAME_GOMOKU && !go))
        return az_fail(AZ_ERR_ARG, "unsupported search configuration");
    if (go && bs != 9 && bs != 13 && bs != 19)
        return az_fail(AZ_ERR_ARG, "Go board %d: GoState supports 9, 13 and 19 (go_state.cpp:24-26)", bs);
    if (c->go_rules != 0 && c->go_rules != AZ_GO_RULES_SET) return az_fail(AZ_ERR_ARG, "go_rules %d: 0 or AZ_GO_RULES_SET", c->go_rules);
    const GoRules rules = go_rules_of(*c);
    if (!std::isfinite(rules.komi) || std::fabs(rules.komi) > 1024.0f)
        return az_fail(AZ_ERR_ARG, "go_komi must be finite with |komi| <= 1024");
    if (!go && !same_rules(rules, GoRules{7.5f, 1, 1}))
        return az_fail(AZ_ERR_ARG, "Go rules (komi / scoring / ko rule) on a Gomoku handle");
    if (c->eval_kind == AZ_EVAL_NET) {
        if (!net) return az_fail(AZ_ERR_ARG, "AZ_EVAL_NET needs a network");
        if (net->d.board_size != bs || net->d.action_size != NA || net->d.in_planes != (go ? 8 : 11))
            return az_fail(AZ_ERR_ARG, "network shape does not match the board");
        if (net->d.max_batch < net_batch) return az_fail(AZ_ERR_ARG, "network max_batch %d < n_games %d", net->d.max_batch, net_batch);
        if (!net->loaded) return az_fail(AZ_ERR_STATE, "network weights not loaded");
    }
    if (c->prior_ring > 0 && c->prior_ring < NA)
        return az_fail(AZ_ERR_ARG, "prior_ring %d is smaller than one policy (%d entries)", c->prior_ring, NA);
    std::lock_guard<std::mutex> lk(e->mu);
    HIPCHK(hipSetDevice(e->device));
    std::unique_ptr<az_search, void (*)(az_search*)> guard(new az_search(), az_search_destroy);   // every early return frees it
    az_search* s = guard.get();
    s->e = e; s->net = net; s->c = *c;
    const int ncap = c->node_capacity > 0 ? c->node_capacity : 3 * std::max(64, c->num_simulations) * NA + 8 * NA + 64;
    const int ring = c->prior_ring > 0 ? c->prior_ring : std::max(1 << 16, 12 * std::max(64, c->num_simulations) * NA);
    s->c.node_capacity = ncap; s->c.prior_ring = ring;
    TreeDev& t = s->t;
    t.G = G; t.bs = bs; t.A = A; t.ncap = ncap; t.game = go ? GAME_GO : GAME_GOMOKU; t.NA = NA;
    t.hmax = go ? 2048 : 0; t.vl = c->virtual_loss; t.cpuct = c->c_puct; t.fpu = c->fpu_reduction;
    t.eval_kind = c->eval_kind; t.tt_slots = 1 << c->tt_log2; t.tt_mask = (uint64_t)t.tt_slots - 1; t.ring = ring;
    t.log_game = -1; t.log_cap = 0;
    t.komi = rules.komi; t.chinese = rules.chinese; t.superko = rules.superko;
    t.stamp_game = g_tree_stamp_game;   // diagnostic phase stamps (az_diag_set_tree_stamps)
    const size_t NG = (size_t)G * ncap;
    int r = 0;
#define SA(p, n) do { if (!r) r = s->pool.alloc(&(p), (size_t)(n)); } while (0)
    for (int k = 0; k < 2; ++k) {
        Nodes& nd = s->arena[k];
        SA(nd.N, NG); SA(nd.W, NG); SA(nd.VL, NG); SA(nd.P, NG); SA(nd.first, NG); SA(nd.act, NG); SA(nd.cnt, NG);
        SA(nd.flag, NG);
    }
    SA(t.atop, G); SA(t.rboard, (size_t)G * A); SA(t.rhist, G * 6); SA(t.rplayer, G); SA(t.rstones, G); SA(t.rply, G);
    SA(t.rhash, G); SA(t.rfresh, G); SA(t.rnode, G); SA(t.active, G); SA(t.gresult, G);
    uint64_t *zko = nullptr, *zp = nullptr, *zpl = nullptr; int* fo = nullptr;   // the TreeDev's const tables, filled below
    if (go) { SA(t.rko, G); SA(t.rpass, G); SA(t.rposh, (size_t)G * t.hmax); SA(t.rnposh, G); SA(t.rcap, 2 * (size_t)G); SA(zko, A + 1); }
    SA(t.path, (size_t)G * AZ_DMAX); SA(t.pact, (size_t)G * AZ_DMAX); SA(t.pstat, (size_t)G * AZ_DMAX); SA(t.rhdr, G); SA(t.plen, G); SA(t.lstatus, G); SA(t.lvalue, G); SA(t.lhash, G); SA(t.ttstore, G);
    SA(t.ttref, G); SA(t.tthslot, G); SA(t.need_eval, G); SA(t.eval_slot, G); SA(t.eval_games, G); SA(t.n_eval, 1);
    SA(t.leafrec, (size_t)G * AZ_REC_BYTES);
    if (t.game == GAME_GO) SA(t.goleaf, (size_t)G * AZ_GOLEAF_BYTES);
    SA(t.tt_hash, (size_t)G * t.tt_slots); SA(t.tt_visits, (size_t)G * t.tt_slots); SA(t.tt_value, (size_t)G * t.tt_slots);
    SA(t.tt_ref, (size_t)G * t.tt_slots);
    SA(t.ring_buf, (size_t)G * ring); SA(t.ring_cur, G); SA(t.cnt, (size_t)G * AZ_NCNT);
    if (!r) r = hipMemset(t.cnt, 0, (size_t)G * AZ_NCNT * 8) == hipSuccess ? 0 : az_fail(AZ_ERR_HIP, "memset");
    SA(zp, 2 * A); SA(zpl, 2); SA(fo, A);
    if (c->eval_kind == AZ_EVAL_RANDOM) SA(t.mt, (size_t)G * 625);
    SA(t.err, 1);
    SA(s->d_src_of, NG);
    if (c->eval_kind == AZ_EVAL_NET || c->eval_kind == AZ_EVAL_CALLBACK) {
        SA(s->d_batch, (size_t)G * A * 16); SA(s->d_logits, (size_t)G * NA); SA(s->d_value, G);
    }
    if (c->eval_kind == AZ_EVAL_NET) SA(s->d_id, G + 1);
    if (c->eval_kind == AZ_EVAL_CALLBACK) { SA(s->d_lmoves, (size_t)G * AZ_DMAX); SA(s->d_llen, G); }
    SA(s->d_noise, (size_t)G * NA); SA(s->d_mask, G); SA(s->d_actions, G); SA(s->d_values, G); SA(s->d_probs, (size_t)G * NA);
    SA(s->d_cact, (size_t)G * NA); SA(s->d_nch, G); SA(s->d_term, G); SA(s->d_res, G); SA(s->d_rexp, G); SA(s->d_games, G); SA(s->d_seed_ids, G); SA(s->d_temps, G);
    SA(s->d_rc, 4 * (size_t)NA + 8); SA(s->d_rcf, 2 * (size_t)NA + 4); SA(s->d_thr, G); SA(s->d_pruned, G);
#undef SA
    if (r) return r;
    t.zpiece = zp; t.zplayer = zpl; t.fresh_order = fo; t.zko = zko;
    if (s->d_id) {
        std::vector<int> id(G + 1);
        for (int i = 0; i <= G; ++i) id[i] = i;
        HIPCHK(hipMemcpy(s->d_id, id.data(), (G + 1) * 4, hipMemcpyHostToDevice));
    }
    if (go) {
        // GoState Zobrist features (go_state.cpp:48-51; ZobristHash::addFeature, zobrist_hash.cpp:58-70):
        // mt19937_64 seeded with std::hash<std::string> of the feature name
        std::mt19937_64 rk(std::hash<std::string>{}("ko_point"));
        std::vector<uint64_t> ko(A + 1);
        for (auto& k : ko) k = rk();
        HIPCHK(hipMemcpy(zko, ko.data(), (A + 1) * 8, hipMemcpyHostToDevice));
        std::mt19937_64 rr(std::hash<std::string>{}("rules"));
        uint64_t zrules[2] = {rr(), rr()};
        std::mt19937_64 rm(std::hash<std::string>{}("komi"));
        uint64_t komi[16];
        for (auto& k : komi) k = rm();
        t.zconst = zrules[rules.chinese ? 1 : 0] ^ komi[((int)(rules.komi * 2)) & 0xF];   // updateHash (go_state.cpp:846-877)
    }
    t.net_logits = s->d_logits; t.net_value = s->d_value;
    // Zobrist keys: ZobristHash(bs, 2, 2, seed) (src/core/zobrist_hash.cpp:9-36)
    {
        std::mt19937_64 rng(c->zobrist_seed);
        std::vector<uint64_t> keys(2 * A + 2);
        for (auto& k : keys) k = rng();
        HIPCHK(hipMemcpy(zp, keys.data(), 2 * A * 8, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(zpl, keys.data() + 2 * A, 16, hipMemcpyHostToDevice));
    }
    // First-query legal order of a fresh GomokuState: libstdc++ unordered_set growth
    {
        std::unordered_set<int> set;
        for (int a = 0; a < A; ++a) set.insert(a);
        std::vector<int> order(set.begin(), set.end());
        HIPCHK(hipMemcpy(fo, order.data(), A * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(t.err, 0, 4));
    if (int r2 = apply_search_opts(s, kDefaultSearchOpts)) return r2;
    if (s->pool.alloc(&s->d_tree, AZ_TREE_SLOTS) || !s->h_tree.get(AZ_TREE_SLOTS)) return az_fail(AZ_ERR_OOM, "TreeDev slots");
    HIPCHK(hipDeviceSynchronize());   // the null-stream copies / memsets above, before the engine stream runs
    // every slot an idle game with a valid root until k_new_games starts it
    t.nd = s->arena[0];
    hipLaunchKernelGGL(k_init_slots, dim3((G + 255) / 256), dim3(256), 0, e->stream, t, s->arena[1]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(e->stream));
    s->stones.assign(G, 0); s->active.assign(G, 0); s->fresh.assign(G, 1); s->ply.assign(G, 0); s->expanded.assign(G, 0);
    s->rng.resize(G);
    s->hist.assign(G, {});
    s->slot_id.resize(G);
    for (int g = 0; g < G; ++g) s->slot_id[g] = g;
    if (!s->h_noise.get((size_t)G * NA)) return az_fail(AZ_ERR_OOM, "hipHostMalloc (noise)");
    std::fill(s->h_noise.p, s->h_noise.p + (size_t)G * NA, 0.0f);
    s->h_mask.assign(G, 0);
    *out = guard.release();
    return 0;
}

extern "C" {

void az_search_destroy(az_search* s) {
    if (!s) return;
    pf_wait(s);
    (void)hipSetDevice(s->e->device);
    {
        std::lock_guard<std::mutex> lk(s->mu);
        replay_detach(s);
    }
    delete s;   // its pool frees every device buffer
}

int az_search_new_games(az_search* s, const int* games, int n) {
    if (!s || (!games && n)) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_new_games(s, games, n);
}

int az_search_add_noise(az_search* s, float alpha, float eps) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_noise(s, alpha, eps, nullptr);
}

int az_search_add_noise_masked(az_search* s, float alpha, float eps, const uint8_t* mask) {
    if (!s || !mask) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_noise(s, alpha, eps, mask);
}

int az_search_run(az_search* s) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_run(s);
}

int az_search_select(az_search* s, int training, float temperature, int* actions, float* root_values, float* probs,
                     int* children_actions, int* n_children) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_select(s, training, nullptr, temperature, actions, root_values, probs, children_actions, n_children);
}

int az_search_simulate(az_search* s, int n) {
    if (!s || n < 0) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    if (int r = search_sims(s, n)) return r;
    return check_err(s);
}

int az_search_release(az_search* s, int threshold, int64_t* pruned) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    return search_release(s, threshold, pruned, nullptr);
}

int az_search_release_masked(az_search* s, int threshold, int64_t* pruned, const uint8_t* mask) {
    if (!s || !mask) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    return search_release(s, threshold, pruned, mask);
}

int az_search_run_masked(az_search* s, const uint8_t* mask) {
    if (!s || !mask) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return with_masked(s, mask, [&] { return search_run(s); });
}

int az_search_simulate_masked(az_search* s, int n, const uint8_t* mask) {
    if (!s || !mask || n < 0) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return with_masked(s, mask, [&] {
        if (int r = search_sims(s, n)) return r;
        return check_err(s);
    });
}

int az_search_new_games_ids(az_search* s, const int* games, const int* seed_ids, int n) {
    if (!s || (!games && n) || (!seed_ids && n)) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_new_games(s, games, n, seed_ids);
}

int az_search_new_games_moves(az_search* s, const int* games, const int* seed_ids, int n, const int* moves,
                              const int* n_moves, int stride) {
    if (!s || (!games && n > 0) || (!n_moves && n > 0)) return az_fail(AZ_ERR_ARG, "null argument");
    if (!moves && n > 0 && stride > 0) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_open_games(s, games, n, seed_ids, moves, n_moves, stride);
}

int az_search_set_openings(az_search* s, const az_openings_cfg* cfg) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    return search_set_openings(s, cfg);
}

int az_search_openings(az_search* s, int* n_openings, int* random_plies, uint64_t* seed) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    if (n_openings) *n_openings = s->op.n;
    if (random_plies) *random_plies = s->op.rplies;
    if (seed) *seed = s->op.seed;
    return 0;
}

int az_search_select_action(az_search* s, int game, int training, float temperature, int batch_inference,
                            const int* legal, int n_legal, int* action) {
    if (!s || !action || game < 0 || game >= s->c.n_games || n_legal < 0 || (n_legal > 0 && !legal))
        return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    const int G = s->c.n_games, NA = s->t.NA;
    std::vector<int> acts(G), cact((size_t)G * NA), nch(G);
    std::vector<float> vals(G), probs((size_t)G * NA);
    const bool stoch = training && temperature > 0.0f;
    if (int r = search_select(s, training ? 1 : 0, nullptr, temperature, acts.data(), vals.data(), probs.data(), cact.data(),
                              nch.data()))
        return r;
    pf_drop(s, game);                                // this draw moves the game's generator
    std::mt19937& rng = s->rng[game];
    const int nc = nch[game];
    if (nc == 0) {                                   // no children: a legal move (parallel_mcts.cpp:994-1010)
        if (n_legal == 0) { *action = -1; return 0; }
        if (batch_inference) { *action = legal[0]; return 0; }
        std::uniform_int_distribution<size_t> dist(0, (size_t)n_legal - 1);
        *action = legal[dist(rng)];
        return 0;
    }
    const int* ca = cact.data() + (size_t)game * NA;
    if (batch_inference) { *action = acts[game]; return 0; }   // k_select_action: the deterministic rules
    if (stoch) {                                     // sample the visit distribution (:1013-1027)
        const float* pd = probs.data() + (size_t)game * NA;
        std::discrete_distribution<int> dist(pd, pd + nc);
        *action = ca[dist(rng)];
        return 0;
    }
    // evaluation or T = 0: the most visited children, one at random when tied (:1028-1046)
    std::vector<int> N(NA), act(NA), VL(NA);
    std::vector<float> W(NA), P(NA);
    int n = 0;
    s->t.nd = s->arena[s->cur];
    int* d_tmp = s->d_rc;
    float* d_f = s->d_rcf;
    hipStream_t st = s->e->stream;
    hipLaunchKernelGGL(k_root_children, dim3(1), dim3(64), 0, st, s->t, game, d_tmp, d_tmp + NA, d_tmp + 2 * NA, d_f,
                       d_f + NA, d_tmp + 3 * NA, d_tmp + 3 * NA + 1, d_f + 2 * NA);
    hipError_t e1 = hipMemcpyAsync(act.data(), d_tmp, NA * 4, hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipMemcpyAsync(N.data(), d_tmp + NA, NA * 4, hipMemcpyDeviceToHost, st);
    hipError_t e3 = hipMemcpyAsync(&n, d_tmp + 3 * NA, 4, hipMemcpyDeviceToHost, st);
    hipError_t e4 = hipStreamSynchronize(st);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess)
        return az_fail(AZ_ERR_HIP, "az_search_sample_action: root children readback failed");
    int mx = 0;
    for (int i = 0; i < n; ++i) mx = std::max(mx, N[i]);
    std::vector<int> best;
    for (int i = 0; i < n; ++i) if (N[i] == mx) best.push_back(act[i]);
    if (best.empty()) { *action = -1; return 0; }
    if (best.size() == 1) { *action = best[0]; return 0; }
    std::uniform_int_distribution<size_t> dist(0, best.size() - 1);
    *action = best[dist(rng)];
    return 0;
}

int az_search_apply(az_search* s, const int* actions, int* terminal, int* result) {
    if (!s || !actions) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    const int G = s->c.n_games, A = s->t.A;
    for (int g = 0; g < G; ++g)
        if (actions[g] >= A || (s->t.game == GAME_GO && actions[g] < AZ_ACTION_NONE))
            return az_fail(AZ_ERR_ARG, "action %d out of range for game %d", actions[g], g);
    HIPCHK(hipMemcpyAsync(s->d_actions, actions, G * 4, hipMemcpyHostToDevice, s->e->stream));
    if (s->t.game == GAME_GO || tree_has_rules(s->t)) {
        // GoState::makeMove / GomokuState::make_move throw on a move that is not legal: refused before anything
        // moves.  (Plain Gomoku has only the occupied cell to refuse and is not judged here: no launch, no wait.)
        std::vector<int> bad(G);
        hipLaunchKernelGGL(k_illegal_moves, dim3(G), dim3(64), 0, s->e->stream, s->t, s->d_actions, s->d_nch);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(bad.data(), s->d_nch, G * 4, hipMemcpyDeviceToHost, s->e->stream));
        HIPCHK(hipStreamSynchronize(s->e->stream));
        for (int g = 0; g < G; ++g)
            if (bad[g]) return az_fail(AZ_ERR_ARG, "action %d of game %d %s", actions[g], g, open_reason(s, bad[g]));
    }
    return search_apply_dev(s, terminal, result);
}

int az_search_root_children(az_search* s, int game, int* actions, int* N, int* VL, float* W, float* P, int* n_children) {
    if (!s || game < 0 || game >= s->c.n_games || !n_children) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    hipStream_t st = s->e->stream;
    const int A = s->t.NA;
    int *da, *dN, *dVL, *dn, *dri; float *dW, *dP, *drw;
    DevPool tmp;   // freed on every return
    int r = 0;
#define TA(p, n) do { if (!r) r = tmp.alloc(&(p), (size_t)(n)); } while (0)
    TA(da, A); TA(dN, A); TA(dVL, A); TA(dn, 1); TA(dri, 2); TA(dW, A); TA(dP, A); TA(drw, 1);
#undef TA
    if (r) return r;
    s->t.nd = s->arena[s->cur];
    hipLaunchKernelGGL(k_root_children, dim3(1), dim3(256), 0, st, s->t, game, da, dN, dVL, dW, dP, dn, dri, drw);
    int n = 0;
    HIPCHK(hipMemcpyAsync(&n, dn, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (actions) HIPCHK(hipMemcpy(actions, da, n * 4, hipMemcpyDeviceToHost));
    if (N) HIPCHK(hipMemcpy(N, dN, n * 4, hipMemcpyDeviceToHost));
    if (VL) HIPCHK(hipMemcpy(VL, dVL, n * 4, hipMemcpyDeviceToHost));
    if (W) HIPCHK(hipMemcpy(W, dW, n * 4, hipMemcpyDeviceToHost));
    if (P) HIPCHK(hipMemcpy(P, dP, n * 4, hipMemcpyDeviceToHost));
    *n_children = n;
    return 0;
}

int az_search_set_evaluator(az_search* s, az_eval_fn fn, void* user) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    if (s->c.eval_kind != AZ_EVAL_CALLBACK) return az_fail(AZ_ERR_STATE, "the handle was not created with AZ_EVAL_CALLBACK");
    std::lock_guard<std::mutex> lk(s->mu);
    s->eval_fn = fn; s->eval_user = user;
    return 0;
}

// A new device net for a handle created with AZ_EVAL_NET, the tree kept (ParallelMCTS::
// setNeuralNetwork only swaps nn_, parallel_mcts.cpp:1190-1207): same engine, board, planes and
// action space, a batch capacity covering the handle's games, weights loaded.
int az_search_set_net(az_search* s, az_net* net) {
    if (!s || !net) return az_fail(AZ_ERR_ARG, "null argument");
    if (s->c.eval_kind != AZ_EVAL_NET) return az_fail(AZ_ERR_STATE, "the handle was not created with AZ_EVAL_NET");
    if (net->e != s->e) return az_fail(AZ_ERR_ARG, "the network lives on another engine");
    const int bs = s->c.board_size, NA = s->t.NA;
    const bool go = s->c.game == AZ_GAME_GO;
    if (net->d.board_size != bs || net->d.action_size != NA || net->d.in_planes != (go ? 8 : 11))
        return az_fail(AZ_ERR_ARG, "network shape does not match the board");
    if (net->d.max_batch < s->c.n_games) return az_fail(AZ_ERR_ARG, "network max_batch < n_games");
    if (!net->loaded) return az_fail(AZ_ERR_STATE, "network weights not loaded");
    std::lock_guard<std::mutex> lk(s->mu);
    if (net->d.max_batch < s->c.n_games * s->leaves)
        return az_fail(AZ_ERR_ARG, "network max_batch %d < n_games %d x leaves %d", net->d.max_batch, s->c.n_games, s->leaves);
    s->net = net;
    s->n_nets = 0;   // back to one net for every slot (the region buffers stay: region 0 is the batch)
    return 0;
}

// Per-slot nets: slot g is evaluated by nets[slot_net[g]] from the next step on; trees, transposition
// tables and generators kept.  Every argument is checked before the handle changes.
int az_search_set_slot_nets(az_search* s, az_net* const* nets, int n_nets, const uint8_t* slot_net) {
    if (!s || !nets || !slot_net) return az_fail(AZ_ERR_ARG, "null argument");
    if (s->c.eval_kind != AZ_EVAL_NET) return az_fail(AZ_ERR_STATE, "the handle was not created with AZ_EVAL_NET");
    if (n_nets < 1 || n_nets > AZ_MAX_SLOT_NETS) return az_fail(AZ_ERR_ARG, "n_nets %d outside 1..%d", n_nets, AZ_MAX_SLOT_NETS);
    static_assert(AZ_MAX_SLOT_NETS == AZ_SCAN_NETS, "k_scan_nets partitions by AZ_MAX_SLOT_NETS nets");
    const int G = s->c.n_games, bs = s->c.board_size, A = s->t.A, NA = s->t.NA;
    const bool go = s->c.game == AZ_GAME_GO;
    int count[AZ_MAX_SLOT_NETS] = {};
    for (int g = 0; g < G; ++g) {
        if (slot_net[g] >= n_nets) return az_fail(AZ_ERR_ARG, "slot %d: net index %d >= n_nets %d", g, slot_net[g], n_nets);
        ++count[slot_net[g]];
    }
    for (int k = 0; k < n_nets; ++k) {
        const az_net* net = nets[k];
        if (!net) return az_fail(AZ_ERR_ARG, "net %d is null", k);
        if (net->e != s->e) return az_fail(AZ_ERR_ARG, "net %d lives on another engine", k);
        if (net->d.board_size != bs || net->d.action_size != NA || net->d.in_planes != (go ? 8 : 11))
            return az_fail(AZ_ERR_ARG, "net %d: shape does not match the board", k);
        if (net->d.max_batch < count[k])
            return az_fail(AZ_ERR_ARG, "net %d: max_batch %d < its %d slots", k, net->d.max_batch, count[k]);
        if (!net->loaded) return az_fail(AZ_ERR_STATE, "net %d: weights not loaded", k);
    }
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->leaves > 1) return az_fail(AZ_ERR_ARG, "per-slot nets on a handle with leaves = %d (leaf parallelism takes one net)", s->leaves);
    HIPCHK(hipSetDevice(s->e->device));
    hipStream_t st = s->e->stream;
    int* games = nullptr; int* n_eval = nullptr; float* logits = nullptr; float* value = nullptr; float* batch = nullptr;
    uint8_t* sn = nullptr;
    const bool grow = n_nets > s->regions;
    DevPool fresh;   // the new buffers, the handle's only once everything succeeded
    int r = 0;
    if (grow) {
        const size_t R = (size_t)n_nets;
        if (!r) r = fresh.alloc(&games, R * G);
        if (!r) r = fresh.alloc(&n_eval, R);
        if (!r) r = fresh.alloc(&logits, R * G * NA);
        if (!r) r = fresh.alloc(&value, R * G);
        if (!r) r = fresh.alloc(&batch, R * G * A * 16);
    }
    if (!r) r = fresh.alloc(&sn, (size_t)G);   // a fresh assignment buffer: a failed upload leaves the old one whole
    hipError_t he = hipStreamSynchronize(st);   // no queued kernel reads the old buffers or the old assignment
    if (!r && he != hipSuccess) r = az_fail(AZ_ERR_HIP, "az_search_set_slot_nets: %s", hipGetErrorString(he));
    if (!r && grow && (hipMemset(games, 0, (size_t)n_nets * G * 4) != hipSuccess || hipMemset(n_eval, 0, (size_t)n_nets * 4) != hipSuccess))
        r = az_fail(AZ_ERR_HIP, "az_search_set_slot_nets: memset");
    if (!r && hipMemcpy(sn, slot_net, (size_t)G, hipMemcpyHostToDevice) != hipSuccess)
        r = az_fail(AZ_ERR_HIP, "az_search_set_slot_nets: slot_net upload");
    if (r) return r;   // the handle as it was
    if (grow) {
        for (void* p : {(void*)s->t.eval_games, (void*)s->t.n_eval, (void*)s->d_logits, (void*)s->d_value, (void*)s->d_batch})
            s->pool.release(p);
        s->t.eval_games = games; s->t.n_eval = n_eval;
        s->d_logits = logits; s->d_value = value; s->d_batch = batch;
        s->t.net_logits = logits; s->t.net_value = value;
        s->regions = n_nets;
    }
    s->pool.release(s->d_slot_net);
    s->pool.adopt(fresh);
    s->d_slot_net = sn;
    for (int k = 0; k < AZ_MAX_SLOT_NETS; ++k) {
        s->nets[k] = k < n_nets ? nets[k] : nullptr;
        s->net_slots[k] = k < n_nets ? count[k] : 0;
    }
    s->n_nets = n_nets;
    s->net = nets[0];
    return 0;
}

// Empty every game's transposition table (a new TranspositionTable object: ParallelMCTS::
// setTranspositionTable, parallel_mcts.cpp:1209-1222); trees and counters kept.
int az_search_clear_tt(az_search* s) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    const int G = s->c.n_games;
    std::vector<int> g(G);
    for (int i = 0; i < G; ++i) g[i] = i;
    hipStream_t st = s->e->stream;
    HIPCHK(hipMemcpyAsync(s->d_games, g.data(), (size_t)G * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tt_clear, dim3(64, G), dim3(256), 0, st, s->t, s->d_games, G);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

int az_search_set_params(az_search* s, const az_search_cfg* c) {
    if (!s || !c) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    const az_search_cfg& o = s->c;
    if (c->n_games != o.n_games || c->board_size != o.board_size || c->eval_kind != o.eval_kind ||
        c->eval_seed != o.eval_seed || c->zobrist_seed != o.zobrist_seed || c->tt_log2 != o.tt_log2 ||
        c->game != o.game || (c->node_capacity > 0 && c->node_capacity != o.node_capacity) ||
        (c->prior_ring > 0 && c->prior_ring != o.prior_ring) || c->num_simulations < 0 || c->virtual_loss < 0)
        return az_fail(AZ_ERR_ARG, "az_search_set_params: shape / evaluator / table changes need a new handle");
    if ((c->go_rules != 0 && c->go_rules != AZ_GO_RULES_SET) || !same_rules(go_rules_of(*c), go_rules_of(o)))
        return az_fail(AZ_ERR_ARG, "az_search_set_params: the Go rules are fixed for a handle's life");
    // the node pool and prior ring were sized for the creation's simulations per search
    const int NA = s->t.NA;
    if (3 * std::max(64, c->num_simulations) * NA + 8 * NA + 64 > o.node_capacity ||
        12 * std::max(64, c->num_simulations) * NA > o.prior_ring)
        return az_fail(AZ_ERR_CAPACITY, "az_search_set_params: %d simulations exceed the node pool sized at creation",
                       c->num_simulations);
    s->c.num_simulations = c->num_simulations;
    s->c.c_puct = c->c_puct; s->c.fpu_reduction = c->fpu_reduction; s->c.virtual_loss = c->virtual_loss;
    s->c.use_dirichlet_each_search = c->use_dirichlet_each_search;
    s->c.dirichlet_alpha = c->dirichlet_alpha; s->c.dirichlet_eps = c->dirichlet_eps;
    s->c.noise_seed = c->noise_seed; s->c.noise_seed_stride = c->noise_seed_stride;
    s->t.cpuct = c->c_puct; s->t.fpu = c->fpu_reduction; s->t.vl = c->virtual_loss;
    return 0;
}

int az_search_set_options(az_search* s, const az_search_opts* opts) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    az_search_opts o = opts ? *opts : kDefaultSearchOpts;
    o.use_td = o.use_td != 0; o.use_widening = o.use_widening != 0;
    if (int r = check_search_opts(o)) return r;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    if (s->leaves > 1) {
        TreeDev probe = s->t;
        probe.sel = o.selection; probe.max_depth = o.max_search_depth; probe.use_td = o.use_td; probe.use_wid = o.use_widening;
        if (tree_has_opts(probe))
            return az_fail(AZ_ERR_ARG, "non-default search options on a handle with leaves = %d (set leaves = 1 first)", s->leaves);
    }
    return apply_search_opts(s, o);
}

// Leaf parallelism: K descents per game and simulation step, one evaluator batch of up to n_games x K leaves.
// Between searches; trees, tables, counters and generators are kept.  The per-step scratch and the batch buffers
// are replaced by ones of n_games x K rows from the handle's pool; every check and allocation comes before the
// handle changes.
int az_search_set_leaves(az_search* s, int leaves) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    if (leaves < 1 || leaves > AZ_MAX_LEAVES) return az_fail(AZ_ERR_ARG, "leaves %d outside 1..%d", leaves, AZ_MAX_LEAVES);
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    TreeDev& t = s->t;
    const int G = s->c.n_games, K = leaves, A = t.A, NA = t.NA;
    if (K > 1) {
        if (s->c.eval_kind == AZ_EVAL_CALLBACK)
            return az_fail(AZ_ERR_ARG, "leaves %d with AZ_EVAL_CALLBACK: the host evaluator takes leaves = 1", K);
        if (tree_has_opts(t)) return az_fail(AZ_ERR_ARG, "leaves %d with non-default search options (az_search_set_options)", K);
        if (tree_has_rules(t)) return az_fail(AZ_ERR_ARG, "leaves %d with the %s rules", K, t.renju ? "Renju" : "Omok");
        if (s->n_nets > 0) return az_fail(AZ_ERR_ARG, "leaves %d with per-slot nets (%d nets)", K, s->n_nets);
    }
    if (s->c.eval_kind == AZ_EVAL_NET && s->net && s->net->d.max_batch < G * K)
        return az_fail(AZ_ERR_ARG, "network max_batch %d < n_games %d x leaves %d = %d", s->net->d.max_batch, G, K, G * K);
    if (K == s->leaves) return 0;
    const size_t Q = (size_t)G * K, R = (size_t)std::max(1, s->regions) * Q;
    const bool net = s->c.eval_kind == AZ_EVAL_NET, cb = s->c.eval_kind == AZ_EVAL_CALLBACK;
    DevPool fresh;   // the new buffers, the handle's only once everything succeeded
    int* path = nullptr; int* pact = nullptr; int4* pstat = nullptr; int* plen = nullptr; int* lstatus = nullptr;
    float* lvalue = nullptr; uint64_t* lhash = nullptr; int* ttstore = nullptr; uint64_t* ttref = nullptr; int* tthslot = nullptr;
    int* need_eval = nullptr; int* eval_slot = nullptr; int* eval_games = nullptr; uint8_t* leafrec = nullptr; uint8_t* goleaf = nullptr;
    float* batch = nullptr; float* logits = nullptr; float* value = nullptr; int* id = nullptr;
    int r = 0;
#define FA(p, n) do { if (!r) r = fresh.alloc(&(p), (size_t)(n)); } while (0)
    FA(path, Q * AZ_DMAX); FA(pact, Q * AZ_DMAX); FA(pstat, Q * AZ_DMAX); FA(plen, Q); FA(lstatus, Q); FA(lvalue, Q); FA(lhash, Q);
    FA(ttstore, Q); FA(ttref, Q); FA(tthslot, Q); FA(need_eval, Q); FA(eval_slot, Q); FA(eval_games, R);
    FA(leafrec, Q * AZ_REC_BYTES);
    if (t.game == GAME_GO) FA(goleaf, Q * AZ_GOLEAF_BYTES);
    if (net || cb) { FA(batch, R * A * 16); FA(logits, R * NA); FA(value, R); }
    if (net) FA(id, Q + 1);
#undef FA
    if (r) return r;
    hipError_t he = hipStreamSynchronize(s->e->stream);   // no queued kernel reads the old buffers
    if (he == hipSuccess) he = hipMemset(lstatus, 0, Q * 4);
    if (he == hipSuccess) he = hipMemset(need_eval, 0, Q * 4);
    if (he == hipSuccess) he = hipMemset(eval_games, 0, R * 4);
    if (he == hipSuccess) he = hipMemset(leafrec, 0, Q * AZ_REC_BYTES);
    if (he == hipSuccess && id) {
        std::vector<int> h(Q + 1);
        for (size_t i = 0; i <= Q; ++i) h[i] = (int)i;
        he = hipMemcpy(id, h.data(), (Q + 1) * 4, hipMemcpyHostToDevice);
    }
    if (he == hipSuccess) he = hipDeviceSynchronize();
    if (he != hipSuccess) return az_fail(AZ_ERR_HIP, "az_search_set_leaves: %s", hipGetErrorString(he));
    for (void* p : {(void*)t.path, (void*)t.pact, (void*)t.pstat, (void*)t.plen, (void*)t.lstatus, (void*)t.lvalue, (void*)t.lhash,
                    (void*)t.ttstore, (void*)t.ttref, (void*)t.tthslot, (void*)t.need_eval, (void*)t.eval_slot, (void*)t.eval_games,
                    (void*)t.leafrec, (void*)t.goleaf})
        s->pool.release(p);
    if (net || cb) for (void* p : {(void*)s->d_batch, (void*)s->d_logits, (void*)s->d_value}) s->pool.release(p);
    if (net) s->pool.release(s->d_id);
    s->pool.adopt(fresh);
    t.path = path; t.pact = pact; t.pstat = pstat; t.plen = plen; t.lstatus = lstatus; t.lvalue = lvalue; t.lhash = lhash;
    t.ttstore = ttstore; t.ttref = ttref; t.tthslot = tthslot; t.need_eval = need_eval; t.eval_slot = eval_slot;
    t.eval_games = eval_games; t.leafrec = leafrec; t.goleaf = goleaf;
    if (net || cb) { s->d_batch = batch; s->d_logits = logits; s->d_value = value; t.net_logits = logits; t.net_value = value; }
    if (net) s->d_id = id;
    s->leaves = K;
    return 0;
}

int az_search_leaves(az_search* s, int* leaves) {
    if (!s || !leaves) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    *leaves = s->leaves;
    return 0;
}

int az_search_options(az_search* s, az_search_opts* out) {
    if (!s || !out) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    *out = s->opts;
    return 0;
}

int az_search_widening_table(float base, float exponent, int n_actions, int* out, int cap, int* len) {
    if (!len || cap < 0 || (cap > 0 && !out)) return az_fail(AZ_ERR_ARG, "null argument");
    if (n_actions < 1 || n_actions > AZ_MAXNA) return az_fail(AZ_ERR_ARG, "n_actions %d outside 1..%d", n_actions, AZ_MAXNA);
    if (int r = check_widening(base, exponent)) return r;
    std::vector<int> tab;
    widening_table(base, exponent, n_actions, g_widening_cap, tab);
    *len = (int)tab.size();
    std::copy(tab.begin(), tab.begin() + std::min<size_t>(tab.size(), (size_t)cap), out);
    return 0;
}

// Diagnostic (tests): the largest widening table from now on, 1 .. 2^22 entries; returns the limit it replaced.
int az_diag_set_widening_cap(int entries) {
    const int old = g_widening_cap;
    g_widening_cap = std::max(1, std::min(entries, 1 << 22));
    return old;
}

int az_search_set_gomoku_rules(az_search* s, const az_gomoku_rules* r) {
    if (!s || !r) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    if (s->t.game != GAME_GOMOKU) return az_fail(AZ_ERR_ARG, "Gomoku rules (Renju / Omok) on a Go handle");
    // its legal order follows libstdc++'s rehash sequence of a position-dependent insertion list
    if (r->pro_long_opening) return az_fail(AZ_ERR_ARG, "the pro-long opening is not supported");
    if (s->used) return az_fail(AZ_ERR_STATE, "az_search_set_gomoku_rules: the handle has searched or moved; the rules are set before");
    const int renju = r->renju != 0, omok = r->omok != 0;
    if ((renju || omok) && s->leaves > 1)
        return az_fail(AZ_ERR_ARG, "Renju / Omok on a handle with leaves = %d (set leaves = 1 first)", s->leaves);
    if ((renju || omok) && !s->t.gforb) {
        uint64_t* m = nullptr;
        if (int e = s->pool.alloc(&m, (size_t)s->c.n_games * AZ_FORB_WORDS)) return e;
        if (hipMemset(m, 0, (size_t)s->c.n_games * AZ_FORB_WORDS * 8) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            s->pool.release(m);
            return az_fail(AZ_ERR_HIP, "az_search_set_gomoku_rules: memset");
        }
        s->t.gforb = m;
    }
    // GomokuState's Zobrist features (gomoku_state.cpp:62-64, 640-649): value 1 of "renju" / "omok" is the second
    // draw of mt19937_64(std::hash<std::string>(name)) (ZobristHash::addFeature)
    uint64_t z = 0;
    for (int k = 0; k < 2; ++k) {
        std::mt19937_64 rf(std::hash<std::string>{}(k == 0 ? "renju" : "omok"));
        rf();
        const uint64_t on = rf();
        if (k == 0 ? renju : omok) z ^= on;
    }
    s->t.renju = renju; s->t.omok = omok; s->t.zconst = z;
    // slots already started (az_search_new_games before the rules): their fresh roots take the rules' hash
    std::vector<int> started;
    for (int g = 0; g < s->c.n_games; ++g) if (s->active[g]) started.push_back(g);
    if (!started.empty()) {
        std::vector<uint64_t> h(s->c.n_games);
        HIPCHK(hipMemcpy(h.data(), s->t.rhash, h.size() * 8, hipMemcpyDeviceToHost));
        uint64_t zpl0 = 0;
        HIPCHK(hipMemcpy(&zpl0, s->t.zplayer, 8, hipMemcpyDeviceToHost));
        for (int g : started) h[g] = zpl0 ^ z;
        HIPCHK(hipMemcpy(s->t.rhash, h.data(), h.size() * 8, hipMemcpyHostToDevice));
    }
    return 0;
}

int az_search_gomoku_rules(az_search* s, az_gomoku_rules* out) {
    if (!s || !out) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    out->renju = s->t.renju; out->omok = s->t.omok; out->pro_long_opening = 0;
    return 0;
}

int az_search_go_rules(az_search* s, float* komi, int* chinese_rules, int* superko) {
    if (!s || !komi || !chinese_rules || !superko) return az_fail(AZ_ERR_ARG, "null argument");
    const GoRules r = go_rules_of(s->c);
    *komi = r.komi; *chinese_rules = r.chinese; *superko = r.superko;
    return 0;
}

int az_search_seed(az_search* s, int game, uint32_t seed) {
    if (!s || game < 0 || game >= s->c.n_games) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    pf_drop(s, game);
    s->rng[game].seed(seed);
    return 0;
}

// std::mt19937's state through its stream operators (libstdc++: the 624 state words, then the
// position), as 625 uint32
int az_search_get_rng(az_search* s, int game, uint32_t* state) {
    if (!s || !state || game < 0 || game >= s->c.n_games) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    pf_wait(s);
    std::ostringstream os;
    os << s->rng[game];
    std::istringstream is(os.str());
    for (int i = 0; i < AZ_RNG_STATE_WORDS; ++i)
        if (!(is >> state[i])) return az_fail(AZ_ERR_ARG, "rng state: unexpected serialisation");
    return 0;
}

int az_search_set_rng(az_search* s, int game, const uint32_t* state) {
    if (!s || !state || game < 0 || game >= s->c.n_games) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    std::ostringstream os;
    for (int i = 0; i < AZ_RNG_STATE_WORDS; ++i) os << state[i] << (i + 1 < AZ_RNG_STATE_WORDS ? " " : "");
    std::istringstream is(os.str());
    std::mt19937 r;
    if (!(is >> r) || state[AZ_RNG_STATE_WORDS - 1] > 624) return az_fail(AZ_ERR_ARG, "rng state: not an mt19937 state");
    pf_drop(s, game);
    s->rng[game] = r;
    return 0;
}

int az_search_root_flags(az_search* s, int game, int* flags) {
    if (!s || !flags || game < 0 || game >= s->c.n_games) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));   // its queued kernels first: the reads below are null-stream copies
    int root = 0;
    uint8_t f = 0;
    HIPCHK(hipMemcpy(&root, s->t.rnode + game, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&f, s->arena[s->cur].flag + (size_t)game * s->t.ncap + root, 1, hipMemcpyDeviceToHost));
    *flags = f;
    return 0;
}

int az_search_root_node(az_search* s, int game, int* N, int* VL, float* W) {
    if (!s || game < 0 || game >= s->c.n_games) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));   // its queued kernels first: the reads below are null-stream copies
    int root = 0;
    HIPCHK(hipMemcpy(&root, s->t.rnode + game, 4, hipMemcpyDeviceToHost));
    const size_t off = (size_t)game * s->t.ncap + root;
    const Nodes& nd = s->arena[s->cur];
    if (N) HIPCHK(hipMemcpy(N, nd.N + off, 4, hipMemcpyDeviceToHost));
    if (VL) HIPCHK(hipMemcpy(VL, nd.VL + off, 4, hipMemcpyDeviceToHost));
    if (W) HIPCHK(hipMemcpy(W, nd.W + off, 4, hipMemcpyDeviceToHost));
    return 0;
}

int az_search_counters(az_search* s, int game, int64_t* out5) {
    if (!s || game < 0 || game >= s->c.n_games || !out5) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));   // its queued kernels first: the reads below are null-stream copies
    long long c[AZ_NCNT];
    HIPCHK(hipMemcpy(c, s->t.cnt + (size_t)game * AZ_NCNT, sizeof c, hipMemcpyDeviceToHost));
    for (int i = 0; i < 5; ++i) out5[i] = c[i];
    return 0;
}

int az_search_enable_eval_log(az_search* s, int game, int capacity) {
    if (!s || game < 0 || game >= s->c.n_games || capacity < 1) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    TreeDev& t = s->t;
    const int npl = t.game == GAME_GO ? 8 : 11;
    // the new log in a pool of its own: a failure below leaves the old log whole and readable
    DevPool fresh;
    float *pol = nullptr, *val = nullptr, *planes = nullptr; int* cnt = nullptr;
    if (int r = fresh.alloc(&pol, (size_t)capacity * t.NA)) return r;
    if (int r = fresh.alloc(&val, capacity)) return r;
    if (int r = fresh.alloc(&planes, (size_t)capacity * npl * t.A)) return r;
    if (int r = fresh.alloc(&cnt, 1)) return r;
    HIPCHK(hipMemset(cnt, 0, 4));
    for (void* p : {(void*)t.log_pol, (void*)t.log_val, (void*)t.log_planes, (void*)t.log_n}) s->pool.release(p);
    s->pool.adopt(fresh);
    t.log_pol = pol; t.log_val = val; t.log_planes = planes; t.log_n = cnt;
    t.log_game = game; t.log_cap = capacity;
    return 0;
}

int az_search_read_eval_log(az_search* s, float* policy, float* value, float* planes, int* count) {
    if (!s || !count) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));   // its queued kernels first: the reads below are null-stream copies
    TreeDev& t = s->t;
    if (!t.log_pol) { *count = 0; return 0; }
    int n = 0;
    HIPCHK(hipMemcpy(&n, t.log_n, 4, hipMemcpyDeviceToHost));
    if (policy) HIPCHK(hipMemcpy(policy, t.log_pol, (size_t)n * t.NA * 4, hipMemcpyDeviceToHost));
    if (value) HIPCHK(hipMemcpy(value, t.log_val, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (planes) HIPCHK(hipMemcpy(planes, t.log_planes, (size_t)n * (t.game == GAME_GO ? 8 : 11) * t.A * 4,
                                 hipMemcpyDeviceToHost));
    *count = n;
    return 0;
}

// diagnostic: TreeDev slot evictions so far (bench.py reports it: a steady-state step should have none)
int64_t az_diag_tree_evictions(az_search* s) { return s ? s->tree_evictions : -1; }

int az_search_profile(az_search* s, int enable) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    s->prof = enable != 0;
    for (ProfClock* pc : {&s->pc, &s->pcf})
        if (s->prof)
            if (int r = pc->enable(s->pool)) return r;
    s->pc.used = 0; s->pcf.used = 0;
    s->prof_steps = 0; s->prof_sampled = 0; s->prof_fused = 0; s->prof_fused_launches = 0;
    s->prof_cnt0.assign((size_t)s->c.n_games * AZ_NCNT, 0);
    HIPCHK(hipMemcpy(s->prof_cnt0.data(), s->t.cnt, s->prof_cnt0.size() * 8, hipMemcpyDeviceToHost));
    return 0;
}

int az_search_profile_read(az_search* s, double* select_ms, double* expand_ms, int64_t* sim_steps,
                           int64_t* select_bytes, int64_t* expand_bytes) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    double sel = 0.0, exp = 0.0;
    const std::vector<double> t = s->pc.read_ms();
    for (size_t i = 0; i + 3 < t.size(); i += 4) {
        sel += t[i + 1] - t[i];
        exp += t[i + 3] - t[i + 2];
    }
    std::vector<long long> c((size_t)s->c.n_games * AZ_NCNT);
    HIPCHK(hipMemcpy(c.data(), s->t.cnt, c.size() * 8, hipMemcpyDeviceToHost));
    long long bs = 0, be = 0;
    for (int g = 0; g < s->c.n_games; ++g) {
        const size_t o = (size_t)g * AZ_NCNT;
        const long long* c0 = s->prof_cnt0.empty() ? nullptr : s->prof_cnt0.data() + o;
        bs += c[o + CNT_BYTES_SEL] - (c0 ? c0[CNT_BYTES_SEL] : 0);
        be += c[o + CNT_BYTES_EXP] - (c0 ? c0[CNT_BYTES_EXP] : 0);
    }
    // sampled steps' kernel times scaled to every simulation step
    const double k = s->prof_sampled ? (double)s->prof_steps / (double)s->prof_sampled : 0.0;
    if (select_ms) *select_ms = sel * k;
    if (expand_ms) *expand_ms = exp * k;
    if (sim_steps) *sim_steps = s->prof_steps;
    if (select_bytes) *select_bytes = bs;
    if (expand_bytes) *expand_bytes = be;
    return 0;
}

int az_search_profile_read_fused(az_search* s, double* fused_ms, int64_t* fused_launches) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    double f = 0.0;
    const std::vector<double> t = s->pcf.read_ms();
    for (size_t i = 0; i + 1 < t.size(); i += 2) f += t[i + 1] - t[i];
    // sampled fused launches' time scaled to every fused launch
    if (fused_ms) *fused_ms = s->prof_fused ? f * (double)s->prof_fused_launches / (double)s->prof_fused : 0.0;
    if (fused_launches) *fused_launches = s->prof_fused_launches;
    return 0;
}

}  // extern "C"
