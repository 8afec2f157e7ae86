// replay.hip -- host side of the device-resident replay buffer (include/az_engine.h az_replay_*): the ring and
// the per-slot staging rows (ReplayDev, tree.h), the hooks the self-play driver calls between its steps
// (search_host.h replay_*), the sampling plan and the gathers.  The kernels are k_replay_stage / k_replay_commit /
// k_replay_gather (tree_kernels.hip); everything runs on the engine stream, so a gather sees every commit queued
// before it.  Lock order: the search handle's mutex, then the buffer's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <vector>

#include "engine_internal.h"
#include "search_host.h"
#include "tree_kernels.h"

struct az_replay {
    az_engine* e = nullptr;
    ReplayDev d{};
    DevPool ring;                          // the ring rows and the counters: the handle's life
    DevPool stage;                         // staging rows, slot ids, commit lists: while attached (sized by the owner's slots)
    DevPool scratch;                       // plan upload and host-form outputs, grow-only
    az_search* owner = nullptr;
    int G = 0;                             // the owner's game slots
    int* d_slots = nullptr; int* d_res = nullptr;   // [G] commit lists
    // scratch for n samples
    int scr_n = 0;
    long long* d_idx = nullptr; int* d_sym = nullptr;
    float* o_states = nullptr; float* o_policy = nullptr; float* o_z = nullptr; float* o_q = nullptr;
    int* o_gid = nullptr; int* o_ply = nullptr;
    uint64_t seed = 0, call = 0;
    // az_diag_replay_profile: HIP events around every stage / commit / gather launch (each then waits for its
    // launch: measurement only), summed per kind
    struct Prof {
        bool on = false;
        hipEvent_t a = nullptr, b = nullptr;
        double ms[3] = {};
        long long n[3] = {};
    } prof;
    std::mutex mu;
};
enum { PROF_STAGE = 0, PROF_COMMIT = 1, PROF_GATHER = 2 };

namespace {

int rows_alloc(DevPool& p, ReplayRows& w, size_t n, const ReplayDev& d, bool ring) {
    if (int rc = p.alloc(&w.rec, n * d.rec)) return rc;
    if (int rc = p.alloc(&w.cnt, n * d.NA)) return rc;
    if (int rc = p.alloc(&w.sum, n)) return rc;
    if (int rc = p.alloc(&w.q, n)) return rc;
    if (int rc = p.alloc(&w.gid, n)) return rc;
    if (int rc = p.alloc(&w.ply, n)) return rc;
    if (int rc = p.alloc(&w.player, n)) return rc;
    if (ring) return p.alloc(&w.z, n);
    return 0;
}

// one launch on the engine stream, between two events when the profile is on
template <class F>
int launch_timed(az_replay* r, int kind, F&& launch) {
    hipStream_t st = r->e->stream;
    az_replay::Prof& p = r->prof;
    if (p.on) HIPCHK(hipEventRecord(p.a, st));
    launch();
    HIPCHK(hipGetLastError());
    if (p.on) {
        HIPCHK(hipEventRecord(p.b, st));
        HIPCHK(hipEventSynchronize(p.b));
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, p.a, p.b));
        p.ms[kind] += ms;
        ++p.n[kind];
    }
    return 0;
}

// the device counters, after everything queued on the engine stream
int read_ctr(az_replay* r, long long* c) {
    HIPCHK(hipMemcpyAsync(c, r->d.ctr, RP_NCTR * sizeof(long long), hipMemcpyDeviceToHost, r->e->stream));
    HIPCHK(hipStreamSynchronize(r->e->stream));
    return 0;
}

int reserve(az_replay* r, int n) {
    if (n <= r->scr_n) return 0;
    HIPCHK(hipStreamSynchronize(r->e->stream));
    r->scratch.clear();
    r->scr_n = 0;
    const size_t m = (size_t)n;
    int rc = r->scratch.alloc(&r->d_idx, m);
    if (!rc) rc = r->scratch.alloc(&r->d_sym, m);
    if (!rc) rc = r->scratch.alloc(&r->o_states, m * r->d.C * r->d.A);
    if (!rc) rc = r->scratch.alloc(&r->o_policy, m * r->d.NA);
    if (!rc) rc = r->scratch.alloc(&r->o_z, m);
    if (!rc) rc = r->scratch.alloc(&r->o_q, m);
    if (!rc) rc = r->scratch.alloc(&r->o_gid, m);
    if (!rc) rc = r->scratch.alloc(&r->o_ply, m);
    if (rc) { r->scratch.clear(); return rc; }
    r->scr_n = n;
    return 0;
}

int check_plan(const int64_t* idx, const int* sym, int n, long long committed) {
    for (int i = 0; i < n; ++i) {
        if (idx[i] < 0 || idx[i] >= committed)
            return az_fail(AZ_ERR_ARG, "replay: index %lld outside [0, %lld)", (long long)idx[i], committed);
        if (sym && (sym[i] < 0 || sym[i] > 7)) return az_fail(AZ_ERR_ARG, "replay: symmetry %d outside 0..7", sym[i]);
    }
    return 0;
}

// the plan on the device (scratch reserved for n)
int upload_plan(az_replay* r, const int64_t* idx, const int* sym, int n) {
    static_assert(sizeof(long long) == sizeof(int64_t), "index width");
    HIPCHK(hipMemcpyAsync(r->d_idx, idx, (size_t)n * 8, hipMemcpyHostToDevice, r->e->stream));
    if (sym) HIPCHK(hipMemcpyAsync(r->d_sym, sym, (size_t)n * 4, hipMemcpyHostToDevice, r->e->stream));
    return 0;
}

// gather of a checked plan to the host buffers; leaves the stream drained
int gather_host(az_replay* r, const int64_t* idx, const int* sym, int n, float* states, float* policy, float* z, float* q,
                int* gid, int* ply) {
    if (int rc = reserve(r, n)) return rc;
    hipStream_t st = r->e->stream;
    int rc = upload_plan(r, idx, sym, n);
    hipError_t he = hipSuccess;
    if (!rc)
        rc = launch_timed(r, PROF_GATHER, [&] {
            az_launch_replay_gather(r->d, r->d_idx, sym ? r->d_sym : nullptr, n, r->o_states, r->o_policy, r->o_z, r->o_q,
                                    r->o_gid, r->o_ply, st);
        });
    if (!rc) {
        const size_t row = (size_t)r->d.C * r->d.A;
        if (he == hipSuccess) he = hipMemcpyAsync(states, r->o_states, (size_t)n * row * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess) he = hipMemcpyAsync(policy, r->o_policy, (size_t)n * r->d.NA * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && z) he = hipMemcpyAsync(z, r->o_z, (size_t)n * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && q) he = hipMemcpyAsync(q, r->o_q, (size_t)n * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && gid) he = hipMemcpyAsync(gid, r->o_gid, (size_t)n * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && ply) he = hipMemcpyAsync(ply, r->o_ply, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (he == hipSuccess) he = se;
    if (!rc && he != hipSuccess) rc = az_fail(AZ_ERR_HIP, "replay gather: %s", hipGetErrorString(he));
    return rc;
}

// the slot ids and empty staging of the owner's slots `games` (null: all); s->mu and r->mu held
int reset_slots(az_replay* r, az_search* s, const int* games, int n) {
    hipStream_t st = r->e->stream;
    if (!games) {
        HIPCHK(hipMemsetAsync(r->d.st_n, 0, (size_t)r->G * sizeof(int), st));
    } else {   // one memset per run of consecutive slots (all slots: one)
        std::vector<int> g(games, games + n);
        std::sort(g.begin(), g.end());
        for (size_t i = 0; i < g.size();) {
            size_t j = i + 1;
            while (j < g.size() && g[j] <= g[j - 1] + 1) ++j;
            HIPCHK(hipMemsetAsync(r->d.st_n + g[i], 0, (size_t)(g[j - 1] - g[i] + 1) * sizeof(int), st));
            i = j;
        }
    }
    HIPCHK(hipMemcpyAsync(r->d.slot_gid, s->slot_id.data(), (size_t)r->G * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

// ---- the self-play driver's hooks (search_host.h); the caller holds s->mu and has set the device
int replay_stage(az_search* s) {
    az_replay* r = s->replay;
    std::lock_guard<std::mutex> lk(r->mu);
    s->t.nd = s->arena[s->cur];
    return launch_timed(r, PROF_STAGE, [&] { az_launch_replay_stage(s->t, r->d, s->d_actions, s->d_values, s->e->stream); });
}

int replay_commit(az_search* s, const std::vector<int>& slots, const std::vector<int>& results) {
    az_replay* r = s->replay;
    const int n = (int)slots.size();
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(r->mu);
    hipStream_t st = s->e->stream;
    HIPCHK(hipMemcpyAsync(r->d_slots, slots.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(r->d_res, results.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (int rc = launch_timed(r, PROF_COMMIT, [&] { az_launch_replay_commit(r->d, r->d_slots, r->d_res, n, st); })) return rc;
    HIPCHK(hipStreamSynchronize(st));      // the lists are the caller's
    return 0;
}

int replay_discard(az_search* s, const int* games, int n) {
    az_replay* r = s->replay;
    std::lock_guard<std::mutex> lk(r->mu);
    return reset_slots(r, s, games, n);
}

void replay_detach(az_search* s) {
    az_replay* r = s->replay;
    if (!r) return;
    std::lock_guard<std::mutex> lk(r->mu);
    (void)hipStreamSynchronize(s->e->stream);
    r->stage.clear();
    r->d.st = ReplayRows{};
    r->d.st_n = nullptr; r->d.slot_gid = nullptr;
    r->d_slots = nullptr; r->d_res = nullptr;
    r->G = 0;
    r->owner = nullptr;
    s->replay = nullptr;
}

extern "C" {

int az_replay_create(az_engine* e, const az_replay_cfg* cfg, az_replay** out) {
    if (!e || !cfg || !out) return az_fail(AZ_ERR_ARG, "null argument");
    if (cfg->game != AZ_GAME_GOMOKU && cfg->game != AZ_GAME_GO)
        return az_fail(AZ_ERR_ARG, "replay: game type %d has no device rules (Gomoku and Go only)", cfg->game);
    if (cfg->board_size < 2 || cfg->board_size * cfg->board_size > AZ_MAXA)
        return az_fail(AZ_ERR_ARG, "replay: board size %d out of range", cfg->board_size);
    if (cfg->capacity < 1 || cfg->max_plies < 1)
        return az_fail(AZ_ERR_ARG, "replay: capacity %d, max_plies %d (both at least 1)", cfg->capacity, cfg->max_plies);
    HIPCHK(hipSetDevice(e->device));
    auto* r = new az_replay();
    r->e = e;
    ReplayDev& d = r->d;
    d.game = cfg->game == AZ_GAME_GO ? GAME_GO : GAME_GOMOKU;
    d.bs = cfg->board_size;
    d.A = d.bs * d.bs;
    d.NA = d.game == GAME_GO ? d.A + 1 : d.A;
    d.C = d.game == GAME_GO ? 8 : 11;
    d.moff = ((d.game == GAME_GO ? 2 * d.A : d.A) + 3) & ~3;
    d.rec = (d.moff + 32 + 15) & ~15;
    d.capacity = cfg->capacity;
    d.max_plies = cfg->max_plies;
    int rc = rows_alloc(r->ring, d.ring, (size_t)d.capacity, d, true);
    if (!rc) rc = r->ring.alloc(&d.ctr, (size_t)RP_NCTR);
    if (!rc && hipMemset(d.ctr, 0, RP_NCTR * sizeof(long long)) != hipSuccess) rc = az_fail(AZ_ERR_HIP, "replay init");
    if (rc) { delete r; return rc; }
    *out = r;
    return 0;
}

void az_replay_destroy(az_replay* r) {
    if (!r) return;
    (void)hipSetDevice(r->e->device);
    if (az_search* s = r->owner) {
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->replay == r) replay_detach(s);
    }
    (void)hipStreamSynchronize(r->e->stream);
    if (r->prof.a) (void)hipEventDestroy(r->prof.a);
    if (r->prof.b) (void)hipEventDestroy(r->prof.b);
    delete r;   // its pools free every device buffer
}

int az_search_attach_replay(az_search* s, az_replay* r) {
    if (!s) return az_fail(AZ_ERR_ARG, "null search");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    if (!r) { replay_detach(s); return 0; }
    if (r->e != s->e) return az_fail(AZ_ERR_ARG, "replay: the buffer belongs to another engine");
    if (r->d.game != s->t.game || r->d.bs != s->t.bs)
        return az_fail(AZ_ERR_ARG, "replay: buffer of game %d board %d, search handle of game %d board %d", r->d.game, r->d.bs,
                       s->t.game, s->t.bs);
    if (s->replay == r) return 0;
    {
        std::lock_guard<std::mutex> lr(r->mu);
        if (r->owner) return az_fail(AZ_ERR_STATE, "replay: the buffer is attached to another search handle");
    }
    replay_detach(s);
    std::lock_guard<std::mutex> lr(r->mu);
    if (r->owner) return az_fail(AZ_ERR_STATE, "replay: the buffer is attached to another search handle");
    const int G = s->c.n_games;
    int rc = rows_alloc(r->stage, r->d.st, (size_t)G * r->d.max_plies, r->d, false);
    if (!rc) rc = r->stage.alloc(&r->d.st_n, (size_t)G);
    if (!rc) rc = r->stage.alloc(&r->d.slot_gid, (size_t)G);
    if (!rc) rc = r->stage.alloc(&r->d_slots, (size_t)G);
    if (!rc) rc = r->stage.alloc(&r->d_res, (size_t)G);
    r->G = G;
    if (!rc) rc = reset_slots(r, s, nullptr, 0);
    if (rc) {
        r->stage.clear();
        r->d.st = ReplayRows{};
        r->d.st_n = nullptr; r->d.slot_gid = nullptr; r->d_slots = nullptr; r->d_res = nullptr;
        r->G = 0;
        return rc;
    }
    r->owner = s;
    s->replay = r;
    return 0;
}

int az_replay_info(az_replay* r, int64_t* committed, int64_t* total_committed, int64_t* games, int64_t* dropped,
                   int64_t* skipped) {
    if (!r) return az_fail(AZ_ERR_ARG, "null replay buffer");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    long long c[RP_NCTR];
    if (int rc = read_ctr(r, c)) return rc;
    if (committed) *committed = std::min<long long>(c[RP_HEAD], r->d.capacity);
    if (total_committed) *total_committed = c[RP_HEAD];
    if (games) *games = c[RP_GAMES];
    if (dropped) *dropped = c[RP_DROPPED];
    if (skipped) *skipped = c[RP_SKIPPED];
    return 0;
}

int az_replay_seed(az_replay* r, uint64_t seed) {
    if (!r) return az_fail(AZ_ERR_ARG, "null replay buffer");
    std::lock_guard<std::mutex> lk(r->mu);
    r->seed = seed;
    r->call = 0;
    return 0;
}

int az_replay_sample_plan(uint64_t seed, uint64_t call, int n, int64_t committed, int augment, int64_t* idx, int* sym) {
    if (n < 0 || (n && (!idx || !sym))) return az_fail(AZ_ERR_ARG, "replay plan: bad argument");
    if (committed < 1 || committed > (int64_t)UINT32_MAX) return az_fail(AZ_ERR_ARG, "replay plan: committed out of range");
    for (int i = 0; i < n; ++i) {
        uint32_t c[4] = {(uint32_t)i, (uint32_t)call, (uint32_t)(call >> 32), 0u};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        idx[i] = (int64_t)(((uint64_t)c[0] * (uint64_t)committed) >> 32);
        sym[i] = augment ? (int)(c[1] & 7u) : 0;
    }
    return 0;
}

int az_replay_sym_cell(int board_size, int sym, int cell) {
    if (board_size < 1 || sym < 0 || sym > 7 || cell < 0 || cell >= board_size * board_size) return -1;
    return replay_sym_cell(board_size, sym, cell);
}

int az_replay_gather(az_replay* r, const int64_t* idx, const int* sym, int n, float* states, float* policy, float* z,
                     float* q, int* game_id, int* ply) {
    if (!r || n < 0 || (n && (!idx || !states || !policy))) return az_fail(AZ_ERR_ARG, "replay gather: bad argument");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    long long c[RP_NCTR];
    if (int rc = read_ctr(r, c)) return rc;
    if (int rc = check_plan(idx, sym, n, std::min<long long>(c[RP_HEAD], r->d.capacity))) return rc;
    if (n == 0) return 0;
    return gather_host(r, idx, sym, n, states, policy, z, q, game_id, ply);
}

int az_replay_sample(az_replay* r, int n, int augment, float* states, float* policy, float* z, float* q, int64_t* idx_out,
                     int* sym_out) {
    if (!r || n < 0 || (n && (!states || !policy))) return az_fail(AZ_ERR_ARG, "replay sample: bad argument");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    long long c[RP_NCTR];
    if (int rc = read_ctr(r, c)) return rc;
    const long long committed = std::min<long long>(c[RP_HEAD], r->d.capacity);
    if (committed == 0) return az_fail(AZ_ERR_STATE, "replay sample: the buffer is empty");
    std::vector<int64_t> idx((size_t)n);
    std::vector<int> sym((size_t)n);
    if (int rc = az_replay_sample_plan(r->seed, r->call, n, committed, augment, idx.data(), sym.data())) return rc;
    if (n)
        if (int rc = gather_host(r, idx.data(), sym.data(), n, states, policy, z, q, nullptr, nullptr)) return rc;
    ++r->call;
    if (idx_out) std::copy(idx.begin(), idx.end(), idx_out);
    if (sym_out) std::copy(sym.begin(), sym.end(), sym_out);
    return 0;
}

int az_replay_sample_device(az_replay* r, int n, int augment, float* d_states, float* d_policy, float* d_z, float* d_q) {
    if (!r || n < 0 || (n && (!d_states || !d_policy))) return az_fail(AZ_ERR_ARG, "replay sample: bad argument");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    long long c[RP_NCTR];
    if (int rc = read_ctr(r, c)) return rc;
    const long long committed = std::min<long long>(c[RP_HEAD], r->d.capacity);
    if (committed == 0) return az_fail(AZ_ERR_STATE, "replay sample: the buffer is empty");
    std::vector<int64_t> idx((size_t)n);
    std::vector<int> sym((size_t)n);
    if (int rc = az_replay_sample_plan(r->seed, r->call, n, committed, augment, idx.data(), sym.data())) return rc;
    if (n) {
        if (int rc = reserve(r, n)) return rc;
        int rc = upload_plan(r, idx.data(), sym.data(), n);
        if (!rc)
            rc = launch_timed(r, PROF_GATHER, [&] {
                az_launch_replay_gather(r->d, r->d_idx, r->d_sym, n, d_states, d_policy, d_z, d_q, nullptr, nullptr,
                                        r->e->stream);
            });
        const hipError_t se = hipStreamSynchronize(r->e->stream);
        if (!rc && se != hipSuccess) rc = az_fail(AZ_ERR_HIP, "replay sample: %s", hipGetErrorString(se));
        if (rc) return rc;
    }
    ++r->call;
    return 0;
}

int az_replay_counts(az_replay* r, const int64_t* idx, int n, int* counts, int* sum) {
    if (!r || n < 0 || (n && (!idx || !counts))) return az_fail(AZ_ERR_ARG, "replay counts: bad argument");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    long long c[RP_NCTR];
    if (int rc = read_ctr(r, c)) return rc;
    if (int rc = check_plan(idx, nullptr, n, std::min<long long>(c[RP_HEAD], r->d.capacity))) return rc;
    if (n == 0) return 0;
    if (int rc = reserve(r, n)) return rc;
    hipStream_t st = r->e->stream;
    int rc = upload_plan(r, idx, nullptr, n);
    hipError_t he = hipSuccess;
    if (!rc) {
        // the counts rows borrow the policy scratch ([n][NA] 4-byte entries), the sums the game-id scratch
        int* dc = reinterpret_cast<int*>(r->o_policy);
        az_launch_replay_counts(r->d, r->d_idx, n, dc, r->o_gid, st);
        he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(counts, dc, (size_t)n * r->d.NA * 4, hipMemcpyDeviceToHost, st);
        if (he == hipSuccess && sum) he = hipMemcpyAsync(sum, r->o_gid, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (he == hipSuccess) he = se;
    if (!rc && he != hipSuccess) rc = az_fail(AZ_ERR_HIP, "replay counts: %s", hipGetErrorString(he));
    return rc;
}

// Measurement (tools/replay_bench.py; not part of az_engine.h): enable != 0 resets the sums and times every stage /
// commit / gather launch from now on with HIP events, each launch waited for; 0 stops.  ms[3] / launches[3]
// (optional): the sums so far, in that order.
int az_diag_replay_profile(az_replay* r, int enable, double* ms, int64_t* launches) {
    if (!r) return az_fail(AZ_ERR_ARG, "null replay buffer");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    az_replay::Prof& p = r->prof;
    for (int k = 0; k < 3; ++k) {
        if (ms) ms[k] = p.ms[k];
        if (launches) launches[k] = p.n[k];
    }
    if (enable) {
        if (!p.a) HIPCHK(hipEventCreate(&p.a));
        if (!p.b) HIPCHK(hipEventCreate(&p.b));
        if (!p.on)
            for (int k = 0; k < 3; ++k) { p.ms[k] = 0.0; p.n[k] = 0; }
    }
    p.on = enable != 0;
    return 0;
}

int az_replay_clear(az_replay* r) {
    if (!r) return az_fail(AZ_ERR_ARG, "null replay buffer");
    std::lock_guard<std::mutex> lk(r->mu);
    HIPCHK(hipSetDevice(r->e->device));
    HIPCHK(hipMemsetAsync(r->d.ctr, 0, RP_NCTR * sizeof(long long), r->e->stream));
    HIPCHK(hipStreamSynchronize(r->e->stream));
    return 0;
}

}  // extern "C"
