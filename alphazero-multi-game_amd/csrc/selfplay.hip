// selfplay.hip -- the self-play driver behind az_selfplay_* (include/az_engine.h): one move of
// every game per step on the search handle's steps (search_host.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include "../../include/az_engine.h"
#include "engine_internal.h"
#include "search_host.h"

extern "C" {

// One playSingleGame move for every active game (self_play_manager.cpp:187-216).
int az_selfplay_step(az_search* s, const az_selfplay_cfg* cfg, int64_t* moves_done, int64_t* evals_done) {
    if (!s || !cfg) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    const int G = s->c.n_games;
    std::vector<long long> c0((size_t)G * AZ_NCNT), c1((size_t)G * AZ_NCNT);
    hipStream_t st = s->e->stream;
    // the counters on the engine stream (a null-stream copy would not wait for its queued kernels)
    if (evals_done) {
        HIPCHK(hipMemcpyAsync(c0.data(), s->t.cnt, c0.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    const auto t0 = std::chrono::steady_clock::now();
    STEP_TRACE("step start");
    if (int r = search_run(s)) return r;
    std::vector<float> temps(G);
    std::vector<int> was_active = s->active;
    std::vector<int> ply0 = s->ply;
    for (int g = 0; g < G; ++g) temps[g] = s->ply[g] >= cfg->temp_drop_move ? cfg->t_final : cfg->t_init;
    std::vector<int> actions(G);
    // the same D2H and MoveData assembly as az_selfplay_run (getActionProbabilities + getRootValue
    // per game, self_play_manager.cpp:187-203); read back with az_selfplay_step_moves
    const int NA = s->t.NA;
    float* probs = s->sp_probs.get((size_t)G * NA);
    int* cact = s->sp_cact.get((size_t)G * NA);
    float* vals = s->sp_values.get(G);
    int* nch = s->sp_nch.get(G);
    if (!probs || !cact || !vals || !nch) return az_fail(AZ_ERR_OOM, "hipHostMalloc (move records)");
    STEP_TRACE("select");
    if (int r = search_select(s, 1, temps.data(), 0.0f, actions.data(), vals, probs, cact, nch))
        return r;
    if (s->replay)
        if (int r = replay_stage(s)) return r;
    STEP_TRACE("apply");
    const int64_t ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    std::vector<int> term(G), res(G);
    if (int r = search_apply_dev(s, term.data(), res.data())) return r;
    if (s->replay) {   // the games this move ended, in slot order
        std::vector<int> fin, fres;
        for (int g = 0; g < G; ++g)
            if (was_active[g] && !s->active[g]) { fin.push_back(g); fres.push_back(res[g]); }
        if (int r = replay_commit(s, fin, fres)) return r;
    }
    int64_t moves = 0;
    std::vector<uint8_t> noise_mask(G, 0);
    const int none = s->t.game == GAME_GO ? AZ_ACTION_NONE : -1;
    s->sp_moves.clear(); s->sp_slots.clear();
    for (int g = 0; g < G; ++g) {
        if (!was_active[g] || actions[g] == none) continue;
        ++moves;
        if (ply0[g] % 2 == 0) noise_mask[g] = 1;
        s->sp_moves.push_back(az_move_rec{actions[g], vals[g], nch[g], probs + (size_t)g * NA, cact + (size_t)g * NA, ms});
        s->sp_slots.push_back(g);
    }
    STEP_TRACE("noise");
    if (int r = search_noise(s, s->c.dirichlet_alpha, s->c.dirichlet_eps, noise_mask.data())) return r;
    STEP_TRACE("restart / counters");
    if (cfg->restart_finished) {
        std::vector<int> fin;
        for (int g = 0; g < G; ++g) if (!s->active[g]) fin.push_back(g);
        if (!fin.empty()) {
            // a restarted slot plays the next game id (slot order), whose evaluator / noise streams
            // it seeds -- as az_selfplay_run hands out ids -- rather than replaying its slot's seed
            std::vector<int> ids(fin.size());
            for (size_t i = 0; i < fin.size(); ++i) ids[i] = s->sp_next_id + (int)i;
            if (int r = search_start_games(s, fin.data(), (int)fin.size(), ids.data(), nullptr, nullptr)) return r;   // openings, if set
            std::vector<uint8_t> m(G, 0);
            for (int g : fin) m[g] = 1;
            if (int r = search_noise(s, s->c.dirichlet_alpha, s->c.dirichlet_eps, m.data())) return r;
        }
    }
    if (s->t.game == GAME_GOMOKU && !s->c.use_dirichlet_each_search) {
        // the next move's noise (games whose next ply is even, self_play_manager.cpp:209-211) is drawn
        // on a host thread while the device searches
        std::vector<uint8_t> want(G, 0);
        for (int g = 0; g < G; ++g) want[g] = s->active[g] && s->ply[g] % 2 == 0;
        prefetch_noise(s, s->c.dirichlet_alpha, want);
    }
    if (moves_done) *moves_done += moves;
    if (evals_done) {
        HIPCHK(hipMemcpyAsync(c1.data(), s->t.cnt, c1.size() * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        long long ev = 0;
        for (int g = 0; g < G; ++g) ev += c1[(size_t)g * AZ_NCNT + CNT_EVALS_TOTAL] - c0[(size_t)g * AZ_NCNT + CNT_EVALS_TOTAL];
        *evals_done += ev;
    }
    STEP_TRACE("step done");
    return 0;
}

int az_selfplay_step_moves(az_search* s, const az_move_rec** moves, const int** slots, int* n) {
    if (!s || !moves || !n) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::mutex> lk(s->mu);
    *moves = s->sp_moves.data();
    if (slots) *slots = s->sp_slots.data();
    *n = (int)s->sp_moves.size();
    return 0;
}

int az_selfplay_run(az_search* s, const az_selfplay_cfg* cfg, int total_games, int max_moves, az_game_sink sink,
                    az_progress_fn progress, void* user, const volatile int* abort_flag) {
    if (!s || !cfg || total_games < 0) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    hipStream_t st = s->e->stream;
    const int G = s->c.n_games, A = s->t.NA;     // child-order records: up to NA children
    const int none = s->t.game == GAME_GO ? AZ_ACTION_NONE : -1;
    struct Rec {
        std::vector<az_move_rec> moves;
        std::vector<std::vector<float>> pol;
        std::vector<std::vector<int>> cact;
    };
    std::vector<Rec> rec(G);
    std::vector<int> game_of(G, -1);
    int next = 0;
    int64_t total_moves = 0;
    // every slot idle, then the first min(G, total) games
    std::fill(s->active.begin(), s->active.end(), 0);
    HIPCHK(hipMemsetAsync(s->t.active, 0, (size_t)G * sizeof(int), st));
    auto start = [&](const std::vector<int>& slots) -> int {
        if (slots.empty()) return 0;
        std::vector<int> ids(slots.size());
        std::vector<uint8_t> mask(G, 0);
        for (size_t i = 0; i < slots.size(); ++i) {
            ids[i] = next++;
            game_of[slots[i]] = ids[i];
            rec[slots[i]] = Rec{};
            mask[slots[i]] = 1;
        }
        // from the empty board, or -- az_search_set_openings -- from the game's opening: its plies head the record
        // (no search behind them: value 0, no children) and the start noise goes on the opened root
        std::vector<std::vector<int>> opened;
        if (int r = search_start_games(s, slots.data(), (int)slots.size(), ids.data(), nullptr, &opened)) return r;
        for (size_t i = 0; i < slots.size(); ++i) {
            Rec& R = rec[slots[i]];
            for (int a : opened[i]) {
                R.pol.emplace_back();
                R.cact.emplace_back();
                R.moves.push_back(az_move_rec{a, 0.0f, 0, nullptr, nullptr, 0});
            }
        }
        return search_noise(s, s->c.dirichlet_alpha, s->c.dirichlet_eps, mask.data());   // :184
    };
    if (s->replay)   // positions staged by earlier calls belong to games this run abandons
        if (int r = replay_discard(s, nullptr, 0)) return r;
    std::vector<int> first;
    for (int g = 0; g < G && g < total_games; ++g) first.push_back(g);
    if (int r = start(first)) return r;
    std::vector<float> temps(G), values(G), probs((size_t)G * A);
    std::vector<int> actions(G), cact((size_t)G * A), nch(G), term(G), res(G);
    for (;;) {
        bool any = false;
        for (int g = 0; g < G; ++g) any |= s->active[g] != 0;
        if (!any || (abort_flag && *abort_flag)) break;
        const auto t0 = std::chrono::steady_clock::now();
        if (int r = search_run(s)) return r;
        for (int g = 0; g < G; ++g) temps[g] = s->ply[g] >= cfg->temp_drop_move ? cfg->t_final : cfg->t_init;  // :236-240
        if (int r = search_select(s, 1, temps.data(), 0.0f, actions.data(), values.data(), probs.data(), cact.data(),
                                  nch.data()))
            return r;
        const int64_t ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
        std::vector<int> was_active = s->active, ply0 = s->ply;
        if (s->replay)
            if (int r = replay_stage(s)) return r;
        for (int g = 0; g < G; ++g) {
            if (!was_active[g] || actions[g] == none) continue;
            Rec& R = rec[g];
            R.pol.emplace_back(probs.begin() + (size_t)g * A, probs.begin() + (size_t)g * A + nch[g]);
            R.cact.emplace_back(cact.begin() + (size_t)g * A, cact.begin() + (size_t)g * A + nch[g]);
            R.moves.push_back(az_move_rec{actions[g], values[g], nch[g], nullptr, nullptr, ms});
            ++total_moves;
            if (progress) progress(user, game_of[g], ply0[g], total_games, total_moves);
        }
        if (int r = search_apply_dev(s, term.data(), res.data())) return r;
        std::vector<uint8_t> noise(G, 0);
        std::vector<int> done, restart;
        for (int g = 0; g < G; ++g) {
            if (!was_active[g]) continue;
            const bool fin = !s->active[g] || (max_moves > 0 && s->ply[g] >= max_moves);
            if (!fin) {
                if (ply0[g] % 2 == 0) noise[g] = 1;                                            // :209-211
                continue;
            }
            done.push_back(g);
        }
        if (int r = search_noise(s, s->c.dirichlet_alpha, s->c.dirichlet_eps, noise.data())) return r;
        if (s->replay) {   // finished or cut (z = 0) games, in slot order, before their slots restart
            std::vector<int> dres;
            for (int g : done) dres.push_back(s->active[g] ? 0 : res[g]);
            if (int r = replay_commit(s, done, dres)) return r;
        }
        for (int g : done) {
            Rec& R = rec[g];
            for (size_t i = 0; i < R.moves.size(); ++i)
                if (R.moves[i].n_children) { R.moves[i].policy = R.pol[i].data(); R.moves[i].child_actions = R.cact[i].data(); }
            const int result = s->active[g] ? 0 : res[g];
            if (s->active[g]) {                     // cut at max_moves: park the slot
                s->active[g] = 0;
                HIPCHK(hipMemsetAsync(s->t.active + g, 0, sizeof(int), st));
            }
            if (sink) sink(user, game_of[g], s->c.board_size, (int)R.moves.size(), R.moves.data(), result);
            rec[g] = Rec{};
            game_of[g] = -1;
            if (next + (int)restart.size() < total_games) restart.push_back(g);
        }
        if (int r = start(restart)) return r;
        if (s->t.game == GAME_GOMOKU && !s->c.use_dirichlet_each_search) {   // as az_selfplay_step
            std::vector<uint8_t> want(G, 0);
            for (int g = 0; g < G; ++g) want[g] = s->active[g] && s->ply[g] % 2 == 0;
            prefetch_noise(s, s->c.dirichlet_alpha, want);
        }
    }
    pf_wait(s);
    if (s->replay)   // an abort leaves games unfinished: their staged positions go
        if (int r = replay_discard(s, nullptr, 0)) return r;
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
