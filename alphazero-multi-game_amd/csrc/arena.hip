// arena.hip -- the two-net evaluation match behind az_arena_* (include/az_engine.h): the game loop
// of the reference's python/scripts/evaluate.py (play_game :186-291, run_evaluation :363-416) for
// T tables in lock step on one search handle with per-slot nets (az_search_set_slot_nets).  Slot 2i
// is net A's tree of table i, slot 2i + 1 net B's; per ply the side to move searches (the other trees
// parked: az_search_run_masked), then the move goes to both trees of its table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/az_engine.h"
#include "engine_internal.h"
#include "net_host.h"
#include "search_host.h"

struct az_arena {
    az_engine* e = nullptr;
    az_search* s = nullptr;
    az_arena_cfg c{};
    int T = 0;
    struct Table {
        int gid = -1;                 // the game it plays (-1: idle)
        int ply = 0;
        std::vector<az_move_rec> moves;
        std::vector<std::vector<float>> pol;
        std::vector<std::vector<int>> cact;
        std::vector<uint8_t> mover;
    };
    std::vector<Table> tab;
    bool begun = false;
    int total = -1, max_moves = 0, next = 0;   // total < 0: ids without end (az_arena_step alone)
    az_arena_sink sink = nullptr; az_progress_fn progress = nullptr; void* user = nullptr;
    std::map<int, double> score;      // finished games: score_a by game id (the Elo order)
    az_arena_summary sum{};
    std::recursive_mutex mu;          // recursive: progress / sink may read the arena back
};

namespace {

// --swap (evaluate.py:365-370): A starts the even games, B the odd ones
bool a_first(const az_arena* a, int gid) { return !a->c.swap_colors || gid % 2 == 0; }

int arena_start(az_arena* a, const std::vector<int>& tables) {
    if (tables.empty()) return 0;
    std::vector<int> slots, ids, open_ids;
    for (int i : tables) {
        az_arena::Table& t = a->tab[i];
        t = az_arena::Table{};
        t.gid = a->next++;
        // az_search_set_openings: both trees of a table play one opening; with swap_colors games 2k and 2k + 1 share it
        const int oid = a->c.swap_colors ? t.gid / 2 : t.gid;
        for (int p = 0; p < 2; ++p) { slots.push_back(2 * i + p); ids.push_back(2 * t.gid + p); open_ids.push_back(oid); }
    }
    az_search* s = a->s;
    std::vector<std::vector<int>> opened;
    {
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->e->device));
        if (int r = search_start_games(s, slots.data(), (int)slots.size(), ids.data(), open_ids.data(), &opened)) return r;
    }
    for (size_t k = 0; k < tables.size(); ++k) {
        az_arena::Table& t = a->tab[tables[k]];
        // the opening plies head the record (no search behind them); the mover is the net that owns the colour
        for (int act : opened[2 * k]) {
            const bool a_moves = (t.ply % 2 == 0) == a_first(a, t.gid);
            t.pol.emplace_back();
            t.cact.emplace_back();
            t.moves.push_back(az_move_rec{act, 0.0f, 0, nullptr, nullptr, 0});
            t.mover.push_back((uint8_t)(a_moves ? 0 : 1));
            t.ply += 1;
        }
    }
    return 0;
}

int arena_begin(az_arena* a, int total, int max_moves) {
    az_search* s = a->s;
    const int G = 2 * a->T;
    {   // every slot idle, then the first min(T, total) games
        std::lock_guard<std::mutex> lk(s->mu);
        HIPCHK(hipSetDevice(s->e->device));
        std::fill(s->active.begin(), s->active.end(), 0);
        HIPCHK(hipMemsetAsync(s->t.active, 0, (size_t)G * sizeof(int), s->e->stream));
        HIPCHK(hipStreamSynchronize(s->e->stream));
    }
    for (auto& t : a->tab) t = az_arena::Table{};
    a->total = total; a->max_moves = max_moves; a->next = 0;
    a->score.clear();
    a->sum = az_arena_summary{};
    a->begun = true;
    std::vector<int> first;
    for (int i = 0; i < a->T && (total < 0 || i < total); ++i) first.push_back(i);
    return arena_start(a, first);
}

// a game cut at max_moves: both trees parked (no search, noise or root step touches them again)
int arena_park(az_arena* a, int table) {
    az_search* s = a->s;
    std::lock_guard<std::mutex> lk(s->mu);
    HIPCHK(hipSetDevice(s->e->device));
    for (int g = 2 * table; g < 2 * table + 2; ++g) {
        if (!s->active[g]) continue;
        s->active[g] = 0;
        HIPCHK(hipMemsetAsync(s->t.active + g, 0, sizeof(int), s->e->stream));
    }
    s->roots_ready = false;
    return 0;
}

int arena_finish(az_arena* a, int table, int result, bool cut) {
    az_arena::Table& t = a->tab[table];
    int64_t ca[5] = {}, cb[5] = {};
    if (int r = az_search_counters(a->s, 2 * table, ca)) return r;
    if (int r = az_search_counters(a->s, 2 * table + 1, cb)) return r;
    if (cut) if (int r = arena_park(a, table)) return r;
    const bool af = a_first(a, t.gid);
    // evaluate.py:259-278: player 1's win is the starter's
    const float score_a = result == 2 ? (af ? 1.0f : 0.0f) : result == 3 ? (af ? 0.0f : 1.0f) : 0.5f;
    for (size_t i = 0; i < t.moves.size(); ++i)
        if (t.moves[i].n_children) { t.moves[i].policy = t.pol[i].data(); t.moves[i].child_actions = t.cact[i].data(); }
    a->sum.games += 1;
    a->sum.wins_a += score_a == 1.0f; a->sum.wins_b += score_a == 0.0f; a->sum.draws += score_a == 0.5f;
    a->sum.evals_a += ca[0]; a->sum.evals_b += cb[0];
    a->score[t.gid] = score_a;
    if (a->sink) {
        const az_arena_game g{t.gid, a->s->c.board_size, af ? 1 : 0, (int)t.moves.size(), t.moves.data(), t.mover.data(),
                              result, score_a, ca[0], cb[0]};
        a->sink(a->user, &g);
    }
    t = az_arena::Table{};
    return 0;
}

int arena_step(az_arena* a, int64_t* moves_done) {
    if (!a->begun) if (int r = arena_begin(a, -1, 0)) return r;
    az_search* s = a->s;
    const int T = a->T, G = 2 * T, NA = s->t.NA;
    const int none = s->t.game == GAME_GO ? AZ_ACTION_NONE : -1;
    std::vector<uint8_t> mask(G, 0);
    std::vector<int> mslot(T, -1);
    bool any = false;
    for (int i = 0; i < T; ++i) {
        const az_arena::Table& t = a->tab[i];
        if (t.gid < 0) continue;
        const bool a_moves = (t.ply % 2 == 0) == a_first(a, t.gid);
        mslot[i] = 2 * i + (a_moves ? 0 : 1);
        mask[mslot[i]] = 1;
        any = true;
    }
    if (!any) return 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (a->c.noise_eps > 0.0f)
        if (int r = az_search_add_noise_masked(s, a->c.noise_alpha, a->c.noise_eps, mask.data())) return r;
    if (int r = az_search_run_masked(s, mask.data())) return r;
    std::vector<int> actions(G), cact((size_t)G * NA), nch(G), term(G), res(G);
    std::vector<float> values(G), probs((size_t)G * NA);
    if (int r = az_search_select(s, 1, a->c.temperature, actions.data(), values.data(), probs.data(), cact.data(), nch.data()))
        return r;
    const int64_t ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
    std::vector<int> apply(G, none);
    for (int i = 0; i < T; ++i) {
        const int g = mslot[i];
        if (g < 0) continue;
        az_arena::Table& t = a->tab[i];
        int act = actions[g];
        if (t.ply < a->c.sample_moves)
            if (int r = az_search_select_action(s, g, 1, a->c.temperature, 0, nullptr, 0, &act)) return r;
        if (act == none) return az_fail(AZ_ERR_STATE, "arena: table %d (game %d) has no move at ply %d", i, t.gid, t.ply);
        t.pol.emplace_back(probs.begin() + (size_t)g * NA, probs.begin() + (size_t)g * NA + nch[g]);
        t.cact.emplace_back(cact.begin() + (size_t)g * NA, cact.begin() + (size_t)g * NA + nch[g]);
        t.moves.push_back(az_move_rec{act, values[g], nch[g], nullptr, nullptr, ms});
        t.mover.push_back((uint8_t)(g & 1));
        a->sum.moves += 1;
        if (moves_done) *moves_done += 1;
        if (a->progress) a->progress(a->user, t.gid, t.ply, a->total, a->sum.moves);
        apply[2 * i] = apply[2 * i + 1] = act;                    // evaluate.py:243-247: both trees
    }
    if (int r = az_search_apply(s, apply.data(), term.data(), res.data())) return r;
    std::vector<int> restart;
    for (int i = 0; i < T; ++i) {
        const int g = mslot[i];
        if (g < 0) continue;
        az_arena::Table& t = a->tab[i];
        t.ply += 1;
        const bool over = term[g] != 0;
        if (!over && !(a->max_moves > 0 && t.ply >= a->max_moves)) continue;
        if (int r = arena_finish(a, i, over ? res[g] : 0, !over)) return r;
        if (a->total < 0 || a->next + (int)restart.size() < a->total) restart.push_back(i);
    }
    return arena_start(a, restart);
}

}  // namespace

extern "C" {

void az_elo_update(double* rating_a, double* rating_b, double score_a, double k_factor) {
    if (!rating_a || !rating_b) return;
    const double ra = *rating_a, rb = *rating_b;
    const double ea = 1.0 / (1.0 + std::pow(10.0, (rb - ra) / 400.0));
    const double eb = 1.0 / (1.0 + std::pow(10.0, (ra - rb) / 400.0));
    *rating_a = ra + k_factor * (score_a - ea);
    *rating_b = rb + k_factor * ((1.0 - score_a) - eb);
}

int az_arena_create(az_engine* e, az_net* na, az_net* nb, const az_search_cfg* search, const az_arena_cfg* cfg, az_arena** out) {
    if (!e || !na || !nb || !search || !cfg || !out) return az_fail(AZ_ERR_ARG, "null argument");
    if (search->eval_kind != AZ_EVAL_NET) return az_fail(AZ_ERR_ARG, "the arena plays two networks (AZ_EVAL_NET)");
    if (search->n_games < 1 || search->n_games > (1 << 20)) return az_fail(AZ_ERR_ARG, "arena tables %d out of range", search->n_games);
    if (cfg->sample_moves < 0 || !(cfg->temperature >= 0.0f) || cfg->noise_eps < 0.0f || cfg->noise_eps > 1.0f ||
        (cfg->noise_eps > 0.0f && !(cfg->noise_alpha > 0.0f)))
        return az_fail(AZ_ERR_ARG, "unsupported arena configuration");
    const int T = search->n_games;
    az_search_cfg sc = *search;
    sc.n_games = 2 * T;
    az_search* s = nullptr;
    if (int r = search_create(e, na, &sc, T, &s)) return r;
    az_net* nets[2] = {na, nb};
    std::vector<uint8_t> slot_net(2 * (size_t)T);
    for (int g = 0; g < 2 * T; ++g) slot_net[g] = (uint8_t)(g & 1);
    if (int r = az_search_set_slot_nets(s, nets, 2, slot_net.data())) { az_search_destroy(s); return r; }
    auto* a = new az_arena();
    a->e = e; a->s = s; a->c = *cfg; a->T = T;
    a->tab.resize(T);
    *out = a;
    return 0;
}

int az_arena_step(az_arena* a, int64_t* moves_done) {
    if (!a) return az_fail(AZ_ERR_ARG, "null arena");
    std::lock_guard<std::recursive_mutex> lk(a->mu);
    return arena_step(a, moves_done);
}

int az_arena_run(az_arena* a, int total_games, int max_moves, az_arena_sink sink, az_progress_fn progress, void* user,
                 const volatile int* abort_flag) {
    if (!a || total_games < 0) return az_fail(AZ_ERR_ARG, "bad argument");
    std::lock_guard<std::recursive_mutex> lk(a->mu);
    a->sink = sink; a->progress = progress; a->user = user;
    int r = arena_begin(a, total_games, max_moves);
    while (!r) {
        bool any = false;
        for (const auto& t : a->tab) any |= t.gid >= 0;
        if (!any || (abort_flag && *abort_flag)) break;
        r = arena_step(a, nullptr);
    }
    a->sink = nullptr; a->progress = nullptr; a->user = nullptr;
    return r;
}

int az_arena_summary_read(az_arena* a, az_arena_summary* out) {
    if (!a || !out) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(a->mu);
    *out = a->sum;
    // evaluate.py:333, :412-416: EloRating(1500, 32), one add_game_result per game in game order
    double ra = 1500.0, rb = 1500.0;
    for (const auto& kv : a->score) az_elo_update(&ra, &rb, kv.second, 32.0);
    out->elo_a = ra; out->elo_b = rb;
    return 0;
}

int az_arena_table_games(az_arena* a, int* game_ids) {
    if (!a || !game_ids) return az_fail(AZ_ERR_ARG, "null argument");
    std::lock_guard<std::recursive_mutex> lk(a->mu);
    for (int i = 0; i < a->T; ++i) game_ids[i] = a->tab[i].gid;
    return 0;
}

az_search* az_arena_search(az_arena* a) { return a ? a->s : nullptr; }

void az_arena_destroy(az_arena* a) {
    if (!a) return;
    az_search_destroy(a->s);
    delete a;
}

}  // extern "C"
