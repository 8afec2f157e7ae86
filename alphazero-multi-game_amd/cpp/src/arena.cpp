// arena.cpp -- alphazero::evaluation::Arena / EloRating over the C ABI (az_arena_*, az_elo_update).
#include "alphazero/evaluation/arena.h"

#include <cmath>
#include <stdexcept>

#include "alphazero/selfplay/openings.h"

namespace alphazero {
namespace evaluation {

namespace {

void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + az_last_error());
}

struct RunCtx {
    std::vector<ArenaGame>* games;
    const std::function<void(int, int, int, int64_t)>* progress;
};

void sinkThunk(void* user, const az_arena_game* g) {
    auto* ctx = static_cast<RunCtx*>(user);
    ArenaGame out;
    out.gameId = g->game_id;
    out.aIsPlayer1 = g->a_is_player1 != 0;
    for (int i = 0; i < g->n_moves; ++i) {
        const az_move_rec& m = g->moves[i];
        selfplay::MoveData md;
        md.action = m.action;
        md.policy.assign(m.policy, m.policy + m.n_children);
        md.value = m.value;
        md.thinking_time_ms = m.thinking_time_ms;
        out.moves.push_back(std::move(md));
        out.movers.push_back(g->mover[i]);
    }
    out.result = static_cast<core::GameResult>(g->result);
    out.scoreA = g->score_a;
    out.evalsA = g->evals_a;
    out.evalsB = g->evals_b;
    if (g->game_id >= 0 && g->game_id < (int)ctx->games->size()) (*ctx->games)[g->game_id] = std::move(out);
}

void progressThunk(void* user, int gameId, int move, int totalGames, int64_t totalMoves) {
    auto* ctx = static_cast<RunCtx*>(user);
    if (*ctx->progress) (*ctx->progress)(gameId, move, totalGames, totalMoves);
}

}  // namespace

double EloRating::expectedScore(double ratingA, double ratingB) {
    return 1.0 / (1.0 + std::pow(10.0, (ratingB - ratingA) / 400.0));
}

double EloRating::getRating(const std::string& playerId) const {
    auto it = ratings_.find(playerId);
    return it == ratings_.end() ? initial_ : it->second;
}

double EloRating::addGameResult(const std::string& playerId, const std::string& opponentId, double score) {
    double a = getRating(playerId), b = getRating(opponentId);
    az_elo_update(&a, &b, score, k_);
    ratings_[playerId] = a;
    ratings_[opponentId] = b;
    return a;
}

Arena::Arena(nn::HipNeuralNetwork& a, nn::HipNeuralNetwork& b, const ArenaConfig& config) : cfg_(config) {
    if (config.gameType != core::GameType::GOMOKU && config.gameType != core::GameType::GO)
        throw std::invalid_argument("Arena: gomoku and go (the reference's chess rules recurse without bound)");
    if (a.engine() != b.engine()) throw std::invalid_argument("Arena: the two nets live on different devices");
    az_search_cfg sc{};
    sc.n_games = config.tables;
    sc.board_size = config.boardSize;
    sc.num_simulations = config.numSimulations;
    sc.c_puct = config.cPuct;
    sc.fpu_reduction = config.fpuReduction;
    sc.virtual_loss = config.virtualLoss;
    sc.eval_kind = AZ_EVAL_NET;
    sc.eval_seed = 7;
    sc.zobrist_seed = 12345;
    sc.noise_seed = config.seed;
    sc.noise_seed_stride = 1;
    sc.dirichlet_alpha = config.noiseAlpha;
    sc.dirichlet_eps = config.noiseEpsilon;
    sc.tt_log2 = config.ttLog2;
    sc.game = config.gameType == core::GameType::GO ? AZ_GAME_GO : AZ_GAME_GOMOKU;
    az_arena_cfg ac{};
    ac.swap_colors = config.swapColors ? 1 : 0;
    ac.temperature = config.temperature;
    ac.sample_moves = config.sampleMoves;
    ac.noise_alpha = config.noiseAlpha;
    ac.noise_eps = config.noiseEpsilon;
    check(az_arena_create(a.engine(), a.handle(), b.handle(), &sc, &ac, &arena_), "az_arena_create");
    const az_search_opts so = mcts::searchOptions(config.searchOptions);   // both nets' trees: every slot
    if (az_search_set_options(az_arena_search(arena_), &so) != 0) {
        const std::string msg = az_last_error();
        az_arena_destroy(arena_);
        arena_ = nullptr;
        throw std::runtime_error("az_search_set_options: " + msg);
    }
    const az_gomoku_rules gr{config.gomokuRenju ? 1 : 0, config.gomokuOmok ? 1 : 0, 0};   // right after creation: nothing has moved
    if ((gr.renju || gr.omok) && az_search_set_gomoku_rules(az_arena_search(arena_), &gr) != 0) {
        const std::string msg = az_last_error();
        az_arena_destroy(arena_);
        arena_ = nullptr;
        throw std::runtime_error("az_search_set_gomoku_rules: " + msg);
    }
}

Arena::~Arena() { az_arena_destroy(arena_); }

int64_t Arena::step() {
    int64_t n = 0;
    check(az_arena_step(arena_, &n), "az_arena_step");
    return n;
}

std::vector<ArenaGame> Arena::run(int totalGames, int maxMoves) {
    std::vector<ArenaGame> games(totalGames > 0 ? totalGames : 0);
    RunCtx ctx{&games, &progress_};
    check(az_arena_run(arena_, totalGames, maxMoves, sinkThunk, progressThunk, &ctx, &abort_), "az_arena_run");
    return games;
}

void Arena::setOpenings(const std::vector<std::vector<int>>& book, int randomPlies, uint64_t seed) {
    selfplay::applyOpenings(az_arena_search(arena_), book, randomPlies, seed);
}

ArenaSummary Arena::summary() const {
    az_arena_summary s{};
    check(az_arena_summary_read(arena_, &s), "az_arena_summary_read");
    ArenaSummary o;
    o.games = s.games; o.winsA = s.wins_a; o.winsB = s.wins_b; o.draws = s.draws; o.moves = s.moves;
    o.evalsA = s.evals_a; o.evalsB = s.evals_b; o.eloA = s.elo_a; o.eloB = s.elo_b;
    return o;
}

}  // namespace evaluation
}  // namespace alphazero
