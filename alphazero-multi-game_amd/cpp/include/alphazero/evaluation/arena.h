// alphazero/evaluation/arena.h -- the evaluation match of the reference's python/scripts/evaluate.py
// (play_game :186-291, run_evaluation :294-460) on the device arena (az_arena_* in
// include/az_engine.h), and the Elo arithmetic of python/alphazero/utils/elo.py (EloRating).
#pragma once
#include <cstdint>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "alphazero/core/igamestate.h"
#include "alphazero/mcts/parallel_mcts.h"
#include "alphazero/nn/hip_neural_network.h"
#include "alphazero/selfplay/game_record.h"
#include "az_engine.h"

namespace alphazero {
namespace evaluation {

// elo.py:43-114: ratings by player id, initial rating for unknown players, add_game_result moves both
// players by k (score - expected) with both expectations taken before the game (az_elo_update).
class EloRating {
 public:
    explicit EloRating(double initialRating = 1500.0, double kFactor = 32.0) : initial_(initialRating), k_(kFactor) {}
    double getRating(const std::string& playerId) const;
    // score: 1 win, 0.5 draw, 0 loss of playerId; returns playerId's new rating
    double addGameResult(const std::string& playerId, const std::string& opponentId, double score);
    static double expectedScore(double ratingA, double ratingB);   // elo.py:12-23

 private:
    double initial_, k_;
    std::map<std::string, double> ratings_;
};

struct ArenaConfig {
    core::GameType gameType = core::GameType::GOMOKU;
    int boardSize = 15;
    int tables = 8;              // games in lock step on the device
    int numSimulations = 800;    // evaluate.py --simulations
    float cPuct = 1.5f;          // evaluate.py:387-391
    float fpuReduction = 0.0f;
    int virtualLoss = 3;
    bool swapColors = false;     // evaluate.py --swap
    float temperature = 0.1f;    // evaluate.py --temperature
    int sampleMoves = 0;         // plies drawn with the stochastic selectAction branch
    float noiseAlpha = 0.03f, noiseEpsilon = 0.0f;   // root noise of the mover (evaluate.py adds none)
    uint32_t seed = 42;          // the games' generators: seed + stream id
    int ttLog2 = 20;             // TranspositionTable(1048576, 1024), evaluate.py:336-337
    bool gomokuRenju = false, gomokuOmok = false;   // the Gomoku rule variant both nets' trees play
    // both trees' search options: only selectionStrategy, maxSearchDepth, the TD and the widening fields
    // are read (mcts::searchOptions)
    mcts::MCTSConfig searchOptions;
};

struct ArenaGame {
    int gameId = -1;
    bool aIsPlayer1 = true;
    std::vector<selfplay::MoveData> moves;   // root value / child-order visit distribution of the mover's tree
    std::vector<int> movers;                 // per move: 0 net A, 1 net B
    core::GameResult result = core::GameResult::ONGOING;   // ONGOING: cut at maxMoves
    float scoreA = 0.5f;                     // evaluate.py:259-278
    int64_t evalsA = 0, evalsB = 0;
};

struct ArenaSummary {
    int64_t games = 0, winsA = 0, winsB = 0, draws = 0, moves = 0, evalsA = 0, evalsB = 0;
    double eloA = 1500.0, eloB = 1500.0;
};

// RAII over az_arena: two device nets of one shape, `tables` boards.  Chess is refused
// (std::invalid_argument), as everywhere in the engine; gomokuRenju / gomokuOmok are set on the
// arena's handle right after its creation.
class Arena {
 public:
    Arena(nn::HipNeuralNetwork& a, nn::HipNeuralNetwork& b, const ArenaConfig& config);
    ~Arena();
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;

    int64_t step();                                           // one ply on every live table; moves played
    std::vector<ArenaGame> run(int totalGames, int maxMoves = 0);   // by game id
    ArenaSummary summary() const;
    // Openings (az_search_set_openings on the arena's handle): every game begins with an opening of the book
    // and / or random plies, both trees of its table alike; with swapColors games 2k and 2k + 1 play opening
    // k % book.size() with the colours swapped.  The opening plies head a game's moves (empty policy), their
    // movers follow the colour.  A refused book throws std::runtime_error.
    void setOpenings(const std::vector<std::vector<int>>& book, int randomPlies = 0, uint64_t seed = 0);
    void setProgressCallback(std::function<void(int, int, int, int64_t)> cb) { progress_ = std::move(cb); }
    void setAbort(bool abort) { abort_ = abort ? 1 : 0; }
    az_arena* handle() const { return arena_; }
    const ArenaConfig& config() const { return cfg_; }

 private:
    ArenaConfig cfg_;
    az_arena* arena_ = nullptr;
    std::function<void(int, int, int, int64_t)> progress_;
    volatile int abort_ = 0;
};

}  // namespace evaluation
}  // namespace alphazero
