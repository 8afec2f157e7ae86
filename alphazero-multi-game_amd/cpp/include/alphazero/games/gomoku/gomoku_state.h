// alphazero/games/gomoku/gomoku_state.h -- host Gomoku position (standard rules, Renju, Omok).
// Same observable behaviour as the engine's device rules (tree_kernels.hip K5/K7) and the
// reference GomokuState: Black (1) moves first; Black wins with exactly five
// in a row, White with five or more; draw on a full board; Zobrist keys of ZobristHash(bs, 2, 2,
// seed) (12345 unless given); 11 enhanced feature planes; legal-move order of
// SURVEY.md A.6 (a fresh state's first query: libstdc++ unordered_set order; afterwards
// descending cell index).
// use_renju / use_omok: the cells csrc/gomoku_rules.h forbids Black are missing from the legal list
// and refused by makeMove (Renju decides when both are set, but makeMove then also refuses what
// Omok forbids, as the reference's make_move does); Black to move with no legal cell is a DRAW; the
// "renju" / "omok" feature keys are part of the hash.  Under these rules a terminal test on a board
// with stones counts as a legal-move query (it computes the legal set, as the reference's does).
// The pro-long opening is not supported (throws): DESIGN.md section 6.
#pragma once
#include <cstdint>
#include <vector>

#include "alphazero/core/igamestate.h"

namespace alphazero {
namespace gomoku {

class GomokuState : public core::IGameState {
 public:
    GomokuState(int board_size = 15, bool use_renju = false, bool use_omok = false, int seed = 0,
                bool use_pro_long_opening = false);

    std::vector<int> getLegalMoves() const override;
    bool isLegalMove(int action) const override;
    void makeMove(int action) override;
    bool undoMove() override;
    bool isTerminal() const override { return getGameResult() != core::GameResult::ONGOING; }
    core::GameResult getGameResult() const override;
    int getCurrentPlayer() const override { return current_player; }
    int getBoardSize() const override { return board_size; }
    int getActionSpaceSize() const override { return board_size * board_size; }
    core::Planes getTensorRepresentation() const override;
    core::Planes getEnhancedTensorRepresentation() const override;
    uint64_t getHash() const override;
    std::unique_ptr<core::IGameState> clone() const override;
    std::string actionToString(int action) const override;
    std::optional<int> stringToAction(const std::string& moveStr) const override;
    std::string toString() const override;
    bool equals(const core::IGameState& other) const override;
    std::vector<int> getMoveHistory() const override { return move_history; }
    bool validate() const override;

    bool isUsingRenjuRules() const { return use_renju_; }
    bool isUsingOmokRules() const { return use_omok_; }
    // the rule in force forbids the side to move the empty cell (always false for White)
    bool isForbidden(int action) const;
    bool is_occupied(int action) const { return cells_[action] != 0; }
    std::vector<std::vector<int>> get_board() const;
    // [11][bs*bs] flat planes (NCHW of one sample), the layout az_net_forward takes
    void enhancedPlanes(float* out) const;

    int board_size;
    int current_player;   // 1 = BLACK, 2 = WHITE
    int action;           // last move or -1
    std::vector<int> move_history;

 private:
    int winnerAfter(int a) const;
    int legalCount() const;         // empty cells the side to move may play (fills forbidden_)
    std::vector<uint8_t> cells_;
    std::vector<uint64_t> zkeys_;   // 2*A piece keys, then 2 player keys
    int winner_ = 0;                // 0 none, 1 / 2
    mutable bool queried_ = false;
    bool use_renju_ = false, use_omok_ = false;
    uint64_t zrules_ = 0;           // "renju"[1] ^ "omok"[1] of the rules in force
    // forbidden-cell mask of the position (csrc/gomoku_rules.h), computed on demand
    mutable std::vector<uint64_t> forbidden_;
    mutable int legal_count_ = -1;  // -1: forbidden_ / legal_count_ not computed for this position
};

}  // namespace gomoku
}  // namespace alphazero
