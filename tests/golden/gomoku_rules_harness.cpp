// tests/golden/gomoku_rules_harness.cpp -- TEST INFRASTRUCTURE ONLY (never shipped, never measured).
//
// Golden-vector driver for the Gomoku rule variants (Renju, Omok).  Links against the minimally
// patched build of the REFERENCE that tests/golden/gen_gomoku_rules_golden.py compiles in a temp
// directory (patches P1 / P2 / P5 of oracle/build_ref.sh and P11, the rule checker's accessor
// recursion: no arithmetic change) and prints JSON:
//
//   game       the Mode S self-play loop of oracle/ref_harness.cpp on GomokuState(bs, renju, omok),
//              with the noise seed, the transposition-table size and the search options as arguments
//   positions  seeded random legal play under one rule set; every position with its moves, side to
//              move, legal list in order, hash, terminal flag and result, and for the empty cells the
//              rule checker's five verdicts (lists of the cells where each one holds): Renju
//              overline, double four, double three NOT allowed; Omok overline, double three
//   replay     the same record for one given move list
//   stalemate  seeded random games played to the end until one ends with Black to move, no legal
//              cell and a board that is not full; that game's record
//
// The evaluator is the HashEvaluator of oracle/ref_harness.cpp (a pure function of the Zobrist
// hash and the last six moves), which the engine restates bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>
#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#define private public
#define protected public
#include "alphazero/mcts/parallel_mcts.h"
#include "alphazero/mcts/transposition_table.h"
#include "alphazero/games/gomoku/gomoku_state.h"
#undef private
#undef protected

using namespace alphazero;

static uint32_t fbits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

static uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

class HashEvaluator : public nn::NeuralNetwork {
public:
    long calls = 0;
    std::pair<std::vector<float>, float> predict(const core::IGameState& s) override {
        ++calls;
        const std::vector<int> hist = s.getMoveHistory();
        const int A = s.getActionSpaceSize();
        uint64_t key = splitmix64(s.getHash() ^ 0x5A17C0DEULL);
        for (int i = 0; i < 6; ++i) {
            const int m = i < (int)hist.size() ? hist[hist.size() - 1 - i] : -1;
            key = splitmix64(key + (uint64_t)(uint32_t)(m + 2));
        }
        std::vector<float> p(A, 0.0f);
        for (int a = 0; a < A; ++a) {
            const uint64_t r = splitmix64(key ^ ((uint64_t)(a + 1) * 0x9E3779B97F4A7C15ULL));
            p[a] = (float)(uint32_t)(r >> 40) * (1.0f / 16777216.0f);
        }
        const uint64_t rv = splitmix64(key ^ 0x76A1ULL);
        const float v = ((float)(int32_t)(uint32_t)(rv >> 40) - 8388608.0f) * (1.0f / 8388608.0f);
        return {p, v};
    }
    void predictBatch(const std::vector<std::reference_wrapper<const core::IGameState>>& states,
                      std::vector<std::vector<float>>& ps, std::vector<float>& vs) override {
        ps.clear(); vs.clear();
        for (auto& r : states) { auto pv = predict(r.get()); ps.push_back(pv.first); vs.push_back(pv.second); }
    }
    std::future<std::pair<std::vector<float>, float>> predictAsync(const core::IGameState& s) override {
        std::promise<std::pair<std::vector<float>, float>> pr; pr.set_value(predict(s)); return pr.get_future();
    }
    bool isGpuAvailable() const override { return false; }
    std::string getDeviceInfo() const override { return "hash"; }
    float getInferenceTimeMs() const override { return 0.f; }
    int getBatchSize() const override { return 1; }
    std::string getModelInfo() const override { return "HashEvaluator"; }
    size_t getModelSizeBytes() const override { return 0; }
    void benchmark(int, int) override {}
    void enableDebugMode(bool) override {}
    void printModelSummary() const override {}
};

static void dump_children(std::ostream& o, const mcts::MCTSNode* n) {
    o << "[";
    for (size_t i = 0; i < n->children.size(); ++i) {
        const mcts::MCTSNode* c = n->children[i].get();
        o << (i ? "," : "") << "[" << n->actions[i] << "," << c->visitCount.load() << "," << c->virtualLoss.load() << ","
          << fbits(c->valueSum.load()) << "," << fbits(c->prior) << "]";
    }
    o << "]";
}

struct Opts {
    int selection = 1, maxDepth = 1000, useTd = 0;
    float lambda = 0.8f;
};

static int run_game(int bs, int sims, int maxMoves, int noiseEachSearch, float cpuct, float fpu, bool renju, bool omok,
                    unsigned noiseSeed, size_t ttSize, const Opts& opt) {
    gomoku::GomokuState state(bs, renju, omok, 1, false);
    mcts::TranspositionTable tt(ttSize);
    mcts::MCTSConfig cfg;
    cfg.numThreads = 1;
    cfg.numSimulations = sims;
    cfg.cPuct = cpuct;
    cfg.fpuReduction = fpu;
    cfg.useBatchInference = false;
    cfg.useBatchedMCTS = false;
    cfg.useDirichletNoise = noiseEachSearch != 0;
    cfg.selectionStrategy = static_cast<mcts::MCTSNodeSelection>(opt.selection);
    cfg.maxSearchDepth = opt.maxDepth;
    cfg.useTemporalDifference = opt.useTd != 0;
    cfg.tdLambda = opt.lambda;
    HashEvaluator net;
    mcts::ParallelMCTS m(state, cfg, &net, &tt);
    m.setDeterministicMode(true);
    m.rng_.seed(noiseSeed);
    const float alpha = 0.03f, eps = 0.25f;
    m.addDirichletNoise(alpha, eps);
    std::ostream& o = std::cout;
    o << "{\"mode\":\"gomoku_rules_game\",\"bs\":" << bs << ",\"sims\":" << sims << ",\"init_root\":";
    dump_children(o, m.rootNode_.get());
    o << ",\"moves\":[";
    int ply = 0;
    while (!state.isTerminal() && ply < maxMoves) {
        m.search();
        const float T = ply >= 30 ? 0.0f : 1.0f;
        auto probs = m.getActionProbabilities(T);
        auto* root = m.rootNode_.get();
        std::ostringstream kids; dump_children(kids, root);
        const int rootN = root->visitCount.load(), rootVL = root->virtualLoss.load();
        const uint32_t rootW = fbits(root->valueSum.load());
        const int action = m.selectAction(true, T);
        const float value = m.getRootValue();
        o << (ply ? "," : "") << "{\"ply\":" << ply << ",\"root\":[" << rootN << "," << rootVL << "," << rootW
          << "],\"children\":" << kids.str() << ",\"probs\":[";
        for (size_t i = 0; i < probs.size(); ++i) o << (i ? "," : "") << fbits(probs[i]);
        o << "],\"action\":" << action << ",\"value\":" << fbits(value) << ",\"tt_lookups\":" << tt.getLookups()
          << ",\"tt_hits\":" << tt.getHits() << ",\"evals\":" << net.calls << "}";
        state.makeMove(action);
        m.updateWithMove(action);
        if (ply % 2 == 0) m.addDirichletNoise(alpha, eps);
        ++ply;
    }
    o << "],\"terminal\":" << (state.isTerminal() ? 1 : 0) << ",\"result\":" << (int)state.getGameResult()
      << ",\"tt_entries\":" << tt.getEntryCount() << "}\n";
    o.flush();
    m.config_.useBatchInference = true;   // ~ParallelMCTS must not delete the stack table
    return 0;
}

static void dump_position(std::ostream& o, const gomoku::GomokuState& s, const std::vector<int>& moves) {
    const int A = s.getBoardSize() * s.getBoardSize();
    o << "{\"bs\":" << s.getBoardSize() << ",\"renju\":" << (s.use_renju ? 1 : 0) << ",\"omok\":" << (s.use_omok ? 1 : 0)
      << ",\"moves\":[";
    for (size_t i = 0; i < moves.size(); ++i) o << (i ? "," : "") << moves[i];
    const bool terminal = s.isTerminal();   // the position's legal-set query, before the hash and the list
    o << "],\"hash\":\"" << s.getHash() << "\",\"terminal\":" << (terminal ? 1 : 0) << ",\"result\":"
      << (int)s.getGameResult() << ",\"player\":" << s.getCurrentPlayer() << ",\"legal\":[";
    const auto legal = terminal ? std::vector<int>() : s.getLegalMoves();   // a finished game has no moves
    for (size_t i = 0; i < legal.size(); ++i) o << (i ? "," : "") << legal[i];
    o << "]";
    auto rules = s.getRules();
    const char* names[5] = {"renju_overline", "renju_double_four", "renju_double_three_refused", "omok_overline",
                            "omok_double_three"};
    for (int k = 0; k < 5; ++k) {
        o << ",\"" << names[k] << "\":[";
        bool first = true;
        for (int a = 0; a < A; ++a) {
            if (s.is_occupied(a)) continue;
            const bool v = k == 0 ? rules->renju_is_overline(a) : k == 1 ? rules->renju_double_four_or_more(a)
                         : k == 2 ? !rules->is_allowed_double_three(a) : k == 3 ? rules->omok_is_overline(a)
                                  : rules->omok_check_double_three_strict(a);
            if (v) { o << (first ? "" : ",") << a; first = false; }
        }
        o << "]";
    }
    o << "}";
}

// With both flags set the legal list is Renju's, but make_move also refuses what Omok forbids
// (gomoku_state.cpp:697-703): a playout keeps to the cells make_move takes.
static bool playable(const gomoku::GomokuState& s, int a) {
    return !(s.use_renju && s.use_omok && s.getCurrentPlayer() == gomoku::BLACK && s.getRules()->is_black_omok_forbidden(a));
}

// Plays inside the central (bs - 2 * margin)^2 cells while one is legal there: lines meet sooner.  -1: no cell.
static int pick(std::mt19937& g, const gomoku::GomokuState& s, int bs, int margin) {
    std::vector<int> in, all;
    for (int a : s.getLegalMoves()) {
        if (!playable(s, a)) continue;
        const int x = a / bs, y = a % bs;
        all.push_back(a);
        if (x >= margin && x < bs - margin && y >= margin && y < bs - margin) in.push_back(a);
    }
    const std::vector<int>& from = in.empty() ? all : in;
    return from.empty() ? -1 : from[g() % from.size()];
}

static int run_positions(int bs, int count, unsigned seed, bool renju, bool omok, int margin) {
    std::mt19937 g(seed);
    std::ostream& o = std::cout;
    o << "{\"mode\":\"gomoku_rules_positions\",\"bs\":" << bs << ",\"positions\":[";
    for (int k = 0; k < count; ++k) {
        gomoku::GomokuState s(bs, renju, omok, 1, false);
        const int span = (bs - 2 * margin) * (bs - 2 * margin);
        const int target = (int)(g() % (unsigned)(span + 1));
        std::vector<int> moves;
        while ((int)moves.size() < target && !s.isTerminal()) {
            const int a = pick(g, s, bs, margin);
            if (a < 0) break;
            s.makeMove(a);
            moves.push_back(a);
        }
        if (k) o << ",";
        dump_position(o, s, moves);
    }
    o << "]}\n";
    return 0;
}

static int run_replay(int bs, bool renju, bool omok, int argc, char** argv, int first) {
    gomoku::GomokuState s(bs, renju, omok, 1, false);
    std::vector<int> moves;
    for (int i = first; i < argc; ++i) {
        if (s.isTerminal()) { std::fprintf(stderr, "replay: terminal before move %d\n", i - first); return 3; }
        moves.push_back(std::atoi(argv[i]));
        s.makeMove(moves.back());
    }
    dump_position(std::cout, s, moves);
    std::cout << "\n";
    return 0;
}

static int run_stalemate(int bs, bool renju, bool omok, unsigned firstSeed, int tries) {
    for (int t = 0; t < tries; ++t) {
        std::mt19937 g(firstSeed + (unsigned)t);
        gomoku::GomokuState s(bs, renju, omok, 1, false);
        std::vector<int> moves;
        while (!s.isTerminal()) {
            const auto legal = s.getLegalMoves();
            const int a = legal[g() % legal.size()];
            s.makeMove(a);
            moves.push_back(a);
        }
        if (s.getGameResult() == core::GameResult::DRAW && (int)moves.size() < bs * bs) {
            std::cout << "{\"seed\":" << (firstSeed + (unsigned)t) << ",\"position\":";
            dump_position(std::cout, s, moves);
            std::cout << "}\n";
            return 0;
        }
    }
    std::fprintf(stderr, "stalemate: none in %d games\n", tries);
    return 4;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: gomoku_rules_harness game|positions|replay|stalemate ...\n"); return 2; }
    const std::string mode = argv[1];
    auto I = [&](int i, int d) { return argc > i ? std::atoi(argv[i]) : d; };
    auto F = [&](int i, float d) { return argc > i ? (float)std::atof(argv[i]) : d; };
    if (mode == "game") {    // bs sims max_moves noise_each cpuct fpu renju omok noise_seed tt_size selection max_depth use_td lambda
        Opts o;
        o.selection = I(12, 1); o.maxDepth = I(13, 1000); o.useTd = I(14, 0); o.lambda = F(15, 0.8f);
        return run_game(I(2, 9), I(3, 100), I(4, 1000), I(5, 0), F(6, 1.5f), F(7, 0.0f), I(8, 1) != 0, I(9, 0) != 0,
                        (unsigned)I(10, 42), (size_t)I(11, 1048576), o);
    }
    if (mode == "positions") // bs count seed renju omok margin
        return run_positions(I(2, 9), I(3, 16), (unsigned)I(4, 1), I(5, 1) != 0, I(6, 0) != 0, I(7, 0));
    if (mode == "replay")    // bs renju omok moves...
        return run_replay(I(2, 9), I(3, 1) != 0, I(4, 0) != 0, argc, argv, 5);
    if (mode == "stalemate") // bs renju omok first_seed tries
        return run_stalemate(I(2, 7), I(3, 1) != 0, I(4, 0) != 0, (unsigned)I(5, 1), I(6, 2000));
    std::fprintf(stderr, "unknown mode\n");
    return 2;
}
