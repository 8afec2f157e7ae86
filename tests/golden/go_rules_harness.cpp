// tests/golden/go_rules_harness.cpp -- TEST INFRASTRUCTURE ONLY (never shipped, never measured).
//
// Golden-vector driver for the Go rule options (komi, Chinese / Japanese scoring, positional
// superko / simple ko).  Links against the minimally patched build of the REFERENCE search that
// tests/golden/gen_go_rules_golden.py compiles in a temp directory (patches P1 / P5 / P6 of
// oracle/build_ref.sh: no arithmetic change) and prints JSON:
//
//   game       the Mode S self-play loop of oracle/ref_harness.cpp's go_game on
//              GoState(bs, komi, chinese, superko), with the noise seed and the
//              transposition-table size as arguments
//   positions  random legal play (passes at weight 1/16) under one scoring x ko combination,
//              komi drawn per position; every position with its board, side to move, ko point,
//              passes, capture counts, legal list, hash, result and both scores (fp32 bits)
//   replay     the same record for one given move list
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
#include "alphazero/games/go/go_state.h"
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

static int run_game(int bs, int sims, int maxMoves, int noiseEachSearch, float cpuct, float fpu, float komi,
                    bool chinese, bool superko, unsigned noiseSeed, size_t ttSize) {
    go::GoState state(bs, komi, chinese, superko);
    mcts::TranspositionTable tt(ttSize);
    mcts::MCTSConfig cfg;
    cfg.numThreads = 1;
    cfg.numSimulations = sims;
    cfg.cPuct = cpuct;
    cfg.fpuReduction = fpu;
    cfg.useBatchInference = false;
    cfg.useBatchedMCTS = false;
    cfg.useDirichletNoise = noiseEachSearch != 0;
    HashEvaluator net;
    mcts::ParallelMCTS m(state, cfg, &net, &tt);
    m.setDeterministicMode(true);
    m.rng_.seed(noiseSeed);
    const float alpha = 0.03f, eps = 0.25f;
    m.addDirichletNoise(alpha, eps);
    std::ostream& o = std::cout;
    o << "{\"mode\":\"go_rules_game\",\"bs\":" << bs << ",\"sims\":" << sims << ",\"init_root\":";
    dump_children(o, m.rootNode_.get());
    o << ",\"moves\":[";
    int ply = 0;
    bool twoPasses = false;
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
    twoPasses = state.isTerminal();
    const auto sc = state.calculateScore();
    o << "],\"terminal\":" << (twoPasses ? 1 : 0) << ",\"result\":" << (int)state.getGameResult() << ",\"captured\":["
      << state.getCapturedStones(1) << "," << state.getCapturedStones(2) << "],\"score\":[" << fbits(sc.first) << ","
      << fbits(sc.second) << "],\"tt_entries\":" << tt.getEntryCount() << "}\n";
    o.flush();
    m.config_.useBatchInference = true;   // ~ParallelMCTS must not delete the stack table
    return 0;
}

static void dump_position(std::ostream& o, const go::GoState& s, const std::vector<int>& moves, float komi, bool chinese,
                          bool superko) {
    const int A = s.getBoardSize() * s.getBoardSize();
    const auto sc = s.calculateScore();
    o << "{\"komi_bits\":" << fbits(komi) << ",\"chinese\":" << (chinese ? 1 : 0) << ",\"superko\":" << (superko ? 1 : 0)
      << ",\"moves\":[";
    for (size_t i = 0; i < moves.size(); ++i) o << (i ? "," : "") << moves[i];
    o << "],\"hash\":\"" << s.getHash() << "\",\"terminal\":" << (s.isTerminal() ? 1 : 0) << ",\"result\":"
      << (int)s.getGameResult() << ",\"player\":" << s.getCurrentPlayer() << ",\"ko\":" << s.getKoPoint()
      << ",\"passes\":" << s.consecutive_passes_ << ",\"captured\":[" << s.getCapturedStones(1) << ","
      << s.getCapturedStones(2) << "],\"score\":[" << fbits(sc.first) << "," << fbits(sc.second) << "],\"legal\":[";
    const auto legal = s.getLegalMoves();
    for (size_t i = 0; i < legal.size(); ++i) o << (i ? "," : "") << legal[i];
    o << "],\"board\":[";
    for (int a = 0; a < A; ++a) o << (a ? "," : "") << s.getStone(a);
    o << "]}";
}

static const float KOMI_SET[6] = {0.0f, 0.5f, 5.5f, 7.0f, 7.5f, -3.5f};

static int run_positions(int bs, int count, unsigned seed, bool chinese, bool superko) {
    std::mt19937 g(seed);
    std::ostream& o = std::cout;
    o << "{\"mode\":\"go_rules_positions\",\"bs\":" << bs << ",\"positions\":[";
    for (int k = 0; k < count; ++k) {
        const float komi = KOMI_SET[g() % 6];
        go::GoState s(bs, komi, chinese, superko);
        const int target = (int)(g() % (unsigned)(2 * bs * bs));
        std::vector<int> moves;
        while ((int)moves.size() < target && !s.isTerminal()) {
            const auto legal = s.getLegalMoves();
            int a = (g() % 16 == 0) ? -1 : legal[1 + g() % (legal.size() - 1 > 0 ? legal.size() - 1 : 1)];
            if (legal.size() == 1) a = -1;
            s.makeMove(a);
            moves.push_back(a);
        }
        if (k) o << ",";
        dump_position(o, s, moves, komi, chinese, superko);
    }
    o << "]}\n";
    return 0;
}

static int run_replay(int bs, float komi, bool chinese, bool superko, int argc, char** argv, int first) {
    go::GoState s(bs, komi, chinese, superko);
    std::vector<int> moves;
    for (int i = first; i < argc; ++i) { moves.push_back(std::atoi(argv[i])); s.makeMove(moves.back()); }
    dump_position(std::cout, s, moves, komi, chinese, superko);
    std::cout << "\n";
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: go_rules_harness game|positions|replay ...\n"); return 2; }
    const std::string mode = argv[1];
    auto I = [&](int i, int d) { return argc > i ? std::atoi(argv[i]) : d; };
    auto F = [&](int i, float d) { return argc > i ? (float)std::atof(argv[i]) : d; };
    if (mode == "game")      // bs sims max_moves noise_each cpuct fpu komi chinese superko noise_seed tt_size
        return run_game(I(2, 9), I(3, 100), I(4, 1000), I(5, 0), F(6, 1.5f), F(7, 0.0f), F(8, 7.5f), I(9, 1) != 0,
                        I(10, 1) != 0, (unsigned)I(11, 42), (size_t)I(12, 1048576));
    if (mode == "positions") // bs count seed chinese superko
        return run_positions(I(2, 9), I(3, 16), (unsigned)I(4, 1), I(5, 1) != 0, I(6, 1) != 0);
    if (mode == "replay")    // bs komi chinese superko moves...
        return run_replay(I(2, 9), F(3, 7.5f), I(4, 1) != 0, I(5, 1) != 0, argc, argv, 6);
    std::fprintf(stderr, "unknown mode\n");
    return 2;
}
