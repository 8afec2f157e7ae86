// tests/golden/search_opts_harness.cpp -- TEST INFRASTRUCTURE ONLY (never shipped, never measured).
//
// Golden-vector driver for the search options of MCTSConfig: selectionStrategy, maxSearchDepth,
// useTemporalDifference / tdLambda and useProgressiveWidening / minVisitsForWidening /
// progressiveWideningBase / progressiveWideningExponent.  Links against the minimally patched build of
// the REFERENCE search that tests/golden/gen_search_opts_golden.py compiles in a temp directory
// (patches P1 / P2 / P5 / P6 of oracle/build_ref.sh: no arithmetic change) and prints JSON:
//
//   game      the Mode S self-play loop of oracle/ref_harness.cpp's run_game (Gomoku or Go) with the
//             options, the virtual loss and the noise seed as arguments; from ply `switch_ply` on
//             (>= 0) a second set of selection / TD options is put in force on the kept tree through
//             the reference's setters (setSelectionStrategy, setConfig)
//   widening  getProgressiveWideningCount(N, children) over a range of N
//
// Evaluators: the HashEvaluator of oracle/ref_harness.cpp (a pure function of the Zobrist hash and
// the last six moves), or the reference's RandomPolicyNetwork(seed); the engine restates both bit
// for bit.
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
#include "alphazero/games/gomoku/gomoku_state.h"
#include "alphazero/nn/random_policy_network.h"
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

class CountingRandom : public nn::RandomPolicyNetwork {
public:
    long calls = 0;
    CountingRandom(int bs, unsigned seed) : nn::RandomPolicyNetwork(core::GameType::GOMOKU, bs, seed) {}
    std::pair<std::vector<float>, float> predict(const core::IGameState& s) override {
        ++calls; return nn::RandomPolicyNetwork::predict(s);
    }
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
    int useWid = 0, widMin = 10;
    float widBase = 2.0f, widExp = 0.5f;
};

static void put(mcts::MCTSConfig& c, const Opts& o) {
    c.selectionStrategy = static_cast<mcts::MCTSNodeSelection>(o.selection);
    c.maxSearchDepth = o.maxDepth;
    c.useTemporalDifference = o.useTd != 0;
    c.tdLambda = o.lambda;
    c.useProgressiveWidening = o.useWid != 0;
    c.minVisitsForWidening = o.widMin;
    c.progressiveWideningBase = o.widBase;
    c.progressiveWideningExponent = o.widExp;
}

static int run_game(bool go, int bs, int sims, int maxMoves, const std::string& evalKind, unsigned evalSeed,
                    int noiseEachSearch, float cpuct, float fpu, int vl, unsigned noiseSeed, const Opts& first,
                    int switchPly, const Opts& second) {
    std::unique_ptr<core::IGameState> state;
    if (go) state = std::make_unique<go::GoState>(bs, 7.5f, true, true);
    else state = std::make_unique<gomoku::GomokuState>(bs, false, false, 1, false);
    mcts::TranspositionTable tt(1048576);
    mcts::MCTSConfig cfg;
    cfg.numThreads = 1;
    cfg.numSimulations = sims;
    cfg.cPuct = cpuct;
    cfg.fpuReduction = fpu;
    cfg.virtualLoss = vl;
    cfg.useBatchInference = false;
    cfg.useBatchedMCTS = false;
    cfg.useDirichletNoise = noiseEachSearch != 0;
    put(cfg, first);
    std::unique_ptr<nn::NeuralNetwork> net;
    HashEvaluator* he = nullptr; CountingRandom* rn = nullptr;
    if (evalKind == "hash") { he = new HashEvaluator(); net.reset(he); }
    else { rn = new CountingRandom(bs, evalSeed); net.reset(rn); }
    {
        mcts::ParallelMCTS m(*state, cfg, net.get(), &tt);
        m.setDeterministicMode(true);
        m.rng_.seed(noiseSeed);
        const float alpha = 0.03f, eps = 0.25f;
        m.addDirichletNoise(alpha, eps);
        std::ostream& o = std::cout;
        o << "{\"mode\":\"search_opts_game\",\"bs\":" << bs << ",\"sims\":" << sims << ",\"init_root\":";
        dump_children(o, m.rootNode_.get());
        o << ",\"moves\":[";
        int ply = 0;
        int minChildN = 0;
        while (!state->isTerminal() && ply < maxMoves) {
            if (ply == switchPly) {
                // the reference's setters, tree kept: setSelectionStrategy, and setConfig for the rest (given
                // useBatchInference off so that it builds no BatchQueue; setDeterministicMode's flag restored)
                m.setSelectionStrategy(static_cast<mcts::MCTSNodeSelection>(second.selection));
                mcts::MCTSConfig c = m.config_;
                c.useBatchInference = false;
                put(c, second);
                m.setConfig(c);
                m.config_.useBatchInference = true;
            }
            m.search();
            const float T = ply >= 30 ? 0.0f : 1.0f;
            auto probs = m.getActionProbabilities(T);
            auto* root = m.rootNode_.get();
            std::ostringstream kids; dump_children(kids, root);
            for (auto& c : root->children) minChildN = std::min(minChildN, c->visitCount.load());
            const int rootN = root->visitCount.load(), rootVL = root->virtualLoss.load();
            const uint32_t rootW = fbits(root->valueSum.load());
            const int action = m.selectAction(true, T);
            const float value = m.getRootValue();
            o << (ply ? "," : "") << "{\"ply\":" << ply << ",\"root\":[" << rootN << "," << rootVL << "," << rootW
              << "],\"children\":" << kids.str() << ",\"probs\":[";
            for (size_t i = 0; i < probs.size(); ++i) o << (i ? "," : "") << fbits(probs[i]);
            o << "],\"action\":" << action << ",\"value\":" << fbits(value) << ",\"tt_lookups\":" << tt.getLookups()
              << ",\"tt_hits\":" << tt.getHits() << ",\"evals\":" << (he ? he->calls : rn->calls) << "}";
            state->makeMove(action);
            m.updateWithMove(action);
            if (ply % 2 == 0) m.addDirichletNoise(alpha, eps);
            ++ply;
        }
        o << "],\"terminal\":" << (state->isTerminal() ? 1 : 0) << ",\"result\":" << (int)state->getGameResult()
          << ",\"min_child_n\":" << minChildN << ",\"tt_entries\":" << tt.getEntryCount() << "}\n";
        o.flush();
        m.config_.useBatchInference = true;   // ~ParallelMCTS must not delete the stack table
    }
    return 0;
}

static int run_widening(float base, float exponent, int children, int n0, int n1) {
    go::GoState state(9, 7.5f, true, true);
    mcts::MCTSConfig cfg;
    cfg.numThreads = 1;
    cfg.useBatchInference = false;
    cfg.progressiveWideningBase = base;
    cfg.progressiveWideningExponent = exponent;
    mcts::ParallelMCTS m(state, cfg, nullptr, nullptr);
    std::cout << "{\"base_bits\":" << fbits(base) << ",\"exponent_bits\":" << fbits(exponent) << ",\"children\":" << children
              << ",\"n0\":" << n0 << ",\"counts\":[";
    for (int n = n0; n <= n1; ++n) std::cout << (n > n0 ? "," : "") << m.getProgressiveWideningCount(n, children);
    std::cout << "]}\n";
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: search_opts_harness game|widening ...\n"); return 2; }
    const std::string mode = argv[1];
    auto I = [&](int i, int d) { return argc > i ? std::atoi(argv[i]) : d; };
    auto F = [&](int i, float d) { return argc > i ? (float)std::atof(argv[i]) : d; };
    auto O = [&](int i) {
        Opts o;
        o.selection = I(i, 1); o.maxDepth = I(i + 1, 1000); o.useTd = I(i + 2, 0); o.lambda = F(i + 3, 0.8f);
        o.useWid = I(i + 4, 0); o.widMin = I(i + 5, 10); o.widBase = F(i + 6, 2.0f); o.widExp = F(i + 7, 0.5f);
        return o;
    };
    if (mode == "game")      // go bs sims max_moves eval eval_seed noise_each cpuct fpu vl noise_seed opts[8] switch_ply opts[8]
        return run_game(I(2, 0) != 0, I(3, 9), I(4, 100), I(5, 1000), argc > 6 ? argv[6] : "hash", (unsigned)I(7, 7),
                        I(8, 0), F(9, 1.5f), F(10, 0.0f), I(11, 3), (unsigned)I(12, 42), O(13), I(21, -1), O(22));
    if (mode == "widening")  // base exponent children n0 n1
        return run_widening(F(2, 2.0f), F(3, 0.5f), I(4, 82), I(5, -4), I(6, 4096));
    std::fprintf(stderr, "unknown mode\n");
    return 2;
}
