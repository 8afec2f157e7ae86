// ReplayBuffer of the host API over az_replay_* (include/az_engine.h).
#include "alphazero/selfplay/replay_buffer.h"

#include <stdexcept>
#include <string>

#include "alphazero/nn/hip_neural_network.h"
#include "az_engine.h"

namespace alphazero {
namespace selfplay {

namespace {
void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + ": " + az_last_error());
}
}  // namespace

ReplayBuffer::ReplayBuffer(core::GameType gameType, int boardSize, int capacity, int maxPlies, int device)
    : type_(gameType) {
    if (gameType != core::GameType::GOMOKU && gameType != core::GameType::GO)
        throw std::invalid_argument("ReplayBuffer: Gomoku or Go (no Chess rules on this engine)");
    const bool go = gameType == core::GameType::GO;
    bs_ = boardSize > 0 ? boardSize : (go ? 19 : 15);
    planes_ = go ? 8 : 11;
    na_ = bs_ * bs_ + (go ? 1 : 0);
    const az_replay_cfg cfg{go ? AZ_GAME_GO : AZ_GAME_GOMOKU, bs_, capacity, maxPlies};
    check(az_replay_create(nn::engineForDevice(device), &cfg, &h_), "az_replay_create");
}

ReplayBuffer::~ReplayBuffer() {
    if (h_) az_replay_destroy(h_);
}

ReplayBuffer::Info ReplayBuffer::info() const {
    Info i;
    check(az_replay_info(h_, &i.committed, &i.totalCommitted, &i.games, &i.dropped, &i.skipped), "az_replay_info");
    return i;
}

void ReplayBuffer::seed(uint64_t seed) { check(az_replay_seed(h_, seed), "az_replay_seed"); }

ReplayBuffer::Batch ReplayBuffer::sample(int n, bool augment) {
    if (n < 0) throw std::invalid_argument("ReplayBuffer::sample: negative count");
    Batch b;
    b.n = n; b.planes = planes_; b.boardSize = bs_; b.policySize = na_;
    b.states.resize((size_t)n * planes_ * bs_ * bs_);
    b.policy.resize((size_t)n * na_);
    b.z.resize(n); b.q.resize(n); b.idx.resize(n); b.sym.resize(n);
    check(az_replay_sample(h_, n, augment ? 1 : 0, b.states.data(), b.policy.data(), b.z.data(), b.q.data(),
                           b.idx.data(), b.sym.data()), "az_replay_sample");
    return b;
}

void ReplayBuffer::sampleInto(int n, bool augment, float* dStates, float* dPolicy, float* dZ, float* dQ) {
    check(az_replay_sample_device(h_, n, augment ? 1 : 0, dStates, dPolicy, dZ, dQ), "az_replay_sample_device");
}

ReplayBuffer::Batch ReplayBuffer::gather(const std::vector<int64_t>& idx, const std::vector<int>& sym) const {
    if (!sym.empty() && sym.size() != idx.size()) throw std::invalid_argument("ReplayBuffer::gather: sym and idx differ in length");
    const int n = (int)idx.size();
    Batch b;
    b.n = n; b.planes = planes_; b.boardSize = bs_; b.policySize = na_;
    b.idx = idx;
    b.sym = sym.empty() ? std::vector<int>(n, 0) : sym;
    b.states.resize((size_t)n * planes_ * bs_ * bs_);
    b.policy.resize((size_t)n * na_);
    b.z.resize(n); b.q.resize(n); b.gameId.resize(n); b.ply.resize(n);
    check(az_replay_gather(h_, idx.data(), sym.empty() ? nullptr : sym.data(), n, b.states.data(), b.policy.data(),
                           b.z.data(), b.q.data(), b.gameId.data(), b.ply.data()), "az_replay_gather");
    return b;
}

std::vector<int> ReplayBuffer::counts(const std::vector<int64_t>& idx, std::vector<int>* sum) const {
    const int n = (int)idx.size();
    std::vector<int> c((size_t)n * na_);
    if (sum) sum->assign(n, 0);
    check(az_replay_counts(h_, idx.data(), n, c.data(), sum ? sum->data() : nullptr), "az_replay_counts");
    return c;
}

void ReplayBuffer::clear() { check(az_replay_clear(h_), "az_replay_clear"); }

int ReplayBuffer::symCell(int boardSize, int sym, int cell) {
    const int c = az_replay_sym_cell(boardSize, sym, cell);
    if (c < 0) throw std::invalid_argument("ReplayBuffer::symCell: argument out of range");
    return c;
}

std::pair<std::vector<int64_t>, std::vector<int>> ReplayBuffer::samplePlan(uint64_t seed, uint64_t call, int n,
                                                                            int64_t committed, bool augment) {
    if (n < 0) throw std::invalid_argument("ReplayBuffer::samplePlan: negative count");
    std::vector<int64_t> idx(n);
    std::vector<int> sym(n);
    check(az_replay_sample_plan(seed, call, n, committed, augment ? 1 : 0, idx.data(), sym.data()), "az_replay_sample_plan");
    return {idx, sym};
}

}  // namespace selfplay
}  // namespace alphazero
