// alphazero/selfplay/replay_buffer.h -- ReplayBuffer of the host API: the device-resident ring of action-space
// training targets of the C-ABI (az_replay_*, include/az_engine.h).  The reference has no counterpart: its Dataset
// keeps child-order policies.  SelfPlayManager::setReplayBuffer makes generateGames fill it -- every position a
// game moves from is staged on the device and committed when the game ends, with the visit counts by action, the
// root value q and the outcome z for the side to move -- and a trainer samples it, to host vectors or straight
// into device memory.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "alphazero/core/igamestate.h"

struct az_replay;

namespace alphazero {
namespace selfplay {

class ReplayBuffer {
 public:
    struct Info {
        int64_t committed = 0, totalCommitted = 0, games = 0, dropped = 0, skipped = 0;
    };
    // n samples: states [n][planes][boardSize][boardSize] as the network takes them, policy [n][policySize]
    // = count / sum by action (Go's pass last), z, q; idx / sym: the plan (sample) or the request (gather);
    // gameId, ply: gather only
    struct Batch {
        int n = 0, planes = 0, boardSize = 0, policySize = 0;
        std::vector<float> states, policy, z, q;
        std::vector<int64_t> idx;
        std::vector<int> sym, gameId, ply;
    };

    // capacity: ring positions; maxPlies: positions staged per game (later plies of a game are dropped);
    // device: as HipNeuralNetwork (-1: LOCAL_RANK, default 0)
    ReplayBuffer(core::GameType gameType, int boardSize, int capacity, int maxPlies, int device = -1);
    ~ReplayBuffer();
    ReplayBuffer(const ReplayBuffer&) = delete;
    ReplayBuffer& operator=(const ReplayBuffer&) = delete;

    Info info() const;
    void seed(uint64_t seed);                      // the seed of sample / sampleInto; their call counter restarts
    Batch sample(int n, bool augment = true);
    // one sampling call into device memory of the buffer's device: dStates, dPolicy required, dZ, dQ optional;
    // returns when they are written
    void sampleInto(int n, bool augment, float* dStates, float* dPolicy, float* dZ = nullptr, float* dQ = nullptr);
    Batch gather(const std::vector<int64_t>& idx, const std::vector<int>& sym = {}) const;
    // the raw visit counts [n][policySize] of ring slots idx; sum (optional) receives their sums
    std::vector<int> counts(const std::vector<int64_t>& idx, std::vector<int>* sum = nullptr) const;
    void clear();

    // host only: the cell map of symmetry sym (0 identity; enumeration in az_engine.h) and the sampling plan
    static int symCell(int boardSize, int sym, int cell);
    static std::pair<std::vector<int64_t>, std::vector<int>> samplePlan(uint64_t seed, uint64_t call, int n,
                                                                        int64_t committed, bool augment = true);

    core::GameType gameType() const { return type_; }
    int boardSize() const { return bs_; }
    int planes() const { return planes_; }
    int policySize() const { return na_; }
    az_replay* handle() const { return h_; }

 private:
    core::GameType type_;
    int bs_, planes_, na_;
    az_replay* h_ = nullptr;
};

}  // namespace selfplay
}  // namespace alphazero
