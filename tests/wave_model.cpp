// tests/wave_model.cpp -- TEST INFRASTRUCTURE ONLY: the leaf-parallel ("wave") schedule of the search,
// derived from the CPU restatement's own Search<State, Zob> (oracle/az_oracle.cpp, included unchanged):
// puct, expand, evaluate, the TT and the evaluators are the oracle's, nothing pinned is restated.
//
// A wave of k descents is Search::simulate() cut between its virtual-loss loop and its leaf handling:
//   phase A, j = 0 .. k-1: clone the root state, root virtual loss, first-max PUCT descent, virtual loss
//            on every path node (simulate()'s first half);
//   phase B, j = 0 .. k-1: terminal test / TT lookup / evaluation + store + expansion, then the virtual
//            loss comes off and the value is backed up (simulate()'s second half) on descent j's leaf.
// This is the reference's runSingleSimulation for numThreads = k in the interleaving where every worker
// has applied its virtual loss before any of them looks at its leaf, and the workers then finish in order.
// k = 1 is simulate() itself.
#include "../oracle/az_oracle.cpp"

#include <unordered_set>

namespace {

struct WaveStats { long same_leaf = 0, wave_tt_hits = 0, expanded_miss = 0, short_waves = 0; };

template <class S, class Z>
struct WaveSearch : Search<S, Z> {
    using Base = Search<S, Z>;
    WaveStats ws;
    WaveSearch(const Cfg& c, int g, Evaluator<S>* e, const Z* z) : Base(c, g, e, z) {}

    struct Descent { S s; std::vector<int> path; int ni; bool was_expanded; };

    void wave(int k) {
        auto& nodes = this->nodes;
        std::vector<Descent> d;
        d.reserve(k);
        for (int j = 0; j < k; ++j) {                    // phase A: simulate() up to its virtual-loss loop
            Descent x{this->rootState, {}, this->root, false};
            this->add_vl(nodes[x.ni]);
            x.path.push_back(x.ni);
            int depth = 0;
            while (nodes[x.ni].expanded && !nodes[x.ni].terminal && depth < 1000) {
                const Node& n = nodes[x.ni];
                const int pv = n.N;
                float best = -std::numeric_limits<float>::max();
                int bc = -1;
                for (int i = 0; i < n.nchild; ++i) {
                    const float sc = this->puct(nodes[n.first + i], n, depth, pv);
                    if (sc > best) { best = sc; bc = n.first + i; }
                }
                if (bc < 0) break;
                x.s.play(nodes[bc].action);
                x.path.push_back(bc);
                x.ni = bc;
                ++depth;
            }
            for (int pi : x.path) this->add_vl(nodes[pi]);
            x.was_expanded = nodes[x.ni].expanded;
            for (const Descent& e : d)
                if (e.ni == x.ni) { ++ws.same_leaf; break; }
            d.push_back(std::move(x));
        }
        std::unordered_set<uint64_t> stored;             // hashes whose entry a descent of this wave created
        for (int j = 0; j < k; ++j) {                    // phase B: the rest of simulate(), in descent order
            Descent& x = d[j];
            const int ni = x.ni;
            const S& s = x.s;
            float value = 0.0f;
            if (nodes[ni].terminal) {
                value = convert_value(nodes[ni].result, s.player);
            } else if (s.terminal()) {
                value = convert_value(s.result(), s.player);
                nodes[ni].terminal = true; nodes[ni].result = s.result();
            } else {
                std::vector<float> p;
                const uint64_t h = s.hash();
                if (this->tt.lookup(h, p, value)) {
                    if (stored.count(h)) ++ws.wave_tt_hits;
                    this->expand(ni, s, p);
                } else if (nodes[ni].expanded) {
                    if (!x.was_expanded) ++ws.expanded_miss;
                    value = nodes[ni].N == 0 ? 0.0f : nodes[ni].W / (float)nodes[ni].N;
                } else {
                    this->evaluate(s, p, value);
                    auto it = this->tt.slots.find(h & this->tt.mask);
                    const bool creates = it == this->tt.slots.end() || (it->second.hash != h && it->second.visits < 5);
                    this->tt.store(h, p, value);
                    if (creates) stored.insert(h);
                    this->expand(ni, s, p);
                }
            }
            float v = value;
            for (auto it = x.path.rbegin(); it != x.path.rend(); ++it) {
                Node& n = nodes[*it];
                this->remove_vl(n);
                n.N += 1;
                n.W = n.W + v;
                v = -v;
            }
        }
    }

    // Search::search() with its simulations run as ceil(sims / K) waves, the last one short
    void search_waves(int K) {
        Node& r = this->nodes[this->root];
        if (!r.expanded && !this->rootState.terminal()) {
            std::vector<float> p; float v;
            this->evaluate(this->rootState, p, v);
            this->tt.store(this->rootState.hash(), p, v);
            this->expand(this->root, this->rootState, p);
        }
        if (this->cfg.noise_each_search && this->nodes[this->root].expanded) this->add_noise(this->cfg.alpha, this->cfg.eps);
        for (int done = 0; done < this->cfg.sims;) {
            const int k = std::min(K, this->cfg.sims - done);
            if (k < K) ++ws.short_waves;
            wave(k);
            done += k;
        }
    }
};

// play_games of the oracle with search() replaced by search_waves(K of the ply); the same JSON
template <class S, class Z>
void wave_play_games(const az_oracle_cfg* c, const Cfg& cfg, const Z& z, Evaluator<S>* ev, int seed_stride, const int* ks,
                     int n_ks, std::ostringstream& o, std::ostringstream& so) {
    for (int g = 0; g < c->n_games; ++g) {
        Cfg gc = cfg;
        gc.noise_seed = c->noise_seed + (unsigned)(seed_stride * g);
        WaveSearch<S, Z> m(gc, g, ev, &z);
        S st(cfg.bs, &z);
        long evals0 = ev->calls;
        m.add_noise(cfg.alpha, cfg.eps);
        if (g) o << ",";
        o << "{\"mode\":\"game\",\"bs\":" << cfg.bs << ",\"sims\":" << cfg.sims << ",\"init_root\":";
        m.dump_children(o);
        o << ",\"moves\":[";
        int move = 0;
        while (!st.terminal() && move < cfg.max_moves) {
            const int K = n_ks <= 0 ? 1 : ks[std::min(move, n_ks - 1)];
            m.search_waves(K);
            float T = move >= cfg.temp_drop ? cfg.t_final : cfg.t_init;
            auto probs = m.probs(T);
            std::ostringstream kids; m.dump_children(kids);
            const Node& r = m.nodes[m.root];
            int rN = r.N, rVL = r.VL; uint32_t rW = fbits(r.W);
            int action = m.select_action(true, T);
            float value = m.root_value();
            if (move) o << ",";
            o << "{\"ply\":" << move << ",\"root\":[" << rN << "," << rVL << "," << rW << "],\"children\":" << kids.str()
              << ",\"probs\":[";
            for (size_t i = 0; i < probs.size(); ++i) o << (i ? "," : "") << fbits(probs[i]);
            o << "],\"action\":" << action << ",\"value\":" << fbits(value) << ",\"tt_lookups\":" << m.tt.lookups
              << ",\"tt_hits\":" << m.tt.hits << ",\"evals\":" << (ev->calls - evals0) << "}";
            st.play(action);
            m.apply(action);
            if (move % 2 == 0) m.add_noise(cfg.alpha, cfg.eps);
            ++move;
        }
        GameResult res = st.result();
        o << "],\"terminal\":" << (res != ONGOING ? 1 : 0) << ",\"result\":" << (int)res << "}";
        so << (g ? "," : "") << "{\"same_leaf\":" << m.ws.same_leaf << ",\"wave_tt_hits\":" << m.ws.wave_tt_hits
           << ",\"expanded_miss\":" << m.ws.expanded_miss << ",\"short_waves\":" << m.ws.short_waves << "}";
    }
}
}  // namespace

extern "C" {

// az_oracle_play with a per-ply list of K (ply p searches with ks[min(p, n_ks - 1)] leaves per wave).
// Returns the games' JSON (az_oracle_play's format); *stats_out gets a JSON array of per-game counters
// {same_leaf, wave_tt_hits, expanded_miss, short_waves}.  Both strings are freed with az_oracle_free.
char* wave_model_play(const az_oracle_cfg* c, int seed_stride, const int* ks, int n_ks, az_eval_cb cb, void* user,
                      char** stats_out) {
    Cfg cfg;
    cfg.bs = c->bs; cfg.sims = c->sims; cfg.max_moves = c->max_moves; cfg.vl = c->vl;
    cfg.noise_each_search = c->noise_each_search; cfg.temp_drop = c->temp_drop; cfg.tt_log2 = c->tt_log2;
    cfg.cpuct = c->cpuct; cfg.fpu = c->fpu; cfg.alpha = c->alpha; cfg.eps = c->eps;
    cfg.t_init = c->t_init; cfg.t_final = c->t_final;
    cfg.zobrist_seed = c->zobrist_seed;
    std::ostringstream o, so;
    o << "[";
    so << "[";
    if (stats_out) *stats_out = nullptr;
    if (c->game == 1) {
        GoZobrist z(cfg.bs * cfg.bs, cfg.zobrist_seed);
        HashEval<GoState> he; CallbackEval<GoState> ne(cb, user, c->eval_kind == 2); UniformEval<GoState> ue;
        RandomEval<GoState> re(c->n_games, c->eval_seed);
        Evaluator<GoState>* ev = c->eval_kind == 0 ? (Evaluator<GoState>*)&he : c->eval_kind == 1 ? (Evaluator<GoState>*)&re
                               : c->eval_kind == 4 ? (Evaluator<GoState>*)&ue : (Evaluator<GoState>*)&ne;
        try { wave_play_games<GoState, GoZobrist>(c, cfg, z, ev, seed_stride, ks, n_ks, o, so); }
        catch (const StopPlay&) { return dup("null"); }
    } else {
        Zobrist z(cfg.bs * cfg.bs, cfg.zobrist_seed);
        HashEval<State> he; RandomEval<State> re(c->n_games, c->eval_seed);
        CallbackEval<State> ne(cb, user, c->eval_kind == 2);
        UniformEval<State> ue;
        Evaluator<State>* ev = c->eval_kind == 0 ? (Evaluator<State>*)&he : c->eval_kind == 1 ? (Evaluator<State>*)&re
                             : c->eval_kind == 4 ? (Evaluator<State>*)&ue : (Evaluator<State>*)&ne;
        try { wave_play_games<State, Zobrist>(c, cfg, z, ev, seed_stride, ks, n_ks, o, so); }
        catch (const StopPlay&) { return dup("null"); }
    }
    o << "]";
    so << "]";
    if (stats_out) *stats_out = dup(so.str());
    return dup(o.str());
}

}  // extern "C"
