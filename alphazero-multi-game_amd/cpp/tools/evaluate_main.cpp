// evaluate -- the reference's model-against-model evaluation (python/scripts/evaluate.py) on the
// MI355X engine: the same flags (:46-74) and the same result file
// <output-dir>/<game>_<a>_vs_<b>.json with the scalar summary keys of :429-460 (no "settings", no
// plots), every game of the match on the device arena (alphazero/evaluation/arena.h).
//
// Engine extensions:
//   --tables N        games in lock step on the device (default min(games, 64))
//   --precision P     trunk precision of both nets: fp16 | f16x3 | bf16x3 | f32 (default: as loaded)
//   --max-moves N     cut games at N moves (a cut game scores 0.5 - 0.5)
//   --device D        the HIP device (default: LOCAL_RANK, else 0)
// Refused: --time-control (the device search counts simulations), --game chess (the reference's
// chess rules recurse without bound) and --variant (this binary plays standard rules; the arena
// itself takes Renju / Omok through ArenaConfig::gomokuRenju / gomokuOmok).  --threads is recorded only.
#include <algorithm>
#include <chrono>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>

#include "alphazero/evaluation/arena.h"
#include "alphazero/nn/hip_neural_network.h"
#include "alphazero/selfplay/game_record.h"
#include "alphazero/selfplay/openings.h"

using namespace alphazero;

namespace {

struct Args {
    std::map<std::string, std::string> kv;
    bool has(const std::string& k) const { return kv.count(k) != 0; }
    std::string get(const std::string& k, const std::string& d) const { return has(k) ? kv.at(k) : d; }
    int getInt(const std::string& k, int d) const { return has(k) ? std::stoi(kv.at(k)) : d; }
    float getFloat(const std::string& k, float d) const { return has(k) ? std::stof(kv.at(k)) : d; }
};

Args parse(int argc, char** argv) {
    Args a;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k.rfind("--", 0) != 0) continue;
        if (i + 1 < argc && std::string(argv[i + 1]).rfind("--", 0) != 0) a.kv[k] = argv[++i];
        else a.kv[k] = "";
    }
    return a;
}

void usage() {
    std::cout << "Usage: evaluate --model-a PATH --model-b PATH [options]\n"
                 "  --model-a PATH          first model file (.pt TorchScript of the reference's ResNet, or .azw)\n"
                 "  --model-b PATH          second model file\n"
                 "  --game TYPE             gomoku | go (default gomoku)\n"
                 "  --size N                board size (default 15 gomoku, 9 go)\n"
                 "  --games N               games to play (default 100)\n"
                 "  --simulations N         MCTS simulations per move (default 800)\n"
                 "  --threads N             recorded only: concurrency is --tables\n"
                 "  --output-dir DIR        result file directory (default results)\n"
                 "  --temperature T         selectAction temperature (default 0.1)\n"
                 "  --swap                  alternate the starting model every game\n"
                 "  --seed S                seed of the games' generators (default 42)\n"
                 "  --tables N              games in lock step on the device (default min(games, 64))\n"
                 "  --precision P           fp16 | f16x3 | bf16x3 | f32 (default: as loaded)\n"
                 "  --max-moves N           cut games at N moves\n"
                 "  --device D              HIP device (default LOCAL_RANK, else 0)\n"
                 "  --openings FILE         openings book: one opening per line, whitespace-separated actions (Go's pass\n"
                 "                          is -1), # comments; with --swap games 2k and 2k + 1 play opening k\n"
                 "  --random-opening-plies N  random legal plies played after the book's, drawn on the device (default 0)\n"
                 "  --openings-seed S       seed of the random opening plies (default 0)\n"
                 "Refused: --time-control, --variant, --game chess\n";
}

int precisionOf(const std::string& s) {
    if (s == "fp16") return AZ_PREC_FP16;
    if (s == "f16x3") return AZ_PREC_F16X3;
    if (s == "bf16x3") return AZ_PREC_BF16X3;
    if (s == "f32") return AZ_PREC_F32;
    throw std::invalid_argument("unknown precision " + s);
}

std::string shortName(const std::string& path) { return std::filesystem::path(path).stem().string(); }

std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

std::unique_ptr<nn::HipNeuralNetwork> loadNet(const std::string& path, core::GameType type, int boardSize) {
    std::unique_ptr<nn::NeuralNetwork> n = nn::NeuralNetwork::create(path, type, boardSize, true);
    auto* hip = dynamic_cast<nn::HipNeuralNetwork*>(n.get());
    if (!hip) throw std::invalid_argument(path + ": not a device network");
    n.release();
    return std::unique_ptr<nn::HipNeuralNetwork>(hip);
}

int run(int argc, char** argv) {
    const Args args = parse(argc, argv);
    if (args.has("--help")) { usage(); return 0; }
    // what the device arena does not play is refused before anything touches the GPU
    if (args.has("--time-control"))
        throw std::invalid_argument("--time-control: the device search counts simulations, not seconds; use --simulations");
    const std::string gameStr = args.get("--game", "gomoku");
    if (args.has("--variant"))
        throw std::invalid_argument("--variant: evaluate plays standard rules only (evaluation::Arena takes Renju / Omok "
                                    "through ArenaConfig)");
    if (gameStr == "chess")
        throw std::invalid_argument("--game chess: the reference's chess rules recurse without bound (DESIGN.md); "
                                    "evaluate plays gomoku and go");
    if (gameStr != "gomoku" && gameStr != "go") throw std::invalid_argument("unknown game " + gameStr);
    const core::GameType type = gameStr == "go" ? core::GameType::GO : core::GameType::GOMOKU;
    const std::string modelA = args.get("--model-a", ""), modelB = args.get("--model-b", "");
    if (modelA.empty() || modelB.empty())
        throw std::invalid_argument("--model-a and --model-b: two model files (the arena plays two device networks)");
    int boardSize = args.getInt("--size", 0);
    if (boardSize <= 0) boardSize = type == core::GameType::GO ? 9 : 15;       // evaluate.py:313-323
    const int games = args.getInt("--games", 100);
    const int simulations = args.getInt("--simulations", 800);
    const int threads = args.getInt("--threads", 4);
    const std::string outputDir = args.get("--output-dir", "results");
    const float temperature = args.getFloat("--temperature", 0.1f);
    const bool swap = args.has("--swap");
    const int tables = args.getInt("--tables", std::max(1, std::min(games, 64)));
    const int maxMoves = args.getInt("--max-moves", 0);
    if (games < 1 || simulations < 1 || tables < 1) throw std::invalid_argument("--games / --simulations / --tables >= 1");
    if (args.has("--device")) (void)nn::engineForDevice(args.getInt("--device", -1));

    auto netA = loadNet(modelA, type, boardSize), netB = loadNet(modelB, type, boardSize);
    if (args.has("--precision")) {
        const int p = precisionOf(args.get("--precision", ""));
        netA->setPrecision(p);
        netB->setPrecision(p);
    }
    const std::string shortA = shortName(modelA), shortB = shortName(modelB);
    std::cout << "Evaluating " << shortA << " vs " << shortB << "\nGame type: " << gameStr << "\nBoard size: " << boardSize
              << "\nNumber of games: " << games << "\nSimulations per move: " << simulations << "\nTemperature: "
              << temperature << "\nTables: " << tables << std::endl;

    evaluation::ArenaConfig cfg;
    cfg.gameType = type;
    cfg.boardSize = boardSize;
    cfg.tables = tables;
    cfg.numSimulations = simulations;
    cfg.swapColors = swap;
    cfg.temperature = temperature;
    cfg.seed = (uint32_t)args.getInt("--seed", 42);
    evaluation::Arena arena(*netA, *netB, cfg);
    const std::string openingsPath = args.get("--openings", "");
    const int randomOpeningPlies = args.getInt("--random-opening-plies", 0);
    const unsigned long long openingsSeed = args.has("--openings-seed") ? std::stoull(args.get("--openings-seed", "0")) : 0ULL;
    if (randomOpeningPlies < 0) throw std::invalid_argument("--random-opening-plies");
    const bool openings = !openingsPath.empty() || randomOpeningPlies > 0;
    if (openings)
        arena.setOpenings(openingsPath.empty() ? selfplay::OpeningBook{} : selfplay::loadOpenings(openingsPath), randomOpeningPlies,
                          openingsSeed);
    const std::vector<evaluation::ArenaGame> recs = arena.run(games, maxMoves);
    const evaluation::ArenaSummary s = arena.summary();

    double moveMs = 0.0;
    for (const auto& g : recs) for (const auto& m : g.moves) moveMs += (double)m.thinking_time_ms;
    const double total = (double)std::max<int64_t>(1, s.games);
    char stamp[32];
    const std::time_t now = std::time(nullptr);
    std::strftime(stamp, sizeof stamp, "%Y-%m-%d %H:%M:%S", std::localtime(&now));
    using selfplay::jsonNumber;
    std::ostringstream js;   // evaluate.py:429-460, json.dump(indent=2)
    js << "{\n"
       << "  \"model_a\": " << quoted(modelA) << ",\n"
       << "  \"model_b\": " << quoted(modelB) << ",\n"
       << "  \"model_a_short\": " << quoted(shortA) << ",\n"
       << "  \"model_b_short\": " << quoted(shortB) << ",\n"
       << "  \"game_type\": " << quoted(gameStr) << ",\n"
       << "  \"board_size\": " << boardSize << ",\n"
       << "  \"variant_rules\": false,\n"
       << "  \"games_played\": " << s.games << ",\n"
       << "  \"wins_a\": " << s.winsA << ",\n"
       << "  \"wins_b\": " << s.winsB << ",\n"
       << "  \"draws\": " << s.draws << ",\n"
       << "  \"win_rate_a\": " << jsonNumber((double)s.winsA / total * 100.0) << ",\n"
       << "  \"win_rate_b\": " << jsonNumber((double)s.winsB / total * 100.0) << ",\n"
       << "  \"draw_rate\": " << jsonNumber((double)s.draws / total * 100.0) << ",\n"
       << "  \"elo_a\": " << jsonNumber(s.eloA) << ",\n"
       << "  \"elo_b\": " << jsonNumber(s.eloB) << ",\n"
       << "  \"simulations\": " << simulations << ",\n"
       << "  \"threads\": " << threads << ",\n"
       << "  \"temperature\": " << jsonNumber((double)temperature) << ",\n"
       << "  \"time_control\": null,\n"
       << "  \"timestamp\": " << quoted(stamp) << ",\n"
       << "  \"avg_move_time\": " << jsonNumber(s.moves ? moveMs / 1000.0 / (double)s.moves : 0.0) << ",\n"
       << "  \"total_moves\": " << s.moves << (openings ? ",\n" : "\n");
    if (openings)   // after the reference's keys, and only for a match that used them
        js << "  \"openings\": " << quoted(openingsPath) << ",\n"
           << "  \"random_opening_plies\": " << randomOpeningPlies << ",\n"
           << "  \"openings_seed\": " << openingsSeed << "\n";
    js << "}\n";
    std::filesystem::create_directories(outputDir);
    const std::string file = (std::filesystem::path(outputDir) / (gameStr + "_" + shortA + "_vs_" + shortB + ".json")).string();
    std::ofstream f(file);
    if (!f) throw std::runtime_error("cannot write " + file);
    f << js.str();
    std::cout << "\nEvaluation Results:\n  " << shortA << ": " << s.winsA << " wins, ELO: " << s.eloA << "\n  " << shortB << ": "
              << s.winsB << " wins, ELO: " << s.eloB << "\n  Draws: " << s.draws << "\n  Total games: " << s.games
              << "\n  Total moves: " << s.moves << "\n\nResults saved to " << file << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception& e) {
        std::cerr << "evaluate: " << e.what() << std::endl;
        return 1;
    }
}
