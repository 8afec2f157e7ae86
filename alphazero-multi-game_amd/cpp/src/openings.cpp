// Openings of the host API: the openings-file parser and the book on a search handle.
#include "alphazero/selfplay/openings.h"

#include <algorithm>
#include <cerrno>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <stdexcept>

namespace alphazero {
namespace selfplay {

OpeningBook parseOpenings(const std::string& text, const std::string& name) {
    OpeningBook book;
    std::istringstream in(text);
    std::string line;
    for (int no = 1; std::getline(in, line); ++no) {
        const std::string body = line.substr(0, line.find('#'));
        std::istringstream words(body);
        std::vector<int> seq;
        std::string w;
        while (words >> w) {
            errno = 0;
            char* end = nullptr;
            const long v = std::strtol(w.c_str(), &end, 10);
            if (end == w.c_str() || *end != '\0' || errno != 0 || v < -1 || v > 1000000)
                throw std::invalid_argument(name + ":" + std::to_string(no) + ": not an action: '" + w + "'");
            seq.push_back((int)v);
        }
        if (!seq.empty()) book.push_back(std::move(seq));
    }
    return book;
}

OpeningBook loadOpenings(const std::string& path) {
    std::ifstream f(path);
    if (!f) throw std::runtime_error("openings file " + path + ": cannot be read");
    std::ostringstream text;
    text << f.rdbuf();
    return parseOpenings(text.str(), path);
}

void applyOpenings(az_search* s, const OpeningBook& book, int randomPlies, uint64_t seed) {
    if (book.empty() && randomPlies == 0) {
        if (az_search_set_openings(s, nullptr)) throw std::runtime_error(az_last_error());
        return;
    }
    size_t stride = 1;
    for (const auto& q : book) stride = std::max(stride, q.size());
    std::vector<int> moves(std::max<size_t>(book.size(), 1) * stride, AZ_ACTION_NONE), n(std::max<size_t>(book.size(), 1), 0);
    for (size_t i = 0; i < book.size(); ++i) {
        std::copy(book[i].begin(), book[i].end(), moves.begin() + i * stride);
        n[i] = (int)book[i].size();
    }
    const az_openings_cfg cfg{moves.data(), n.data(), (int)book.size(), (int)stride, randomPlies, seed};
    if (az_search_set_openings(s, &cfg)) throw std::runtime_error(az_last_error());
}

}  // namespace selfplay
}  // namespace alphazero
