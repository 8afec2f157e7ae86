// Openings: the move sequences games are started from (az_search_set_openings, include/az_engine.h).
//
// The openings file has one opening per line: whitespace-separated actions (cell = row * boardSize + column;
// Go's pass is -1).  `#` starts a comment that runs to the end of the line; blank lines are ignored.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "az_engine.h"

namespace alphazero {
namespace selfplay {

using OpeningBook = std::vector<std::vector<int>>;

// The openings of a file's text; a malformed line throws std::invalid_argument("<name>:<line>: ...").
OpeningBook parseOpenings(const std::string& text, const std::string& name = "<openings>");
// parseOpenings of a file; std::runtime_error when it cannot be read.
OpeningBook loadOpenings(const std::string& path);

// Puts the book and the random plies in force on a search handle (an empty book and no random plies: none).
// A refused book -- an illegal opening, one that ends the game -- throws std::runtime_error(az_last_error());
// the handle stays usable with the openings it had.
void applyOpenings(az_search* s, const OpeningBook& book, int randomPlies, uint64_t seed);

}  // namespace selfplay
}  // namespace alphazero
