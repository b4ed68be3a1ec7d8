// Start positions of `katago selfplay` / `gatekeeper` (startPosesFromSgfDir, startPosesFile,
// startPosesLoadProb; the reference's GameInitializer, play.cpp:186-248): the candidates of
// this CLI's own .sgfs files and of *.startposes.txt files, as coffee_start_position samples.
// Host-only and header-only, like cli_config.h; the device check of the samples
// (coffee_start_positions_check) is the caller's.
//
// From an SGF game every proper prefix of length 1 .. moves-1 is a candidate (the final
// position is game over).  Identical move-list prefixes are kept once -- a simplification of
// the reference's position-hash dedup (Sgf::iterAllUniquePositions).  Each candidate is kept
// with probability loadProb, drawn from a stream seeded by the caller (the run seed), in the
// order the candidates are met: directories as listed, files by name, lines in order.
//
// A startposes line is one JSON object {"moves":["ccb","bca"],"weight":1.0} with the moves
// in the SGF writer's three-letter form (column, row, direction a..d) from the empty board,
// black first; optional integers "xSize", "ySize", "winLen" name the geometry.  The
// reference's layout carries a board without its move history; the V1 planes cannot be built
// from that, so it is not accepted (counted as bad).
#pragma once
#include <dirent.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <stdexcept>

#include "../../include/katacoffee.h"
#include "cli_config.h"

namespace kccli {

struct StartPosLoad {
  std::vector<coffee_start_position> samples;
  int64_t files = 0, games = 0, candidates = 0, duplicates = 0, notLoaded = 0, wrongGeometry = 0, bad = 0;
};

// "ccb" -> dir * A + cell, or -1 (also for a coordinate off the x * y board)
inline int startPosParseMove(const std::string& m, int x, int y) {
  static const char* coord = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ";
  if(m.size() != 3)
    return -1;
  const char* cx = strchr(coord, m[0]);
  const char* cy = strchr(coord, m[1]);
  if(!cx || !cy || !m[0] || !m[1] || m[2] < 'a' || m[2] > 'd')
    return -1;
  const int ix = (int)(cx - coord), iy = (int)(cy - coord);
  if(ix >= x || iy >= y)
    return -1;
  return (m[2] - 'a') * (x * y) + iy * x + ix;
}

// The value of SGF property `key` in the game's root node ("" if absent).
inline std::string sgfProp(const std::string& g, const std::string& key) {
  const size_t firstMove = std::min(g.find(";B["), g.find(";W["));
  const size_t p = g.find(key + "[");
  if(p == std::string::npos || p > firstMove || (p > 0 && std::isupper((unsigned char)g[p - 1])))
    return "";
  const size_t a = p + key.size() + 1, b = g.find(']', a);
  return b == std::string::npos ? "" : g.substr(a, b - a);
}

namespace detail {
inline void addCandidate(StartPosLoad& out, std::set<std::string>& seen, std::mt19937_64& rng, double loadProb,
                         const uint16_t* moves, int n, float weight) {
  out.candidates++;
  const std::string key((const char*)moves, (size_t)n * sizeof(uint16_t));
  if(!seen.insert(key).second) {
    out.duplicates++;
    return;
  }
  // 53 random bits as a uniform in [0, 1)
  const double u = (double)(rng() >> 11) * (1.0 / 9007199254740992.0);
  if(!(u < loadProb)) {
    out.notLoaded++;
    return;
  }
  coffee_start_position s;
  memset(&s, 0, sizeof(s));
  s.weight = weight;
  s.num_moves = n;
  memcpy(s.moves, moves, (size_t)n * sizeof(uint16_t));
  out.samples.push_back(s);
}
}  // namespace detail

// One line of an .sgfs file: a game of this CLI's writer (sgfGame in cli_util.h).
inline void startPosFromSgf(const std::string& g, int x, int y, int winLen, double loadProb, std::mt19937_64& rng,
                            std::set<std::string>& seen, StartPosLoad& out) {
  if(g.find("GM[Coffee]") == std::string::npos)
    return;
  out.games++;
  const std::string sz = sgfProp(g, "SZ"), wll = sgfProp(g, "WLL");
  int gx = 0, gy = 0;
  const size_t colon = sz.find(':');
  gx = atoi(sz.c_str());
  gy = colon == std::string::npos ? gx : atoi(sz.c_str() + colon + 1);
  if(gx != x || gy != y || atoi(wll.c_str()) != winLen) {
    out.wrongGeometry++;
    return;
  }
  uint16_t moves[COFFEE_ANALYSIS_MAX_MOVES];
  int n = 0;
  size_t p = 0;
  for(;;) {
    const size_t b = g.find(";B[", p), w = g.find(";W[", p);
    const size_t q = std::min(b, w);
    if(q == std::string::npos)
      break;
    const bool black = q == b;
    const size_t e = g.find(']', q);
    const int mv = e == std::string::npos ? -1 : startPosParseMove(g.substr(q + 3, e - q - 3), x, y);
    if(mv < 0 || black != (n % 2 == 0) || n >= COFFEE_ANALYSIS_MAX_MOVES || n >= x * y) {
      out.bad++;
      return;
    }
    moves[n++] = (uint16_t)mv;
    p = e;
  }
  for(int len = 1; len < n; len++)
    detail::addCandidate(out, seen, rng, loadProb, moves, len, 1.0f);
}

// One line of a startposes file.  Returns false for a line that is not a sample (counted).
inline bool startPosFromJsonLine(const std::string& line, int x, int y, int winLen, double loadProb,
                                 std::mt19937_64& rng, std::set<std::string>& seen, StartPosLoad& out) {
  auto intOf = [&](const char* key, int& v) {
    const size_t p = line.find(std::string("\"") + key + "\"");
    if(p == std::string::npos)
      return false;
    const size_t c = line.find(':', p);
    if(c == std::string::npos)
      return false;
    v = atoi(line.c_str() + c + 1);
    return true;
  };
  const size_t mp = line.find("\"moves\"");
  if(mp == std::string::npos || line.find("\"board\"") != std::string::npos) {
    out.bad++;  // the reference's layout (a board without its history) included
    return false;
  }
  int gx = x, gy = y, gw = winLen;
  intOf("xSize", gx);
  intOf("ySize", gy);
  intOf("winLen", gw);
  if(gx != x || gy != y || gw != winLen) {
    out.wrongGeometry++;
    return false;
  }
  const size_t lb = line.find('[', mp), rb = lb == std::string::npos ? lb : line.find(']', lb);
  if(rb == std::string::npos) {
    out.bad++;
    return false;
  }
  uint16_t moves[COFFEE_ANALYSIS_MAX_MOVES];
  int n = 0;
  size_t p = lb + 1;
  while(p < rb) {
    const size_t a = line.find('"', p);
    if(a == std::string::npos || a > rb)
      break;
    const size_t b = line.find('"', a + 1);
    const int mv = b == std::string::npos || b > rb ? -1 : startPosParseMove(line.substr(a + 1, b - a - 1), x, y);
    if(mv < 0 || n >= COFFEE_ANALYSIS_MAX_MOVES || n >= x * y - 1) {
      out.bad++;
      return false;
    }
    moves[n++] = (uint16_t)mv;
    p = b + 1;
  }
  float weight = 1.0f;
  const size_t wp = line.find("\"weight\"");
  if(wp != std::string::npos) {
    const size_t c = line.find(':', wp);
    char* end = nullptr;
    const double w = c == std::string::npos ? -1.0 : strtod(line.c_str() + c + 1, &end);
    if(c == std::string::npos || end == line.c_str() + c + 1 || !(w >= 0.0) || !std::isfinite(w)) {
      out.bad++;
      return false;
    }
    weight = (float)w;
  }
  detail::addCandidate(out, seen, rng, loadProb, moves, n, weight);
  return true;
}

inline std::vector<std::string> startPosFilesOf(const std::string& dir, const char* suffix) {
  std::vector<std::string> files;
  if(DIR* d = opendir(dir.c_str())) {
    while(dirent* e = readdir(d)) {
      const std::string n = e->d_name;
      const size_t sl = strlen(suffix);
      if(n.size() > sl && n.compare(n.size() - sl, sl, suffix) == 0)
        files.push_back(dir + "/" + n);
    }
    closedir(d);
  }
  std::sort(files.begin(), files.end());
  return files;
}

// sgfDirs: comma-separated directories of .sgfs files; posFile: a startposes file ("" none).
inline StartPosLoad loadStartPositions(const std::string& sgfDirs, const std::string& posFile, int x, int y,
                                       int winLen, double loadProb, uint64_t seed) {
  StartPosLoad out;
  std::set<std::string> seen;
  std::mt19937_64 rng(seed ^ 0x5354415254504F53ULL);
  std::stringstream ds(sgfDirs);
  std::string dir;
  while(std::getline(ds, dir, ',')) {
    const size_t a = dir.find_first_not_of(" \t"), b = dir.find_last_not_of(" \t");
    if(a == std::string::npos)
      continue;
    for(const std::string& f : startPosFilesOf(dir.substr(a, b - a + 1), ".sgfs")) {
      std::ifstream in(f);
      std::string line;
      out.files++;
      while(std::getline(in, line))
        startPosFromSgf(line, x, y, winLen, loadProb, rng, seen, out);
    }
  }
  if(!posFile.empty()) {
    std::ifstream in(posFile);
    std::string line;
    if(in)
      out.files++;
    while(std::getline(in, line))
      if(line.find_first_not_of(" \t\r\n") != std::string::npos)
        startPosFromJsonLine(line, x, y, winLen, loadProb, rng, seen, out);
  }
  return out;
}

// Cumulative weight and effective sample size (sum w)^2 / sum w^2 of the table's
// probabilities w_i = weight * exp(-num_moves * lambda), as the reference logs them.
inline void startPosWeightStats(const std::vector<coffee_start_position>& s, double lambda, double& sum, double& ess) {
  double sq = 0.0;
  sum = 0.0;
  for(const coffee_start_position& p : s) {
    const double w = (double)p.weight * std::exp(-(double)p.num_moves * lambda);
    sum += w;
    sq += w * w;
  }
  ess = sq > 0.0 ? sum * sum / sq : 0.0;
}

// The table of a run (both commands): loaded, checked on the device, logged like the
// reference's loader (kept, dropped, cumulative weight, effective sample size).  An empty
// table logs a line and leaves the feature off.  Every engine of the run gets this table
// (coffee_*_set_start_positions), once: it stays across hot reloads.
template <class LogF>
inline std::vector<coffee_start_position> prepareStartPositions(const StartPosSettings& sp, int x, int y, int winLen,
                                                                uint64_t seed, const char* cmd, LogF&& log) {
  std::vector<coffee_start_position> kept;
  if(!(sp.params.prob > 0.0f))
    return kept;
  if(sp.sgfDirs.empty() && sp.file.empty()) {
    log(std::string(cmd) + ": startPosesProb > 0 but neither startPosesFromSgfDir nor startPosesFile is set: "
                           "start positions off");
    return kept;
  }
  StartPosLoad ld = loadStartPositions(sp.sgfDirs, sp.file, x, y, winLen, sp.loadProb, seed);
  int64_t rejected = 0, zeroWeight = 0;
  if(!ld.samples.empty()) {
    std::vector<int32_t> status(ld.samples.size()), info(ld.samples.size());
    if(coffee_start_positions_check(x, y, winLen, (int)ld.samples.size(), ld.samples.data(), status.data(),
                                    info.data()) != COFFEE_OK)
      throw std::runtime_error(std::string("start positions check: ") + coffee_last_error());
    for(size_t i = 0; i < ld.samples.size(); i++) {
      if(status[i] != COFFEE_ANALYSIS_OK)
        rejected++;
      else if(!(ld.samples[i].weight > 0.0f))
        zeroWeight++;
      else
        kept.push_back(ld.samples[i]);
    }
  }
  double sum = 0.0, ess = 0.0;
  startPosWeightStats(kept, sp.params.turn_weight_lambda, sum, ess);
  log(std::string(cmd) + ": start positions: " + std::to_string(ld.files) + " files, " + std::to_string(ld.games) +
      " games, " + std::to_string(ld.candidates) + " candidates; kept " + std::to_string(kept.size()) +
      ", dropped " + std::to_string(ld.duplicates) + " duplicates, " + std::to_string(ld.notLoaded) +
      " by startPosesLoadProb, " + std::to_string(ld.wrongGeometry) + " of another geometry, " +
      std::to_string(ld.bad) + " unreadable, " + std::to_string(rejected) + " rejected by the rules, " +
      std::to_string(zeroWeight) + " of weight 0");
  log(std::string(cmd) + ": start positions: cumulative weight " + std::to_string(sum) + ", effective sample size " +
      std::to_string(ess) + ", startPosesProb " + std::to_string(sp.params.prob));
  if(kept.empty() || !(sum > 0.0)) {
    log(std::string(cmd) + ": no start positions loaded: start positions off");
    kept.clear();
  }
  return kept;
}

}  // namespace kccli
