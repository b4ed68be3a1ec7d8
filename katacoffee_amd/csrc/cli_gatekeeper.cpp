// `katago gatekeeper` for Coffee on MI355X: plays a newly trained net against the current
// one and moves its file to the accepted or the rejected directory (the reference's
// command/gatekeeper.cpp).  Host C++ over the C ABI's match engine (coffee_match_*).
//
//   katago gatekeeper -config <cfg> -test-models-dir <dir> -accepted-models-dir <dir>
//                     -rejected-models-dir <dir> -sgf-output-dir <dir> [-selfplay-dir <dir>]
//                     [-quit-if-no-nets-to-test] [-no-autoreject-old-models]
//                     [-override-config k=v,k=v,...]
//
// The candidate is the newest file of the test directory, the baseline the newest file of
// the accepted directory; a candidate older than the baseline is moved to the rejected
// directory without a game unless -no-autoreject-old-models.  numGamesPerGating (N) games
// are played on G = min(numGameThreads, N) concurrent slots of one match engine: game
// number n of slot s counts iff n * G + s < N, the candidate is black iff s + n is even.
// Counted games are tallied in the order the engine hands them out (win 1, draw 0.5 each),
// written to <sgf-output-dir>/<candidate>/<hex>.sgfs with PB / PW the two model names, and
// play stops as soon as the remaining games cannot change the verdict.  The candidate wins
// ties.  On acceptance <selfplay-dir>/<candidate>/{sgfs,tdata,vadata} are made first.
// Without -quit-if-no-nets-to-test the test directory is polled for the next candidate.
// Config: the search keys of cli_config.h on coffee_match_params_default; keys of the
// reference's gatekeeper config that only mean something for Go are ignored, as for
// selfplay.  allowResignation is noted once: a Coffee game has at most A moves and is
// played out.
#include <atomic>
#include <chrono>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../include/katacoffee.h"
#include "cli_config.h"
#include "cli_startpos.h"
#include "cli_util.h"

using namespace kccli;

namespace {

std::atomic<bool> gQuit(false);
void onQuit(int) { gQuit = true; }

[[noreturn]] void fail(const std::string& msg) {
  fprintf(stderr, "katago gatekeeper: %s\n", msg.c_str());
  exit(1);
}

void must(int rc, const char* what) {
  if(rc != COFFEE_OK)
    fail(std::string(what) + ": " + coffee_last_error());
}

struct Dirs {
  std::string test, accepted, rejected, sgf, selfplay;
};

void moveModel(const std::string& file, const std::string& toDir) {
  mkdirs(toDir);
  const std::string to = toDir + "/" + file.substr(file.find_last_of('/') + 1);
  if(rename(file.c_str(), to.c_str()) != 0)
    fail("cannot move " + file + " to " + to);
  logf("gatekeeper: moved %s to %s", file.c_str(), toDir.c_str());
}

// One gating: true when a candidate was found (and judged), false when there was none.
bool gateOnce(const Settings& s, int gamesPerGating, const Dirs& d, bool autoReject, uint64_t seed,
              const std::vector<coffee_start_position>& startPos) {
  time_t candTime = 0, baseTime = 0;
  const std::string cand = newestModelOrEmpty(d.test, &candTime);
  if(cand.empty())
    return false;
  const std::string candName = modelNameOf(cand);
  logf("gatekeeper: candidate %s", candName.c_str());
  const std::string base = newestModelOrEmpty(d.accepted, &baseTime);
  if(base.empty()) {
    logf("gatekeeper: no accepted model in %s", d.accepted.c_str());
    return false;
  }
  const std::string baseName = modelNameOf(base);
  if(baseTime > candTime && autoReject) {
    logf("gatekeeper: candidate %s is older than the accepted %s, rejected without playing", candName.c_str(),
         baseName.c_str());
    moveModel(cand, d.rejected);
    return true;
  }
  const int N = gamesPerGating, G = std::min(s.games, N), A = s.x * s.y;
  coffee_match_config c;
  memset(&c, 0, sizeof(c));
  c.x = s.x;
  c.y = s.y;
  c.win_len = s.winLen;
  c.num_games = G;
  c.seed = seed;
  c.slot_base = 0;
  c.commit_interval = 16;  // as `katago selfplay`
  c.model_path[0] = base.c_str();
  c.model_path[1] = cand.c_str();
  c.search = s.sp;
  c.nn_cache_log2 = s.nnCacheLog2;
  c.nn_precision = s.nnPrecision;
  coffee_match* h = nullptr;
  must(coffee_match_create(&c, &h), "create match engine");
  must(coffee_match_set_uncertainty(h, &s.unc), "set uncertainty");  // one setting for both nets
  must(coffee_match_set_exploration(h, -1, &s.ex), "set exploration");  // likewise
  must(coffee_match_set_root_search(h, -1, &s.rs), "set root search");
  if(s.unc.use_uncertainty)
    logf("gatekeeper: uncertainty weighting on for both nets: coeff %g, exponent %g, max weight %g",
         s.unc.uncertainty_coeff, s.unc.uncertainty_exponent, s.unc.uncertainty_max_weight);
  // opening variety that depends on neither net's policy (cli_startpos.h)
  if(!startPos.empty())
    must(coffee_match_set_start_positions(h, startPos.data(), (int)startPos.size(), &s.startPos.params),
         "set start positions");
  logf("gatekeeper: %s (candidate) against %s, %d games on %d slots, %dx%d win %d, %d visits", candName.c_str(),
       baseName.c_str(), N, G, s.x, s.y, s.winLen, s.sp.max_visits);
  const std::string sgfDir = d.sgf + "/" + candName;
  mkdirs(sgfDir);
  char name[64];
  snprintf(name, sizeof(name), "%016llX.sgfs", (unsigned long long)std::mt19937_64(seed ^ 0x5851F42D4C957F2DULL)());
  FILE* sgf = fopen((sgfDir + "/" + name).c_str(), "w");
  if(!sgf)
    fail("cannot write sgfs in " + sgfDir);
  std::vector<int32_t> hdr((size_t)2 * G * 5);
  std::vector<uint8_t> mv((size_t)2 * G * A * 2);
  double candPts = 0.0, basePts = 0.0;
  int tallied = 0;
  bool decided = false;
  while(!gQuit && tallied < N && !decided) {
    must(coffee_match_step(h, 128, nullptr), "step");
    int got = 0;
    must(coffee_match_drain_games(h, 2 * G, hdr.data(), mv.data(), &got), "drain games");
    for(int i = 0; i < got && tallied < N && !decided; i++) {
      const int32_t* r = hdr.data() + 5 * i;
      if((int64_t)r[1] * G + r[0] >= N)
        continue;  // a slot's games past the gating's total are played and not counted
      double cp = 0.0, bp = 0.0;
      must(coffee_match_score(r, 1, &cp, &bp), "score");
      candPts += cp;
      basePts += bp;
      tallied++;
      const bool candBlack = r[4] == 1;
      fputs(sgfGame(s.x, s.y, s.winLen, candBlack ? candName : baseName, candBlack ? baseName : candName, r,
                    mv.data() + (size_t)i * A * 2)
                .c_str(),
            sgf);
      logf("gatekeeper: game %d (slot %d, game %d): %s, candidate %s", tallied, r[0], r[1],
           r[3] == 0 ? "draw" : (r[3] == 1 ? "black wins" : "white wins"), candBlack ? "black" : "white");
      // the games still to come cannot change the verdict (the candidate wins ties)
      const int left = N - tallied;
      if(left > 0 && candPts >= basePts + left) {
        logf("gatekeeper: the candidate cannot lose any more, stopping after %d games", tallied);
        decided = true;
      } else if(left > 0 && basePts > candPts + left + 1e-10) {
        logf("gatekeeper: the candidate cannot win any more, stopping after %d games", tallied);
        decided = true;
      }
    }
  }
  fclose(sgf);
  coffee_match_stats st;
  must(coffee_match_stats_get(h, &st), "stats");
  logf("gatekeeper: %llu rounds, evaluations baseline %llu candidate %llu", (unsigned long long)st.rounds,
       (unsigned long long)st.nn_evals[0], (unsigned long long)st.nn_evals[1]);
  must(coffee_match_destroy(h), "destroy");
  if(gQuit)
    return true;  // interrupted: the candidate stays where it is
  if(basePts > candPts + 1e-10) {
    logf("gatekeeper: candidate %s rejected: score %.3f to %.3f in %d games", candName.c_str(), candPts, basePts,
         tallied);
    moveModel(cand, d.rejected);
  } else {
    logf("gatekeeper: candidate %s accepted: score %.3f to %.3f in %d games", candName.c_str(), candPts, basePts,
         tallied);
    if(!d.selfplay.empty())
      for(const char* sub : {"sgfs", "tdata", "vadata"})
        mkdirs(d.selfplay + "/" + candName + "/" + sub);
    moveModel(cand, d.accepted);
  }
  return true;
}

}  // namespace

int gatekeeperMain(int argc, char** argv) {
  Dirs d;
  std::string cfgPath, overrides;
  bool quitIfNone = false, autoReject = true;
  for(int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    auto next = [&]() -> std::string {
      if(i + 1 >= argc)
        fail("missing value for " + a);
      return argv[++i];
    };
    if(a == "-config")
      cfgPath = next();
    else if(a == "-test-models-dir")
      d.test = next();
    else if(a == "-accepted-models-dir")
      d.accepted = next();
    else if(a == "-rejected-models-dir")
      d.rejected = next();
    else if(a == "-sgf-output-dir")
      d.sgf = next();
    else if(a == "-selfplay-dir")
      d.selfplay = next();
    else if(a == "-quit-if-no-nets-to-test")
      quitIfNone = true;
    else if(a == "-no-autoreject-old-models")
      autoReject = false;
    else if(a == "-override-config")
      overrides = next();
    else
      fail("unknown argument " + a);
  }
  if(cfgPath.empty() || d.test.empty() || d.accepted.empty() || d.rejected.empty() || d.sgf.empty())
    fail("-config, -test-models-dir, -accepted-models-dir, -rejected-models-dir and -sgf-output-dir are required");
  std::map<std::string, std::string> kv;
  if(!readConfig(cfgPath, kv))
    fail("cannot read config " + cfgPath);
  std::stringstream os(overrides);
  std::string item;
  while(std::getline(os, item, ',')) {
    const size_t eq = item.find('=');
    if(eq != std::string::npos)
      kv[trim(item.substr(0, eq))] = trim(item.substr(eq + 1));
  }
  Settings s;
  s.games = 128;  // gatekeeper1.cfg numGameThreads
  coffee_match_params_default(&s.sp);
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  int gamesPerGating = 200;  // gatekeeper1.cfg numGamesPerGating
  try {
    applyConfig(kv, s);
    auto it = kv.find("numGamesPerGating");
    if(it != kv.end()) {
      size_t used = 0;
      gamesPerGating = std::stoi(it->second, &used);
      if(used != it->second.size())
        throw std::invalid_argument("config key numGamesPerGating: bad value '" + it->second + "'");
    }
  } catch(const std::invalid_argument& e) {
    fail(e.what());
  } catch(const std::exception&) {
    fail("config key numGamesPerGating: bad value");
  }
  if(gamesPerGating < 1 || s.games < 1)
    fail("numGamesPerGating and numGameThreads must be positive");
  mkdirs(d.sgf);
  mkdirs(d.rejected);
  char lname[64];
  time_t now = time(nullptr);
  strftime(lname, sizeof(lname), "log%Y%m%d-%H%M%S.log", localtime(&now));
  gLog = fopen((d.sgf + "/" + lname).c_str(), "w");
  {
    auto it = kv.find("allowResignation");
    if(it != kv.end() && (it->second == "true" || it->second == "True" || it->second == "1"))
      logf("gatekeeper: allowResignation is set: Coffee games have at most %d moves and are played out", s.x * s.y);
  }
  std::signal(SIGINT, onQuit);
  std::signal(SIGTERM, onQuit);
  // the run seed: `seed` in the config (or -override-config) repeats a run -- the gatings' engine
  // seeds and the startPosesLoadProb draws all come from it; unset, it is drawn and logged
  uint64_t runSeed = 0;
  {
    std::random_device rd;
    runSeed = rd() ^ ((uint64_t)rd() << 32);
    auto it = kv.find("seed");
    if(it != kv.end()) {
      char* end = nullptr;
      runSeed = strtoull(it->second.c_str(), &end, 10);
      if(it->second.empty() || *end != 0)
        fail("config key seed: bad value '" + it->second + "'");
    }
  }
  logf("gatekeeper: run seed %llu", (unsigned long long)runSeed);
  std::mt19937_64 seeds(runSeed);
  // the run's start positions: loaded and checked once, the same table for every gating
  std::vector<coffee_start_position> startPos;
  try {
    startPos = prepareStartPositions(s.startPos, s.x, s.y, s.winLen, runSeed, "gatekeeper",
                                     [](const std::string& m) { logf("%s", m.c_str()); });
  } catch(const std::exception& e) {
    fail(e.what());
  }
  while(!gQuit) {
    const uint64_t seed = seeds();
    if(!gateOnce(s, gamesPerGating, d, autoReject, seed, startPos)) {
      if(quitIfNone)
        break;
      for(int i = 0; i < 20 && !gQuit; i++)
        std::this_thread::sleep_for(std::chrono::milliseconds(200));
    }
  }
  logf("gatekeeper: done");
  if(gLog)
    fclose(gLog);
  gLog = nullptr;
  return 0;
}
