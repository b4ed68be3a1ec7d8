// `katago match` for Coffee on MI355X: plays two bots against each other -- two nets, or one
// net with two search settings -- and reports the result as a score, an Elo difference with its
// interval and the likelihood of superiority (the reference's command/match.cpp).  Host C++ over
// the C ABI's match engine with per-side settings (coffee_match_create2).
//
//   katago match -config <cfg> -sgf-output-dir <dir> [-log-file <file>] [-override-config k=v,...]
//
// Config (the reference's match_example.cfg): numBots (must be 2), botName0/1, nnModelFile0/1
// (or nnModelFile for both; none: the stand-in network), numGamesTotal, numGameThreads, seed,
// bSizes / winLen, nnPrecision, nnCacheSizePowerOfTwo, logGamesEvery, the start-position keys.
// Every search key of cli_config.h and the four uncertainty keys resolve per bot as key<i> over
// key over the default (coffee_match_params_default, uncertainty off).  The game-level settings
// (initGamesWithPolicy, policyInitAreaProp, policyInitAreaTemperature) are one per match: the
// unsuffixed keys; a bot that differs there is refused by the library.
// Equal model files turn share_net on: one network instance, one launch a round, one cache.
// Bot 1 is the match engine's side 1: black in game n of slot s iff s + n is even.
// numGamesTotal (N) games are played on G = min(numGameThreads, N) concurrent slots: game n of
// slot s counts iff n * G + s < N.  Every counted game is played out: there is no early stop.
// The games go to <sgf-output-dir>/<hex of the seed>.sgfs with PB / PW the bot names, the games
// of one drain in (game number, slot) order, so a seed repeats the file.  Every logGamesEvery
// games (default 50) and at the end one summary line gives bot 1's W-D-L, its split by colour,
// and score, Elo, interval and LOS from coffee_match_elo.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <sstream>
#include <string>
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
  fprintf(stderr, "katago match: %s\n", msg.c_str());
  exit(1);
}

void must(int rc, const char* what) {
  if(rc != COFFEE_OK)
    fail(std::string(what) + ": " + coffee_last_error());
}

int intKey(const std::map<std::string, std::string>& kv, const char* k, int def, bool required) {
  auto it = kv.find(k);
  if(it == kv.end()) {
    if(required)
      fail(std::string("config key ") + k + " is required");
    return def;
  }
  return ConfigReader::parseInt(k, it->second);
}

std::string eloText(double v) {
  if(std::isinf(v))
    return v > 0 ? "+inf" : "-inf";
  char b[32];
  snprintf(b, sizeof(b), "%+.1f", v);
  return b;
}

// Bot 1's results: wins, draws, losses in all and as black / as white.
struct Tally {
  int64_t w = 0, d = 0, l = 0, asBlack[3] = {0, 0, 0}, asWhite[3] = {0, 0, 0};
  void add(int winner, bool bot1Black) {
    const int k = winner == 0 ? 1 : ((winner == 1) == bot1Black ? 0 : 2);
    (k == 0 ? w : (k == 1 ? d : l))++;
    (bot1Black ? asBlack : asWhite)[k]++;
  }
  int64_t games() const { return w + d + l; }
};

void logSummary(const Tally& t, const MatchBot bots[2]) {
  double score = 0, elo = 0, lo = 0, hi = 0, los = 0;
  must(coffee_match_elo(t.w, t.d, t.l, &score, &elo, &lo, &hi, &los), "elo");
  logf("match: %s against %s after %lld games: W-D-L %lld-%lld-%lld (as black %lld-%lld-%lld, as white "
       "%lld-%lld-%lld), score %.4f, Elo %s [%s, %s], LOS %.1f%%",
       bots[1].name.c_str(), bots[0].name.c_str(), (long long)t.games(), (long long)t.w, (long long)t.d,
       (long long)t.l, (long long)t.asBlack[0], (long long)t.asBlack[1], (long long)t.asBlack[2],
       (long long)t.asWhite[0], (long long)t.asWhite[1], (long long)t.asWhite[2], score, eloText(elo).c_str(),
       eloText(lo).c_str(), eloText(hi).c_str(), 100.0 * los);
}

}  // namespace

int matchMain(int argc, char** argv) {
  std::string cfgPath, sgfDir, logFile, overrides;
  for(int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    auto next = [&]() -> std::string {
      if(i + 1 >= argc)
        fail("missing value for " + a);
      return argv[++i];
    };
    if(a == "-config")
      cfgPath = next();
    else if(a == "-sgf-output-dir")
      sgfDir = next();
    else if(a == "-log-file")
      logFile = next();
    else if(a == "-override-config")
      overrides = next();
    else
      fail("unknown argument " + a);
  }
  if(cfgPath.empty() || sgfDir.empty())
    // (with the program's own usage line, which names the commands' common form)
    fail("usage: katago match -config <cfg> -sgf-output-dir <dir> [-log-file <file>] [-override-config k=v,...]\n"
         "the other commands: usage: katago selfplay -config <cfg> -models-dir <dir> -output-dir <dir> "
         "[-max-games-total N] [-override-config k=v,...], katago gatekeeper, katago analysis");
  std::map<std::string, std::string> kv;
  if(!readConfig(cfgPath, kv))
    fail("cannot read config " + cfgPath);
  {
    std::stringstream os(overrides);
    std::string item;
    while(std::getline(os, item, ',')) {
      const size_t eq = item.find('=');
      if(eq != std::string::npos)
        kv[trim(item.substr(0, eq))] = trim(item.substr(eq + 1));
    }
  }
  Settings s;
  s.games = 128;
  coffee_match_params_default(&s.sp);
  coffee_uncertainty_params_default(&s.unc);
  coffee_exploration_params_default(&s.ex);
  const coffee_exploration_params defEx = s.ex;
  const coffee_search_params defSp = s.sp;
  const coffee_uncertainty_params defUnc = s.unc;
  MatchBot bots[2];
  int N = 0, logEvery = 50;
  try {
    applyConfig(kv, s);  // geometry, threads, cache, precision, start positions; s.sp: the game-level settings
    applyMatchBots(kv, defSp, defUnc, defEx, bots);
    N = intKey(kv, "numGamesTotal", 0, true);
    logEvery = intKey(kv, "logGamesEvery", 50, false);
  } catch(const std::invalid_argument& e) {
    fail(e.what());
  }
  if(N < 1 || s.games < 1 || logEvery < 1)
    fail("numGamesTotal, numGameThreads and logGamesEvery must be positive");
  mkdirs(sgfDir);
  if(logFile.empty()) {
    char lname[64];
    time_t now = time(nullptr);
    strftime(lname, sizeof(lname), "log%Y%m%d-%H%M%S.log", localtime(&now));
    logFile = sgfDir + "/" + lname;
  }
  gLog = fopen(logFile.c_str(), "w");
  if(!gLog)
    fail("cannot write the log file " + logFile);
  std::signal(SIGINT, onQuit);
  std::signal(SIGTERM, onQuit);
  uint64_t seed = 0;
  {
    std::random_device rd;
    seed = rd() ^ ((uint64_t)rd() << 32);
    auto it = kv.find("seed");
    if(it != kv.end()) {
      char* end = nullptr;
      seed = strtoull(it->second.c_str(), &end, 10);
      if(it->second.empty() || *end != 0)
        fail("config key seed: bad value '" + it->second + "'");
    }
  }
  logf("match: run seed %llu", (unsigned long long)seed);
  std::vector<coffee_start_position> startPos;
  try {
    startPos = prepareStartPositions(s.startPos, s.x, s.y, s.winLen, seed, "match",
                                     [](const std::string& m) { logf("%s", m.c_str()); });
  } catch(const std::exception& e) {
    fail(e.what());
  }
  const int G = std::min(s.games, N), A = s.x * s.y;
  const bool shared = bots[0].model == bots[1].model;
  coffee_match_config c;
  memset(&c, 0, sizeof(c));
  c.x = s.x;
  c.y = s.y;
  c.win_len = s.winLen;
  c.num_games = G;
  c.seed = seed;
  c.slot_base = 0;
  c.commit_interval = 16;  // as `katago selfplay`
  for(int i = 0; i < 2; i++)
    c.model_path[i] = bots[i].model.empty() ? nullptr : bots[i].model.c_str();
  c.search = s.sp;
  c.nn_cache_log2 = s.nnCacheLog2;
  c.nn_precision = s.nnPrecision;
  coffee_match_options o;
  memset(&o, 0, sizeof(o));
  o.per_side = 1;
  o.share_net = shared ? 1 : 0;
  for(int i = 0; i < 2; i++) {
    o.side[i].search = bots[i].sp;
    o.side[i].unc = bots[i].unc;
    logf("match: bot %d %s: model %s, %d visits, cpuct %g, uncertainty %s", i, bots[i].name.c_str(),
         bots[i].model.empty() ? "(stand-in network)" : bots[i].model.c_str(), bots[i].sp.max_visits,
         bots[i].sp.cpuct_exploration, bots[i].unc.use_uncertainty ? "on" : "off");
  }
  logf(shared ? "match: both bots use the same model file: the net is shared (one instance, one launch a round, "
                "one cache)"
              : "match: two model files: each bot's net has its own launch and cache");
  coffee_match* h = nullptr;
  must(coffee_match_create2(&c, &o, &h), "create match engine");
  for(int i = 0; i < 2; i++) {
    must(coffee_match_set_exploration(h, i, &bots[i].ex), "set exploration");
    must(coffee_match_set_root_search(h, i, &bots[i].rs), "set root search");
    if(bots[i].rs.wide_root_noise > 0.0f || bots[i].rs.futile_visits_threshold > 0.0f)
      logf("match: bot %d: wide root noise %g, futile visits threshold %g", i, bots[i].rs.wide_root_noise,
           bots[i].rs.futile_visits_threshold);
    if(bots[i].ex.use_noise_pruning || bots[i].ex.cpuct_utility_stdev_scale != 0.0f)
      logf("match: bot %d: cpuct stdev scale %g (prior %g, weight %g), noise pruning %s", i,
           bots[i].ex.cpuct_utility_stdev_scale, bots[i].ex.cpuct_utility_stdev_prior,
           bots[i].ex.cpuct_utility_stdev_prior_weight, bots[i].ex.use_noise_pruning ? "on" : "off");
  }
  if(!startPos.empty())
    must(coffee_match_set_start_positions(h, startPos.data(), (int)startPos.size(), &s.startPos.params),
         "set start positions");
  logf("match: %d games on %d slots, %dx%d win %d", N, G, s.x, s.y, s.winLen);
  char name[64];
  snprintf(name, sizeof(name), "%016llX.sgfs", (unsigned long long)std::mt19937_64(seed ^ 0x5851F42D4C957F2DULL)());
  FILE* sgf = fopen((sgfDir + "/" + name).c_str(), "w");
  if(!sgf)
    fail("cannot write sgfs in " + sgfDir);
  std::vector<int32_t> hdr((size_t)2 * G * 5);
  std::vector<uint8_t> mv((size_t)2 * G * A * 2);
  std::vector<int> order;
  Tally t;
  while(!gQuit && t.games() < N) {
    must(coffee_match_step(h, 128, nullptr), "step");
    int got = 0;
    must(coffee_match_drain_games(h, 2 * G, hdr.data(), mv.data(), &got), "drain games");
    // the games of one drain in (game number, slot) order: the order the device hands them out
    // within a commit is not fixed, their set is
    order.resize(got);
    for(int i = 0; i < got; i++)
      order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) {
      const int32_t *ra = hdr.data() + 5 * a, *rb = hdr.data() + 5 * b;
      return ra[1] != rb[1] ? ra[1] < rb[1] : ra[0] < rb[0];
    });
    for(int i : order) {
      const int32_t* r = hdr.data() + 5 * i;
      if((int64_t)r[1] * G + r[0] >= N)
        continue;  // a slot's games past the total are played and not counted
      const bool bot1Black = r[4] == 1;
      t.add(r[3], bot1Black);
      fputs(sgfGame(s.x, s.y, s.winLen, bots[bot1Black ? 1 : 0].name, bots[bot1Black ? 0 : 1].name, r,
                    mv.data() + (size_t)i * A * 2)
                .c_str(),
            sgf);
      if(t.games() % logEvery == 0 && t.games() < N)
        logSummary(t, bots);
    }
  }
  fclose(sgf);
  coffee_match_stats st;
  must(coffee_match_stats_get(h, &st), "stats");
  logf("match: %llu rounds, evaluations net 0 %llu net 1 %llu", (unsigned long long)st.rounds,
       (unsigned long long)st.nn_evals[0], (unsigned long long)st.nn_evals[1]);
  must(coffee_match_destroy(h), "destroy");
  if(t.games() > 0)
    logSummary(t, bots);
  logf(gQuit ? "match: interrupted" : "match: done");
  if(gLog)
    fclose(gLog);
  gLog = nullptr;
  return 0;
}
