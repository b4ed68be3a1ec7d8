// Config-file layer of `katago selfplay` (cli_selfplay.cpp): KataGo-style `key = value`
// files (the reference's ConfigParser, core/config_parser.cpp, restricted to what this
// path reads) mapped onto Settings.  Host-only and header-only so the sanitizer build
// (tests/san, tests/test_sanitizers.py) checks the same code the CLI runs.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstdlib>
#include <fstream>
#include <map>
#include <stdexcept>
#include <string>

#include "../../include/katacoffee.h"

namespace kccli {

inline std::string trim(const std::string& s) {
  size_t a = s.find_first_not_of(" \t\r\n"), b = s.find_last_not_of(" \t\r\n");
  return a == std::string::npos ? "" : s.substr(a, b - a + 1);
}

inline bool readConfig(const std::string& path, std::map<std::string, std::string>& kv) {
  std::ifstream in(path);
  if(!in)
    return false;
  std::string line;
  while(std::getline(in, line)) {
    size_t h = line.find('#');
    if(h != std::string::npos)
      line = line.substr(0, h);
    size_t eq = line.find('=');
    if(eq == std::string::npos)
      continue;
    std::string k = trim(line.substr(0, eq)), v = trim(line.substr(eq + 1));
    if(!k.empty())
      kv[k] = v;
  }
  return true;
}

// startPosesFromSgfDir / startPosesFile / startPosesLoadProb and the library's parameters
// (startPosesProb, startPosesTurnWeightLambda, startPosesPolicyInitAreaProp): cli_startpos.h
struct StartPosSettings {
  std::string sgfDirs, file;
  float loadProb = 1.0f;
  coffee_start_positions_params params = {0.0f, 0.0f, 0.0f};
};

struct Settings {
  int x = 5, y = 5, winLen = 4, games = 4096, gpus = 1, maxRowsPerFile = 10000;
  int servers = 1;  // numNNServerThreadsPerModel: self-play engines (own stream, batch, cache) over all GPUs
  float modelPollSeconds = 10.0f;
  int nnCacheLog2 = 21;  // selfplay1.cfg:121 nnCacheSizePowerOfTwo
  // nnPrecision = auto | corrected | accurate | fast | fastLayered (the reference's useFP16,
  // whose default Auto is mapped to the path within 1e-3 of fp32: corrected / accurate)
  int nnPrecision = COFFEE_NN_DEFAULT;
  int64_t maxGamesTotal = -1;
  uint64_t seed = 0;
  coffee_search_params sp;
  // useUncertainty & co: like sp, set to the library's defaults (coffee_uncertainty_params_default:
  // off) by the command before applyConfig; off unless the config turns it on, for all three
  // commands (the reference's loader defaults it on for analysis, GTP and match, setup.cpp:539-562)
  coffee_uncertainty_params unc;
  // cpuctUtilityStdevScale, useNoisePruning & co: like unc, the library's defaults
  // (coffee_exploration_params_default: both off) unless the config turns them on, for all four
  // commands (the reference's loader defaults them on for analysis, GTP and match, setup.cpp:453-537)
  coffee_exploration_params ex = {0, 0.15f, FLT_MAX, 0.40f, 2.0f, 0.0f};
  // wideRootNoise, futileVisitsThreshold: off unless the config sets them, for all
  // four commands (the reference's loader defaults wideRootNoise to 0.04 for analysis, setup.cpp:725-730)
  coffee_root_search_params rs = {0.0f, 0.0f};
  // rootSymmetryPruning (`katago analysis` only): off unless the config turns it on -- the
  // reference's loader defaults it on for analysis and GTP (setup.cpp:639-644)
  int32_t rootSymmetryPruning = 0;
  // numSearchThreadsPerAnalysisThread (alias numSearchThreads) and numVirtualLossesPerThread
  // (DESIGN.md 8j), read by `katago analysis` alone (applySearchThreadsConfig): one playout a
  // round unless the config asks for more (the reference's analysis example sets 16)
  int searchThreads = 1;
  float virtualLossesPerThread = 1.0f;
  StartPosSettings startPos;  // off unless startPosesProb > 0 and a source is named
};

// The typed lookups of a config map.  suffix (the `katago match` bot index, "0" / "1"; empty:
// none): a key is read as key<suffix> where the file has that, else as the plain key -- the
// reference's precedence for per-bot search keys (Setup::loadParams, setup.cpp).
struct ConfigReader {
  const std::map<std::string, std::string>& kv;
  std::string suffix;
  // the entry a key resolves to (kv.end(): absent); name: the key as the file spells it
  std::map<std::string, std::string>::const_iterator find(const char* k, std::string& name) const {
    if(!suffix.empty()) {
      auto it = kv.find(k + suffix);
      if(it != kv.end()) {
        name = k + suffix;
        return it;
      }
    }
    name = k;
    return kv.find(k);
  }
  bool has(const char* k) const {
    std::string n;
    return find(k, n) != kv.end();
  }
  // a value that is not a whole number of the key's type is an error naming the key
  // (the reference's ConfigParser::getInt / getFloat throw IOError the same way)
  static std::invalid_argument bad(const std::string& k, const std::string& v) {
    return std::invalid_argument("config key " + k + ": bad value '" + v + "'");
  }
  static int parseInt(const std::string& k, const std::string& v) {
    size_t used = 0;
    int r = 0;
    try {
      r = std::stoi(v, &used);
    } catch(const std::exception&) {
      throw bad(k, v);
    }
    if(used != v.size())
      throw bad(k, v);
    return r;
  }
  void geti(const char* k, int& v) const {
    std::string n;
    auto it = find(k, n);
    if(it != kv.end())
      v = parseInt(n, it->second);
  }
  void getf(const char* k, float& v) const {
    std::string n;
    auto it = find(k, n);
    if(it == kv.end())
      return;
    size_t used = 0;
    try {
      v = std::stof(it->second, &used);
    } catch(const std::exception&) {
      throw bad(n, it->second);
    }
    if(used != it->second.size())
      throw bad(n, it->second);
  }
  void getb(const char* k, int32_t& v) const {
    std::string n;
    auto it = find(k, n);
    if(it != kv.end())
      v = (it->second == "true" || it->second == "True" || it->second == "1") ? 1 : 0;
  }
  // a value outside [lo, hi] (NaN included) is an error naming the key, like
  // ConfigParser::getDouble(key, min, max)
  void getfIn(const char* k, float& v, float lo, float hi) const {
    std::string n;
    if(find(k, n) == kv.end())
      return;
    getf(k, v);
    if(!(v >= lo && v <= hi))
      throw std::invalid_argument("config key " + n + ": value " + std::to_string(v) + " outside [" +
                                  std::to_string(lo) + ", " + std::to_string(hi) + "]");
  }
  void gets(const char* k, std::string& v) const {
    std::string n;
    auto it = find(k, n);
    if(it != kv.end())
      v = it->second;
  }
};

// The search keys and the four uncertainty keys onto p / unc (r.suffix: the bot of `katago match`).
inline void applySearchConfig(const ConfigReader& r, coffee_search_params& p, coffee_uncertainty_params& unc) {
  r.geti("maxVisits", p.max_visits);
  r.getf("cpuctExploration", p.cpuct_exploration);
  r.getf("cpuctExplorationLog", p.cpuct_exploration_log);
  r.getf("cpuctExplorationBase", p.cpuct_exploration_base);
  r.getf("fpuReductionMax", p.fpu_reduction_max);
  r.getf("rootFpuReductionMax", p.root_fpu_reduction_max);
  r.getf("fpuLossProp", p.fpu_loss_prop);
  r.getf("rootFpuLossProp", p.root_fpu_loss_prop);
  r.getb("fpuParentWeightByVisitedPolicy", p.fpu_parent_weight_by_visited_policy);
  r.getf("fpuParentWeightByVisitedPolicyPow", p.fpu_parent_weight_by_visited_policy_pow);
  r.getf("valueWeightExponent", p.value_weight_exponent);
  r.getb("rootNoiseEnabled", p.root_noise_enabled);
  r.getf("rootDirichletNoiseTotalConcentration", p.root_dirichlet_noise_total_concentration);
  r.getf("rootDirichletNoiseWeight", p.root_dirichlet_noise_weight);
  r.getf("rootPolicyTemperature", p.root_policy_temperature);
  r.getf("rootPolicyTemperatureEarly", p.root_policy_temperature_early);
  r.getf("rootDesiredPerChildVisitsCoeff", p.root_desired_per_child_visits_coeff);
  r.geti("rootNumSymmetriesToSample", p.root_num_symmetries_to_sample);
  r.getf("chosenMoveTemperature", p.chosen_move_temperature);
  r.getf("chosenMoveTemperatureEarly", p.chosen_move_temperature_early);
  r.getf("chosenMoveTemperatureHalflife", p.chosen_move_temperature_halflife);
  r.getf("chosenMoveSubtract", p.chosen_move_subtract);
  r.getf("chosenMovePrune", p.chosen_move_prune);
  r.getb("useLcbForSelection", p.use_lcb_for_selection);
  r.getf("lcbStdevs", p.lcb_stdevs);
  r.getf("minVisitPropForLCB", p.min_visit_prop_for_lcb);
  r.getf("subtreeValueBiasFactor", p.subtree_value_bias_factor);
  r.getf("subtreeValueBiasWeightExponent", p.subtree_value_bias_weight_exponent);
  r.getf("subtreeValueBiasFreeProp", p.subtree_value_bias_free_prop);
  r.getb("useGraphSearch", p.use_graph_search);
  // PlaySettings (playsettings.cpp:80-99)
  r.getf("cheapSearchProb", p.cheap_search_prob);
  r.geti("cheapSearchVisits", p.cheap_search_visits);
  r.getf("cheapSearchTargetWeight", p.cheap_search_target_weight);
  r.getb("reduceVisits", p.reduce_visits);
  r.getf("reduceVisitsThreshold", p.reduce_visits_threshold);
  r.geti("reduceVisitsThresholdLookback", p.reduce_visits_threshold_lookback);
  r.geti("reducedVisitsMin", p.reduced_visits_min);
  r.getf("reducedVisitsWeight", p.reduced_visits_weight);
  r.getf("policySurpriseDataWeight", p.policy_surprise_data_weight);
  r.getf("valueSurpriseDataWeight", p.value_surprise_data_weight);
  r.getb("initGamesWithPolicy", p.init_games_with_policy);
  r.getf("policyInitAreaProp", p.policy_init_area_prop);
  r.getf("policyInitAreaTemperature", p.policy_init_area_temperature);
  r.getf("earlyForkGameProb", p.early_fork_game_prob);
  r.getf("earlyForkGameExpectedMoveProp", p.early_fork_game_expected_move_prop);
  r.getf("forkGameProb", p.fork_game_prob);
  r.geti("forkGameMinChoices", p.fork_game_min_choices);
  r.geti("earlyForkGameMaxChoices", p.early_fork_game_max_choices);
  r.geti("forkGameMaxChoices", p.fork_game_max_choices);
  r.getf("sidePositionProb", p.side_position_prob);
  // PlaySettings fields the reference's loader never reads (playsettings.cpp:14): accepted
  // here so the recording can be switched on from a config
  r.getb("recordTreePositions", p.record_tree_positions);
  r.geti("recordTreeThreshold", p.record_tree_threshold);
  r.getf("recordTreeTargetWeight", p.record_tree_target_weight);
  // uncertainty weighting, with the reference's ranges (setup.cpp:539-562)
  r.getb("useUncertainty", unc.use_uncertainty);
  r.getfIn("uncertaintyCoeff", unc.uncertainty_coeff, 0.0001f, 1.0f);
  r.getfIn("uncertaintyExponent", unc.uncertainty_exponent, 0.0f, 2.0f);
  r.getfIn("uncertaintyMaxWeight", unc.uncertainty_max_weight, 1.0f, 100.0f);
}

// The six exploration keys onto ex, with the reference's ranges (setup.cpp:453-470, :520-537;
// r.suffix: the bot of `katago match`).  A noisePruningCap above FLT_MAX (the reference's default
// is 1e50) is stored as FLT_MAX.
inline void applyExplorationConfig(const ConfigReader& r, coffee_exploration_params& ex) {
  r.getfIn("cpuctUtilityStdevPrior", ex.cpuct_utility_stdev_prior, 0.0f, 10.0f);
  r.getfIn("cpuctUtilityStdevPriorWeight", ex.cpuct_utility_stdev_prior_weight, 0.0f, 100.0f);
  r.getfIn("cpuctUtilityStdevScale", ex.cpuct_utility_stdev_scale, 0.0f, 1.0f);
  r.getb("useNoisePruning", ex.use_noise_pruning);
  r.getfIn("noisePruneUtilityScale", ex.noise_prune_utility_scale, 0.001f, 10.0f);
  {
    std::string n;
    auto it = r.find("noisePruningCap", n);
    if(it != r.kv.end()) {
      char* end = nullptr;
      const double c = strtod(it->second.c_str(), &end);
      if(it->second.empty() || end != it->second.c_str() + it->second.size())
        throw ConfigReader::bad(n, it->second);
      if(!(c >= 0.0))
        throw std::invalid_argument("config key " + n + ": value " + it->second + " outside [0, inf)");
      ex.noise_pruning_cap = c > (double)FLT_MAX ? FLT_MAX : (float)c;
    }
  }
  if(ex.cpuct_utility_stdev_prior == 0.0f && ex.cpuct_utility_stdev_scale > 0.0f)
    throw std::invalid_argument("config key cpuctUtilityStdevPrior" + r.suffix +
                                ": must be > 0 with cpuctUtilityStdevScale > 0");
}

// The two root-search keys onto rs, with the reference's ranges (setup.cpp:725-730, :843-848;
// r.suffix: the bot of `katago match`).
inline void applyRootSearchConfig(const ConfigReader& r, coffee_root_search_params& rs) {
  r.getfIn("wideRootNoise", rs.wide_root_noise, 0.0f, 5.0f);
  r.getfIn("futileVisitsThreshold", rs.futile_visits_threshold, 0.01f, 1.0f);
}

// The parallel-playout keys: numSearchThreadsPerAnalysisThread in 1..32, under its
// short name numSearchThreads where the file has only that, and numVirtualLossesPerThread with
// the reference's range (setup.cpp: 0.01 to 1000).  `katago analysis` alone calls this, after
// applyConfig: the other commands make one playout a round and go on ignoring the keys, which the
// reference's self-play, match and gatekeeper configs carry with values of their own.
inline void applySearchThreadsConfig(const ConfigReader& r, int& threads, float& perThread) {
  const char* key = r.has("numSearchThreadsPerAnalysisThread") ? "numSearchThreadsPerAnalysisThread" : "numSearchThreads";
  r.geti(key, threads);
  if(threads < 1 || threads > COFFEE_SEARCH_THREADS_MAX)
    throw std::invalid_argument(std::string("config key ") + key + ": value " + std::to_string(threads) +
                                " outside [1, " + std::to_string(COFFEE_SEARCH_THREADS_MAX) + "]");
  r.getfIn("numVirtualLossesPerThread", perThread, 0.01f, 1000.0f);
}

inline void applyConfig(const std::map<std::string, std::string>& kv, Settings& s) {
  const ConfigReader r{kv, ""};
  auto it = kv.find("bSizes");
  if(it != kv.end())
    s.x = s.y = ConfigReader::parseInt("bSizes", trim(it->second.substr(0, it->second.find(','))));
  r.geti("boardXLen", s.x);
  r.geti("boardYLen", s.y);
  r.geti("winLen", s.winLen);
  r.geti("numGameThreads", s.games);
  r.geti("numGamesPerGpu", s.games);
  r.geti("numGpus", s.gpus);
  r.geti("numNNServerThreadsPerModel", s.servers);
  r.geti("maxRowsPerTrainFile", s.maxRowsPerFile);
  r.getf("modelPollSeconds", s.modelPollSeconds);
  r.geti("nnCacheSizePowerOfTwo", s.nnCacheLog2);  // setup.cpp:268; <= 0 disables the cache
  s.nnCacheLog2 = std::max(0, s.nnCacheLog2);
  it = kv.find("nnPrecision");
  if(it != kv.end()) {
    if(it->second == "auto")
      s.nnPrecision = COFFEE_NN_DEFAULT;
    else if(it->second == "fast")
      s.nnPrecision = COFFEE_NN_FAST;
    else if(it->second == "accurate")
      s.nnPrecision = COFFEE_NN_ACCURATE;
    else if(it->second == "fastLayered")
      s.nnPrecision = COFFEE_NN_FAST_LAYERED;
    else if(it->second == "corrected")
      s.nnPrecision = COFFEE_NN_CORRECTED;
    else
      throw std::invalid_argument("nnPrecision must be auto, corrected, accurate, fast or fastLayered");
  }
  applySearchConfig(r, s.sp, s.unc);
  applyExplorationConfig(r, s.ex);
  applyRootSearchConfig(r, s.rs);
  r.getb("rootSymmetryPruning", s.rootSymmetryPruning);
  // start positions (play.cpp:186-196 getters: the same ranges)
  r.gets("startPosesFromSgfDir", s.startPos.sgfDirs);
  r.gets("startPosesFile", s.startPos.file);
  r.getfIn("startPosesProb", s.startPos.params.prob, 0.0f, 1.0f);
  r.getfIn("startPosesLoadProb", s.startPos.loadProb, 0.0f, 1.0f);
  r.getfIn("startPosesTurnWeightLambda", s.startPos.params.turn_weight_lambda, -10.0f, 10.0f);
  r.getfIn("startPosesPolicyInitAreaProp", s.startPos.params.start_policy_init_area_prop, 0.0f, 1.0f);
}


// `katago match` (cli_match.cpp): the two bots of a match config, as the reference's
// match_example.cfg names them.  Every search key and the four uncertainty keys resolve as
// key<i> over key over the default the caller put into `def`; nnModelFile<i> over nnModelFile.
struct MatchBot {
  std::string name, model;
  coffee_search_params sp;
  coffee_uncertainty_params unc;
  coffee_exploration_params ex;  // the six exploration keys, per bot like every search key
  coffee_root_search_params rs;  // wideRootNoise / futileVisitsThreshold, likewise (off unless set)
};

inline void applyMatchBots(const std::map<std::string, std::string>& kv, const coffee_search_params& defSp,
                           const coffee_uncertainty_params& defUnc, const coffee_exploration_params& defEx,
                           MatchBot bots[2]) {
  {
    auto it = kv.find("numBots");
    if(it != kv.end() && ConfigReader::parseInt("numBots", it->second) != 2)
      throw std::invalid_argument("config key numBots: this command plays exactly 2 bots, numBots must be 2 (got " +
                                  it->second + ")");
  }
  for(int i = 0; i < 2; i++) {
    const ConfigReader r{kv, std::to_string(i)};
    bots[i].sp = defSp;
    bots[i].unc = defUnc;
    applySearchConfig(r, bots[i].sp, bots[i].unc);
    bots[i].ex = defEx;
    applyExplorationConfig(r, bots[i].ex);
    bots[i].rs = coffee_root_search_params{0.0f, 0.0f};
    applyRootSearchConfig(r, bots[i].rs);
    bots[i].name = "bot" + std::to_string(i);
    r.gets("botName", bots[i].name);
    bots[i].model.clear();
    r.gets("nnModelFile", bots[i].model);
  }
}

// (exploration from the library's defaults: both mechanisms off)
inline void applyMatchBots(const std::map<std::string, std::string>& kv, const coffee_search_params& defSp,
                           const coffee_uncertainty_params& defUnc, MatchBot bots[2]) {
  coffee_exploration_params defEx;
  coffee_exploration_params_default(&defEx);
  applyMatchBots(kv, defSp, defUnc, defEx, bots);
}

}  // namespace kccli
